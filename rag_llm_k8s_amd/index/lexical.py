"""Lexical (BM25) index next to the dense one: the analyzer, the resident CSR, and reciprocal rank fusion.

Analyzer -- one fixed function over the UTF-8 bytes of a text, no language knowledge:
  * a token is a maximal run of bytes that are ASCII letters, ASCII digits or >= 0x80; ASCII upper case is
    lowered, nothing else is folded, stemmed or stopped;
  * the term id is the 32-bit FNV-1a of the token's bytes, 0xFFFFFFFF remapped to 0xFFFFFFFE (the padding id);
    collisions are accepted;
  * a document yields its distinct term ids ascending, their counts (tf, saturating at 65535) and its length in
    tokens; a query keeps its first 64 distinct terms in order of appearance.
The C++ implementation lives in the `_ragk_rt` runtime (csrc/runtime/lexical.h, GIL released); `py_analyze_batch`
is its pure-Python twin with the same output -- the fallback when the runtime is not built, and the oracle.

LexicalIndex -- a doc-major CSR of (term, tf) entries plus doc_len on the store's device (torch tensors: CPU
memory or HBM). Row i is metadata entry i, so its ids are the dense index's ids. It is not persisted: the store
rebuilds it from the metadata texts. Search = ops lex_df (live document frequencies) -> idf / avgdl on the host
in float64 numpy -> ops lex_search (csrc/kernels/lexical.hip on the GPU, ops/reference.py on the CPU).
"""
from __future__ import annotations

import re
import threading

import numpy as np
import torch

from .flat import check_keep, masks_device, masks_host, pack_masks

PAD_TERM = 0xFFFFFFFF
QUERY_MAX_TERMS = 64    # distinct terms kept per query
LAUNCH_MAX_QUERIES = 64  # queries per lex_search launch (one membership bit each)
_TOKEN = re.compile(rb"[0-9A-Za-z\x80-\xff]+")


# ---------------------------------------------------------------------------------------- analyzer
def lex_remap(h: int) -> int:
    """The padding id never names a term."""
    return 0xFFFFFFFE if h == PAD_TERM else h


def fnv1a32(token: bytes) -> int:
    h = 2166136261
    for c in token:
        h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    return h


def _utf8(text) -> bytes:
    if isinstance(text, bytes):
        return text
    return str(text).encode("utf-8", "replace")


def py_tokens(text, cache=None) -> list:
    """Term id of every token, in order of appearance (pure Python)."""
    cache = {} if cache is None else cache
    out = []
    for tok in _TOKEN.findall(_utf8(text).lower()):  # bytes.lower() lowers ASCII only
        h = cache.get(tok)
        if h is None:
            h = cache[tok] = lex_remap(fnv1a32(tok))
        out.append(h)
    return out


def py_analyze_batch(texts):
    """Pure-Python twin of the runtime's lex_analyze_batch: (row_ptr int64 [n + 1], terms uint32, tf uint16,
    doc_len int32 [n])."""
    row_ptr, terms, tfs, dls = [0], [], [], []
    cache = {}
    for t in texts:
        toks = py_tokens(t, cache)
        dls.append(min(len(toks), 0x7FFFFFFF))
        if toks:
            u, c = np.unique(np.asarray(toks, dtype=np.uint32), return_counts=True)
            terms.append(u)
            tfs.append(np.minimum(c, 65535).astype(np.uint16))
        row_ptr.append(row_ptr[-1] + (len(terms[-1]) if toks else 0))
    return (np.asarray(row_ptr, dtype=np.int64),
            np.concatenate(terms) if terms else np.zeros(0, np.uint32),
            np.concatenate(tfs) if tfs else np.zeros(0, np.uint16),
            np.asarray(dls, dtype=np.int32))


def analyze_batch(texts, use_native=True):
    """A batch of texts -> CSR arrays, by the C++ runtime when it is built (else the Python twin)."""
    data = [_utf8(t) for t in texts]
    rt = None
    if use_native:
        from ..runtime import native_rt

        rt = native_rt()
    if rt is not None and hasattr(rt, "lex_analyze_batch"):
        rp, te, tf, dl = rt.lex_analyze_batch(data)
        return (np.asarray(rp, np.int64), np.asarray(te, np.uint32), np.asarray(tf, np.uint16),
                np.asarray(dl, np.int32))
    return py_analyze_batch(data)


def query_terms(text) -> list:
    """The first QUERY_MAX_TERMS distinct term ids of a query, in order of appearance."""
    return list(dict.fromkeys(py_tokens(text)))[:QUERY_MAX_TERMS]


def doc_text(meta) -> str:
    """The text a metadata entry contributes: an entry that is no dict or has no "text" is an empty document."""
    if isinstance(meta, dict):
        t = meta.get("text")
        if isinstance(t, (str, bytes)):
            return t
    return ""


# ---------------------------------------------------------------------------------------- host-side numbers
def launch_table(queries):
    """queries: <= 64 lists of term ids -> (sorted distinct term ids uint32 [T], membership words uint64 [T]:
    bit q set = query q holds the term)."""
    if len(queries) > LAUNCH_MAX_QUERIES:
        raise ValueError("at most %d queries per launch" % LAUNCH_MAX_QUERIES)
    words = {}
    for q, ts in enumerate(queries):
        for t in ts:
            words[int(t)] = words.get(int(t), 0) | (1 << q)
    terms = sorted(words)
    return np.asarray(terms, dtype=np.uint32), np.asarray([words[t] for t in terms], dtype=np.uint64)


def bm25_idf(df, n_live) -> np.ndarray:
    """float32(log1p((n_live - df + 0.5) / (df + 0.5))) in float64 numpy: the one idf both backends use."""
    df = np.asarray(df, dtype=np.float64)
    return np.log1p((float(n_live) - df + 0.5) / (df + 0.5)).astype(np.float32)


def rrf_fuse(lists, rrf_k, k):
    """Reciprocal rank fusion in float64: fused(d) = sum over the lists that hold d of 1 / (rrf_k + rank), rank
    1-based. lists: ranked id sequences (best first; ids < 0 are padding and are skipped without taking a rank
    from the ids after them -- padding only ever ends a list). Returns [(id, fused)] by fused descending, then
    id ascending, cut to k."""
    fused = {}
    for ids in lists:
        rank = 0
        for d in ids:
            d = int(d)
            if d < 0:
                continue
            rank += 1
            fused[d] = fused.get(d, 0.0) + 1.0 / (float(rrf_k) + rank)
    return sorted(fused.items(), key=lambda kv: (-kv[1], kv[0]))[:k]


# ---------------------------------------------------------------------------------------- the index
class LexicalIndex:
    def __init__(self, device="cpu", capacity=1024, entry_capacity=1 << 16):
        self.device = torch.device(device)
        self.ntotal = 0
        self.nnz = 0
        self._cap = max(1, int(capacity))
        self._ecap = max(1, int(entry_capacity))
        self._lock = threading.RLock()
        self._row_ptr = torch.zeros(self._cap + 1, dtype=torch.int64, device=self.device)
        self._terms = torch.zeros(self._ecap, dtype=torch.int32, device=self.device)  # uint32 bit patterns
        self._tf = torch.zeros(self._ecap, dtype=torch.int16, device=self.device)     # uint16 bit patterns
        self._doc_len = torch.zeros(self._cap, dtype=torch.int32, device=self.device)
        self._dl_host = np.zeros(self._cap, dtype=np.int32)  # host mirror: avgdl of the live set without a sync
        from ..ops.backend import get_backend

        self._be = get_backend(self.device)

    # ---------------------------------------------------------------- mutation
    def _grow(self, need_docs, need_entries):
        if need_docs > self._cap:
            cap = max(need_docs, 2 * self._cap)
            rp = torch.zeros(cap + 1, dtype=torch.int64, device=self.device)
            rp[:self.ntotal + 1] = self._row_ptr[:self.ntotal + 1]
            dl = torch.zeros(cap, dtype=torch.int32, device=self.device)
            dl[:self.ntotal] = self._doc_len[:self.ntotal]
            dh = np.zeros(cap, dtype=np.int32)
            dh[:self.ntotal] = self._dl_host[:self.ntotal]
            self._row_ptr, self._doc_len, self._dl_host, self._cap = rp, dl, dh, cap
        if need_entries > self._ecap:
            ecap = max(need_entries, 2 * self._ecap)
            te = torch.zeros(ecap, dtype=torch.int32, device=self.device)
            te[:self.nnz] = self._terms[:self.nnz]
            tf = torch.zeros(ecap, dtype=torch.int16, device=self.device)
            tf[:self.nnz] = self._tf[:self.nnz]
            self._terms, self._tf, self._ecap = te, tf, ecap

    def add(self, texts, use_native=True):
        """Append one document per text (analysed on the host, C++ when built)."""
        texts = list(texts)
        if not texts:
            return
        rp, te, tf, dl = analyze_batch(texts, use_native=use_native)
        m, e = len(texts), len(te)
        with self._lock:
            n0, e0 = self.ntotal, self.nnz
            self._grow(n0 + m, e0 + e)
            self._row_ptr[n0 + 1:n0 + m + 1] = torch.from_numpy(rp[1:] + e0).to(self.device)
            if e:
                self._terms[e0:e0 + e] = torch.from_numpy(te.view(np.int32)).to(self.device)
                self._tf[e0:e0 + e] = torch.from_numpy(tf.view(np.int16)).to(self.device)
            self._doc_len[n0:n0 + m] = torch.from_numpy(dl).to(self.device)
            self._dl_host[n0:n0 + m] = dl
            self.ntotal, self.nnz = n0 + m, e0 + e

    def reset(self):
        with self._lock:
            self.ntotal = self.nnz = 0

    def compact(self, keep):
        """Drop every document whose id is not in `keep` (sorted ids): afterwards the index equals a fresh one
        built from the kept documents in their original order (new id = rank among the kept)."""
        with self._lock:
            keep = check_keep(keep, self.ntotal)
            if len(keep) == self.ntotal:
                return
            kt = torch.from_numpy(keep).to(self.device)
            rp = self._row_ptr[:self.ntotal + 1]
            lens = (rp[1:] - rp[:-1])[kt]
            nrp = torch.zeros(len(keep) + 1, dtype=torch.int64, device=self.device)
            nrp[1:] = torch.cumsum(lens, 0)
            e = int(nrp[-1])
            if e:
                src = torch.repeat_interleave(rp[:-1][kt] - nrp[:-1], lens) + torch.arange(e, device=self.device)
                self._terms[:e] = self._terms[src]  # the right-hand side is gathered before the write
                self._tf[:e] = self._tf[src]
            self._row_ptr[:len(keep) + 1] = nrp
            self._doc_len[:len(keep)] = self._doc_len[kt]
            self._dl_host[:len(keep)] = self._dl_host[keep]
            self.ntotal, self.nnz = len(keep), e

    # ---------------------------------------------------------------- query
    def live_stats(self, live=None):
        """(n_live, avgdl float32) of the live documents (live: bool [ntotal] or None = all)."""
        dl = self._dl_host[:self.ntotal]
        if live is not None:
            dl = dl[np.asarray(live, dtype=bool)[:self.ntotal]]
        n_live = int(len(dl))
        total = int(dl.astype(np.int64).sum())
        avgdl = np.float32(total / n_live) if total else np.float32(1.0)  # no tokens at all: nothing can match
        return n_live, float(avgdl)

    def search(self, queries, k, k1=1.2, b=0.75, masks=None, qmask=None, live=None):
        """queries: per query a string or a list of term ids -> (scores fp32 [nq, k] descending, ids int64
        [nq, k]) on the host; ties -> lower id, padding (0, -1). live: bool [ntotal] -- the documents that count
        for df / avgdl (None = all); masks / qmask: the per-query id bitmaps of the dense search (a deleted
        document must also be masked there to stay out of the results). More than 64 queries are cut into
        launches."""
        qts = [query_terms(q) if isinstance(q, (str, bytes)) else list(q)[:QUERY_MAX_TERMS] for q in queries]
        nq = len(qts)
        S = torch.zeros((nq, k), dtype=torch.float32)
        I = torch.full((nq, k), -1, dtype=torch.int64)
        if not 1 <= k <= 64:
            raise ValueError("lexical search: 1 <= k <= 64")
        if (masks is None) != (qmask is None):
            raise ValueError("masks and qmask go together")
        with self._lock:
            n = self.ntotal
            if nq == 0 or n == 0:
                return S, I
            n_live, avgdl = self.live_stats(live)
            live_row = None
            if live is not None:
                live_row = torch.from_numpy(pack_masks(np.asarray(live, dtype=bool)[:n])[0].view(np.int32))
            cuda = self.device.type == "cuda"
            md = None
            if masks is not None:
                md = masks_device(masks, self.device) if cuda else torch.from_numpy(masks_host(masks).view(np.int32))
                qm_all = np.asarray(qmask.cpu() if isinstance(qmask, torch.Tensor) else qmask, dtype=np.int32).reshape(-1)
                if len(qm_all) != nq:
                    raise ValueError("qmask: one entry per query")
            k1f, bf = np.float32(k1), np.float32(b)
            k1p1 = np.float32(k1f + np.float32(1.0))
            for q0 in range(0, nq, LAUNCH_MAX_QUERIES):
                part = qts[q0:q0 + LAUNCH_MAX_QUERIES]
                terms, member = launch_table(part)
                if len(terms) == 0:
                    continue
                qt = torch.from_numpy(terms.view(np.int32))
                df = self._be.lex_df(self._row_ptr, self._terms, n, qt, live=live_row).cpu().numpy()
                idf = torch.from_numpy(bm25_idf(df, n_live))
                qm = torch.from_numpy(qm_all[q0:q0 + len(part)].copy()) if md is not None else None
                s, i = self._be.lex_search(self._row_ptr, self._terms, self._tf, self._doc_len, n, qt, idf,
                                           torch.from_numpy(member.view(np.int64)), len(part), float(k1f),
                                           float(k1p1), float(bf), avgdl, k, masks=md, qmask=qm)
                S[q0:q0 + len(part)] = s.cpu()
                I[q0:q0 + len(part)] = i.cpu()
        return S, I

    # ---------------------------------------------------------------- introspection
    def state(self):
        """The live part of the CSR on the host (tests: two indexes are equal iff their states are)."""
        with self._lock:
            n, e = self.ntotal, self.nnz
            return {"row_ptr": self._row_ptr[:n + 1].cpu(), "terms": self._terms[:e].cpu(), "tf": self._tf[:e].cpu(),
                    "doc_len": self._doc_len[:n].cpu(), "dl_host": torch.from_numpy(self._dl_host[:n].copy())}

    def memory_bytes(self):
        return (self._cap + 1) * 8 + self._ecap * 6 + self._cap * 4
