"""Shared cases of the BM25 lexical search tests (test_lexical_cpu.py: the fp32 replica against a float64
oracle; test_lexical_gpu.py: the kernels against the replica, torch.equal).

A case is a synthetic corpus given directly as CSR entries -- per document sorted distinct term ids (uint32, drawn
over the whole unsigned range, so an id above 2^31 must compare as unsigned), tf and a length -- plus <= 64
queries given as term-id lists, k, and optionally per-query id bitmaps and a live row."""
import math

import numpy as np
import torch

from rag_llm_k8s_amd.index.flat import pack_masks
from rag_llm_k8s_amd.index.lexical import bm25_idf, launch_table

K1, B = 1.2, 0.75


class Case:
    def __init__(self, name, docs, queries, k, allowed=None, qmask=None, live=None):
        """docs: [(terms uint32 ascending, tf, doc_len)]; queries: term-id lists; allowed: bool [n_masks, n]
        rows (per-query id bitmaps) with qmask [nq]; live: bool [n] (the documents that count for df / avgdl)."""
        self.name, self.docs, self.queries, self.k = name, docs, [list(map(int, q)) for q in queries], k
        self.allowed = None if allowed is None else np.asarray(allowed, dtype=bool)
        self.qmask = None if qmask is None else np.asarray(qmask, dtype=np.int32)
        self.live = None if live is None else np.asarray(live, dtype=bool)
        self.n = len(docs)

    def __repr__(self):
        return self.name

    def csr(self):
        rp = np.zeros(self.n + 1, dtype=np.int64)
        rp[1:] = np.cumsum([len(t) for t, _, _ in self.docs])
        cat = lambda i, dt: (np.concatenate([np.asarray(d[i], dtype=dt) for d in self.docs]) if self.n
                             else np.zeros(0, dt))  # noqa: E731
        return rp, cat(0, np.uint32), cat(1, np.uint16), np.asarray([d[2] for d in self.docs], dtype=np.int32)

    def tensors(self):
        """The launch's inputs as CPU tensors in the layout of ops/reference.py (bit patterns in signed types)."""
        rp, te, tf, dl = self.csr()
        qt, member = launch_table(self.queries)
        t = {"row_ptr": torch.from_numpy(rp), "terms": torch.from_numpy(te.view(np.int32)),
             "tf": torch.from_numpy(tf.view(np.int16)), "doc_len": torch.from_numpy(dl),
             "qterms": torch.from_numpy(qt.view(np.int32)), "member": torch.from_numpy(member.view(np.int64)),
             "live": None, "masks": None, "qmask": None}
        if self.live is not None:
            t["live"] = torch.from_numpy(pack_masks(self.live)[0].view(np.int32).copy())
        if self.allowed is not None:
            t["masks"] = torch.from_numpy(pack_masks(self.allowed).view(np.int32).copy())
            t["qmask"] = torch.from_numpy(self.qmask)
        return t

    def host_numbers(self, df):
        """(idf fp32 tensor [T], avgdl) the way the index computes them from the lex_df counts."""
        live = np.ones(self.n, bool) if self.live is None else self.live
        dl = np.asarray([d[2] for d in self.docs], dtype=np.int64)[live]
        total = int(dl.sum())
        avgdl = float(np.float32(total / len(dl))) if total else 1.0
        return torch.from_numpy(bm25_idf(np.asarray(df), int(live.sum()))), avgdl

    # ---- the independent float64 oracle: Python dicts, no shared code with the replica
    def oracle(self):
        """Per query [(score float64, id)] of every candidate the query may return, best first (score
        descending, id ascending), and the df dict."""
        live = [True] * self.n if self.live is None else [bool(x) for x in self.live]
        post = [{int(t): int(f) for t, f in zip(d[0], d[1])} for d in self.docs]
        n_live = sum(live)
        tot = sum(d[2] for d, lv in zip(self.docs, live) if lv)
        avgdl = tot / n_live if tot else 1.0
        df = {}
        for p, lv in zip(post, live):
            if lv:
                for t in p:
                    df[t] = df.get(t, 0) + 1
        out = []
        for qi, q in enumerate(self.queries):
            terms = sorted(set(q))
            row = None if self.qmask is None or self.qmask[qi] < 0 else self.allowed[self.qmask[qi]]
            res = []
            for d, p in enumerate(post):
                if row is not None and not row[d]:
                    continue
                s, hit = 0.0, False
                for t in terms:
                    if t in p:
                        hit = True
                        idf = math.log1p((n_live - df.get(t, 0) + 0.5) / (df.get(t, 0) + 0.5))
                        norm = K1 * ((1 - B) + B * (self.docs[d][2] / avgdl))
                        s += idf * ((p[t] * (K1 + 1)) / (p[t] + norm))
                if hit:
                    res.append((s, d))
            out.append(sorted(res, key=lambda x: (-x[0], x[1])))
        return out, df


def _vocab(rng, size):
    v = np.unique(rng.integers(0, 0xFFFFFFFE, size=2 * size + 8, dtype=np.uint64))
    return rng.permutation(v)[:size].astype(np.uint32)


def _doc(rng, vocab, m, dl_extra=True):
    terms = np.sort(rng.choice(vocab, size=min(m, len(vocab)), replace=False))
    tf = rng.integers(1, 7, size=len(terms)).astype(np.int64)
    return terms.astype(np.uint32), tf, int(tf.sum()) + (int(rng.integers(0, 4)) if dl_extra else 0)


def _corpus(seed, n, vocab_size, sizes):
    rng = np.random.default_rng(seed)
    vocab = _vocab(rng, vocab_size)
    return rng, vocab, [_doc(rng, vocab, int(sizes(rng, i))) for i in range(n)]


def _queries(rng, vocab, nq, nt):
    return [list(rng.choice(vocab, size=min(nt, len(vocab)), replace=False)) for _ in range(nq)]


def n_sweep():
    """N = 1 / 63 / 64 / 65 / 257 / 1025: below, at and above one tile, several tiles, more tiles than a wave's
    share; short documents over a small vocabulary, so most documents match and the lists are full."""
    out = []
    for n in (1, 63, 64, 65, 257, 1025):
        rng, vocab, docs = _corpus(100 + n, n, 40, lambda r, i: r.integers(0, 12))
        out.append(Case("n%d" % n, docs, _queries(rng, vocab, 5, 4), 5))
    return out


def mixed_sizes():
    """Documents of 0 / 1 / 64 / 65 / 1500 entries in one index (the entry stream's chunk boundaries)."""
    sizes = [0, 1, 64, 65, 1500]
    rng, vocab, docs = _corpus(7, 70, 3000, lambda r, i: sizes[i % 5])
    return Case("mixed_sizes", docs, _queries(rng, vocab, 13, 5), 5)


def t_sweep():
    """T = 1 / 64 / 65 / 4096 table terms (4096 = 64 queries of 64 distinct terms each)."""
    out = []
    rng, vocab, docs = _corpus(11, 130, 6000, lambda r, i: r.integers(0, 400))
    out.append(Case("T1", docs, [[vocab[3]]], 5))
    out.append(Case("T64", docs, [list(vocab[:64])], 5))
    out.append(Case("T65", docs, [list(vocab[:64]), [vocab[64]]], 5))
    out.append(Case("T4096", docs, [list(vocab[64 * q:64 * q + 64]) for q in range(64)], 5))
    return out


def nq_k_sweep():
    """nq = 1 / 33 / 64 with k = 1 / 5 / 64 (a query per lane up to the full wave; one, a few, a full list)."""
    out = []
    rng, vocab, docs = _corpus(13, 300, 60, lambda r, i: r.integers(1, 15))
    for nq, k in ((1, 1), (33, 5), (64, 64), (1, 64), (64, 1)):
        out.append(Case("nq%d_k%d" % (nq, k), docs, _queries(rng, vocab, nq, 3), k))
    return out


def edge_cases():
    out = []
    rng, vocab, docs = _corpus(17, 200, 300, lambda r, i: r.integers(1, 30))
    rare = [d for d in range(200) if vocab[0] in docs[d][0]]
    # k above the number of matches (padding), a query with no terms, a term in no document
    out.append(Case("k_above_matches", docs, [[vocab[0]], [], [0x12345678 if 0x12345678 not in vocab else 1],
                                             [vocab[1], vocab[2]]], 64))
    assert 0 < len(rare) < 64
    # a term in every document (df = n: the smallest idf) next to a rare one
    every = [(np.sort(np.append(t[t != 77], 77)).astype(np.uint32), None, dl) for t, _, dl in docs]
    every = [(t, rng.integers(1, 7, size=len(t)), dl) for t, _, dl in every]
    out.append(Case("term_in_every_doc", every, [[77], [77, int(every[5][0][0])]], 7))
    # all documents identical: every score ties, ids ascending (130 documents: three tiles)
    one = _doc(rng, vocab, 9)
    out.append(Case("identical_docs", [one] * 130, [list(one[0][:3]), [int(one[0][4])]], 64))
    # ties across tile boundaries: copies of one document at ids 10, 63, 64, 70, 200 among different ones
    tied = list(docs)
    for i in (10, 63, 64, 70, 199):
        tied[i] = docs[10]
    out.append(Case("ties_across_tiles", tied, [list(docs[10][0][:2]), [int(docs[10][0][0])]], 8))
    return out


def mask_cases():
    """Per-query bitmaps: ids 31 / 32 / 33 (a word boundary) and the last id, a mask that removes the winner, an
    unfiltered query next to filtered ones, and a live row that changes df (and with it the order)."""
    out = []
    rng, vocab, docs = _corpus(19, 100, 30, lambda r, i: r.integers(1, 10))
    qs = _queries(rng, vocab, 4, 3)
    al = np.zeros((3, 100), bool)
    al[0, [31, 32, 33, 99]] = True
    al[1, 32] = True
    al[2, :] = True
    out.append(Case("mask_word_boundary", docs, qs, 5, allowed=al, qmask=[0, 1, -1, 2]))
    base = Case("tmp", docs, qs, 5)
    winner = base.oracle()[0][0][0][1]
    al = np.ones((1, 100), bool)
    al[0, winner] = False
    out.append(Case("mask_removes_winner", docs, qs, 5, allowed=al, qmask=[0, -1, -1, 0]))
    live = np.ones(100, bool)
    live[rng.choice(100, size=40, replace=False)] = False
    out.append(Case("live_row_changes_df", docs, qs, 5, allowed=live[None, :], qmask=[0, 0, 0, 0], live=live))
    return out


def kernel_cases():
    return n_sweep() + [mixed_sizes()] + t_sweep() + nq_k_sweep() + edge_cases() + mask_cases()


def replica_cases():
    """The cases the replica is checked on against the float64 oracle: those whose neighbouring float64 scores
    are either exactly equal or farther apart than the two fp32 error bounds together (the test asserts it). The
    64-query cases rank 300 documents 64 deep for 64 queries and hold a few closer pairs, and T = 4096 adds
    nothing a float64 comparison could see; the kernel test runs them against the replica."""
    return [c for c in kernel_cases() if c.name not in ("T4096", "nq64_k64", "nq64_k1")]


def rel_bound(T):
    """(T + 8) * 2^-24: six roundings per term (idf, the two products, the sum and the quotient of the
    contribution, the norm's share) and one per add; every term is positive, so nothing cancels."""
    return (T + 8) * 2.0 ** -24
