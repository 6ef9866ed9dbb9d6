"""Second-stage retrieval: a cross-encoder scores every (query, chunk) pair and the best k are kept.

The bi-encoder search returns `rerank_candidates` chunks per query in L2 order; this engine builds the
sentence pair of each (the layout is the tokenizer's own post-processor), packs all pairs of a micro-batch
into varlen batches like the embedding engine, runs the encoder + classification head
(models/encoder.py: score_packed) and orders each query's candidates by score on the device
(ops: rerank_select -- stable, so ties stay in L2 order).

Chunks recur across queries, so their token arrays are kept in a bounded LRU (keyed by the chunk text,
bounded by total tokens); only the short queries are tokenised per request.
"""
from __future__ import annotations

import threading
from collections import OrderedDict

import numpy as np
import torch

from ..ops.backend import get_backend
from .encoder_engine import pack_batches

MAX_CANDIDATES = 64  # rerank_select: one wave lane per candidate


class PairLayout:
    """The sentence-pair template of a tokenizer.json post-processor: a list of ("tok", id, type),
    ("A", type) and ("B", type) items, e.g. [CLS] A [SEP] B:1 [SEP]:1 or <s> A </s> </s> B </s>."""

    def __init__(self, items):
        self.items = items
        self.specials = sum(1 for it in items if it[0] == "tok")
        if [it[0] for it in items if it[0] != "tok"] != ["A", "B"]:
            raise ValueError("pair template must hold the sequences A and B once each, in this order")

    @classmethod
    def from_spec(cls, spec, token_to_id):
        pp = spec.get("post_processor")
        found = cls._find(pp)
        if found is None:
            raise ValueError("tokenizer.json has no TemplateProcessing / BertProcessing / RobertaProcessing "
                             "post-processor: cannot build sentence pairs")
        kind = found["type"]
        if kind == "TemplateProcessing":
            if not found.get("pair"):
                raise ValueError("tokenizer.json: TemplateProcessing without a pair template")
            special = found.get("special_tokens", {})
            items = []
            for it in found["pair"]:
                if "SpecialToken" in it:
                    st = it["SpecialToken"]
                    ids = special.get(st["id"], {}).get("ids")
                    if ids is None:
                        tid = token_to_id(st["id"])
                        if tid is None:
                            raise ValueError("pair template names an unknown special token %r" % st["id"])
                        ids = [tid]
                    items.extend(("tok", int(i), int(st.get("type_id", 0))) for i in ids)
                else:
                    sq = it["Sequence"]
                    items.append((sq["id"], int(sq.get("type_id", 0))))
            return cls(items)
        sep, cl = int(found["sep"][1]), int(found["cls"][1])
        if kind == "BertProcessing":
            return cls([("tok", cl, 0), ("A", 0), ("tok", sep, 0), ("B", 1), ("tok", sep, 1)])
        return cls([("tok", cl, 0), ("A", 0), ("tok", sep, 0), ("tok", sep, 0), ("B", 0), ("tok", sep, 0)])

    @classmethod
    def _find(cls, pp):
        if not isinstance(pp, dict):
            return None
        if pp.get("type") in ("TemplateProcessing", "BertProcessing", "RobertaProcessing"):
            return pp
        for sub in pp.get("processors", []) or []:
            f = cls._find(sub)
            if f is not None:
                return f
        return None

    def build(self, a, b):
        """(ids, type_ids) int32 arrays of the pair of token arrays a, b."""
        ids, types = [], []
        for it in self.items:
            if it[0] == "tok":
                ids.append(np.array([it[1]], dtype=np.int32))
                types.append(np.array([it[2]], dtype=np.int32))
            else:
                seq = a if it[0] == "A" else b
                ids.append(np.asarray(seq, dtype=np.int32))
                types.append(np.full(len(seq), it[1], dtype=np.int32))
        return np.concatenate(ids), np.concatenate(types)


class TokenCache:
    """Thread-safe LRU of token arrays keyed by text, bounded by the total number of cached tokens."""

    def __init__(self, max_tokens):
        self.max_tokens = int(max_tokens)
        self.tokens = 0
        self._d = OrderedDict()
        self._lock = threading.Lock()

    def __len__(self):
        return len(self._d)

    def get(self, text):
        with self._lock:
            v = self._d.get(text)
            if v is not None:
                self._d.move_to_end(text)
            return v

    def put(self, text, ids):
        n = len(ids)
        if n > self.max_tokens:
            return
        with self._lock:
            old = self._d.pop(text, None)
            if old is not None:
                self.tokens -= len(old)
            self._d[text] = ids
            self.tokens += n
            while self.tokens > self.max_tokens:
                _, ev = self._d.popitem(last=False)
                self.tokens -= len(ev)


class Reranker:
    def __init__(self, model, tokenizer, max_len: int = 512, max_batch_tokens: int = 65536,
                 cache_tokens: int = 8_000_000):
        if getattr(model.w, "head", None) is None:
            raise ValueError("the reranker model has no sequence-classification head")
        self.model = model
        self.tok = tokenizer
        self.device = model.device
        self.be = get_backend(self.device)
        self.layout = PairLayout.from_spec(tokenizer.spec, tokenizer.token_to_id)
        cfg = model.cfg
        pos_off = cfg.pad_token_id + 1 if cfg.model_type == "xlm-roberta" else 0
        self.max_len = min(int(max_len), cfg.max_position_embeddings - pos_off)  # capped by the model's positions
        self.budget = self.max_len - self.layout.specials
        if self.budget < 2:
            raise ValueError("RERANK_MAX_LEN %d leaves no room for a query and a document" % max_len)
        self.max_batch_tokens = int(max_batch_tokens)
        self.typed = cfg.type_vocab_size > 1
        self.cache = TokenCache(cache_tokens)

    # ------------------------------------------------------------------ tokens
    def _doc_tokens(self, docs):
        """Token arrays (no special tokens, at most `budget` tokens) of the documents, through the cache."""
        out, missing = {}, []
        for d in docs:
            if d in out:
                continue
            v = self.cache.get(d)
            out[d] = v
            if v is None:
                missing.append(d)
        if missing:
            enc = self.tok.encode_batch(missing, add_special_tokens=False, max_length=self.budget)
            for d, ids in zip(missing, enc):
                arr = np.asarray(ids[:self.budget], dtype=np.int32)
                out[d] = arr
                self.cache.put(d, arr)
        return out

    def build_pair(self, q_ids, d_ids):
        """Truncate and join one pair: the query keeps at most budget // 2 tokens, the document the rest
        (HF truncation="only_second" whenever the query is shorter than half the budget)."""
        q = np.asarray(q_ids, dtype=np.int32)[:self.budget // 2]
        d = np.asarray(d_ids, dtype=np.int32)[:self.budget - len(q)]
        return self.layout.build(q, d)

    def pairs(self, queries, docs_per_query):
        """[(ids, type_ids)] of every (query, document) pair, query-major."""
        q_tok = self.tok.encode_batch(list(queries), add_special_tokens=False, max_length=self.budget // 2)
        d_tok = self._doc_tokens([d for docs in docs_per_query for d in docs])
        return [self.build_pair(q_tok[i], d_tok[d]) for i, docs in enumerate(docs_per_query) for d in docs]

    # ------------------------------------------------------------------ scoring
    @torch.no_grad()
    def _score_flat(self, queries, docs_per_query):
        """fp32 device tensor with one score per pair, query-major."""
        pairs = self.pairs(queries, docs_per_query)
        n = len(pairs)
        out = torch.empty((n,), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        lens = np.array([len(p[0]) for p in pairs], dtype=np.int32)
        for rows, row_lens in pack_batches(lens, self.max_batch_tokens):
            ids = torch.from_numpy(np.concatenate([pairs[r][0] for r in rows])).to(self.device)
            types = None
            if self.typed:
                types = torch.from_numpy(np.concatenate([pairs[r][1] for r in rows])).to(self.device)
            s = self.model.score_packed(ids, [int(x) for x in row_lens], types)
            out[torch.from_numpy(rows).to(self.device)] = s
        return out

    def score(self, queries, docs_per_query):
        """Per query, an fp32 numpy array with the relevance score of each of its documents."""
        flat = self._score_flat(queries, docs_per_query).cpu().numpy()
        cuts = np.cumsum([len(d) for d in docs_per_query])[:-1]
        return [np.ascontiguousarray(a) for a in np.split(flat, cuts)] if len(docs_per_query) else []

    # ------------------------------------------------------------------ reranking
    def rerank(self, queries, results, k):
        """results: per query a ragged list of (metadata, distance) in L2 order (DocumentStore.search).
        Returns the same structure, ordered by cross-encoder score (ties keep the L2 order) and cut to k.
        Every metadata dict is a copy with `rerank_score` added; the distance is unchanged."""
        Q = len(results)
        counts = [len(r) for r in results]
        N = max(counts) if counts else 0
        if N == 0:
            return [[] for _ in results]
        if N > MAX_CANDIDATES:
            raise ValueError("rerank: at most %d candidates per query (got %d)" % (MAX_CANDIDATES, N))
        k = max(1, min(int(k), N))
        flat = self._score_flat(queries, [[m.get("text", "") for m, _ in r] for r in results])
        slot = np.concatenate([q * N + np.arange(c, dtype=np.int64) for q, c in enumerate(counts)])
        scores = torch.zeros((Q * N,), dtype=torch.float32, device=self.device)
        scores[torch.from_numpy(slot).to(self.device)] = flat
        dist = np.zeros((Q, N), dtype=np.float32)
        for q, r in enumerate(results):
            dist[q, :len(r)] = [d for _, d in r]
        cand = torch.arange(N, dtype=torch.int64).repeat(Q, 1).to(self.device)
        oi, _, osc = self.be.rerank_select(scores.view(Q, N), cand, torch.from_numpy(dist).to(self.device),
                                           torch.tensor(counts, dtype=torch.int32).to(self.device), k)
        oi, osc = oi.cpu().view(Q, k).tolist(), osc.cpu().view(Q, k).tolist()
        out = []
        for q, r in enumerate(results):
            rows = []
            for c, s in zip(oi[q], osc[q]):
                if c < 0:
                    break
                m = dict(r[c][0])
                m["rerank_score"] = float(s)
                rows.append((m, r[c][1]))
            out.append(rows)
        return out
