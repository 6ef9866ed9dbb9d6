"""The packed int32 argument block of one sampling step, and the key of the decode graph variant that reads it.

One block per step, one H2D copy: decode metadata, sampling parameters, the carry map, and the sections of the
opt-in features a row of the step uses. StepLayout is the only place that knows the order and the widths; the
engine, its graphs and its eager paths read the block through the named views and fill it with pack().
"""
from typing import NamedTuple

import numpy as np
import torch

from .kv_manager import BLOCK

BAN_IDS_MAX = 16  # width of the per-row ban id table (the ids a request stops on, banned before min_new_tokens)


class GraphKey(NamedTuple):
    """A decode graph variant: the batch bucket and the optional sections of its step block. Build with graph_key."""
    bucket: int
    processors: bool = False
    logprobs: bool = False
    penalties: bool = False


def graph_key(bucket, processors=False, logprobs=False, penalties=False):
    """The penalty fields belong to the processor launch: penalties implies processors (6 variants per bucket)."""
    return GraphKey(int(bucket), bool(processors or penalties), bool(logprobs), bool(penalties))


class StepLayout:
    """Word layout of the block for n rows (a graph's bucket, or the rows of an eager call):

        ids | pos | slots | kv_lens | block table [n, max_blocks] | pad to an even word count
        seeds (int64) | temps (f32) | top_p (f32) | top_k | steps | carry
        processors: rows | penalty (f32) | ngram | ban_count | ban_ids [n, BAN_IDS_MAX]
        penalties:  gen_start | presence (f32) | frequency (f32) | bias_count
        logprobs:   nlp

    The seeds come first in their section, behind the pad, so that their int64 view is 8-byte aligned. A block
    without a block table (max_blocks = 0) serves the eager sampling of prefill's rows: ids and slots stay 0.
    """

    def __init__(self, n, max_blocks, processors=False, penalties=False, logprobs=False):
        self.n, self.max_blocks = n, max_blocks
        self.processors, self.penalties, self.logprobs = bool(processors or penalties), bool(penalties), bool(logprobs)
        sections = [("ids", n), ("pos", n), ("slots", n), ("kv_lens", n),
                    ("block_table", n * max_blocks, None, max_blocks), (None, (4 * n + n * max_blocks) % 2),
                    ("seeds", 2 * n, "int64"), ("temps", n, "float32"), ("top_p", n, "float32"), ("top_k", n),
                    ("steps", n), ("carry", n)]
        if self.processors:
            sections += [("rows", n), ("penalty", n, "float32"), ("ngram", n), ("ban_count", n),
                         ("ban_ids", n * BAN_IDS_MAX, None, BAN_IDS_MAX)]
        if self.penalties:
            sections += [("gen_start", n), ("presence", n, "float32"), ("frequency", n, "float32"), ("bias_count", n)]
        if self.logprobs:
            sections += [("nlp", n)]
        self._views, self.words = [], 0
        for name, words, *kind in sections:
            if name is not None:
                self._views.append((name, self.words, self.words + words, *(kind + [None, None])[:2]))
            self.words += words

    def views(self, buf):
        """{name: view} of an int32 [words] buffer, a torch tensor (device or host) or a numpy array."""
        lib = np if isinstance(buf, np.ndarray) else torch
        out = {}
        for name, a, b, dtype, cols in self._views:
            v = buf[a:b]
            if dtype is not None:
                v = v.view(getattr(lib, dtype))
            out[name] = v.reshape(self.n, cols) if cols is not None else v
        return out

    def pack(self, seqs, carried=None, *, top_k_cap, stop_ids, bt_row=None):
        """The host block of a step over `seqs` (at most n; the other rows are padding that touches nothing: one
        scratch token, history row -1, no carry, no logprobs).

        carried: None, or per sequence the row of the in-flight step whose sampled token it feeds on (-1: none).
        Such a row sits one position further, takes its id on the device (carry) and has generated one more token.
        top_k_cap: the candidate list width, served to a top_k outside 1..top_k_cap. stop_ids(params): the ids
        min_new_tokens bans. bt_row(seq, blocks): the sequence's block table row [max_blocks]."""
        n = len(seqs)
        host = np.zeros(self.words, dtype=np.int32)
        v = self.views(host)
        v["kv_lens"][:] = 1
        v["top_p"][:] = 1.0
        v["top_k"][:] = 1
        v["carry"][:] = -1
        if self.processors:
            v["rows"][:] = -1
            v["penalty"][:] = 1.0
        if self.logprobs:
            v["nlp"][:] = -1
        if not n:
            return host
        if carried is None:
            c = np.zeros(n, dtype=np.int32)
        else:
            v["carry"][:n] = carried
            c = (v["carry"][:n] >= 0).astype(np.int32)
        p = np.fromiter((s.length - 1 for s in seqs), dtype=np.int32, count=n) + c
        v["pos"][:n] = p
        v["kv_lens"][:n] = p + 1
        if self.max_blocks:  # the forward's inputs; a block without a block table feeds no forward
            v["ids"][:n] = [0 if ci else s.token_at(int(q)) for s, q, ci in zip(seqs, p, c)]
            bt = v["block_table"]
            bt[:n] = np.stack([bt_row(s, int(q) // BLOCK + 1) for s, q in zip(seqs, p)])
            v["slots"][:n] = bt[np.arange(n), p // BLOCK] * BLOCK + p % BLOCK
        gen = np.fromiter((len(s.out) for s in seqs), dtype=np.int32, count=n) + c  # generated before this sample
        par = [s.params for s in seqs]
        v["seeds"][:n] = [int(s.seed) & 0x7FFFFFFFFFFFFFFF for s in seqs]
        v["temps"][:n] = [q.temperature if q.do_sample else 0.0 for q in par]
        v["top_p"][:n] = [q.top_p for q in par]
        v["top_k"][:n] = [q.top_k if 0 < q.top_k <= top_k_cap else top_k_cap for q in par]
        v["steps"][:n] = gen
        if self.logprobs:
            v["nlp"][:n] = [q.logprobs if s.logprobs is not None else -1 for s, q in zip(seqs, par)]
        if self.processors:
            for i, (s, q) in enumerate(zip(seqs, par)):
                if s.hist_row < 0:
                    continue
                v["rows"][i], v["penalty"][i], v["ngram"][i] = s.hist_row, q.repetition_penalty, q.no_repeat_ngram_size
                if not q.ignore_eos and gen[i] < q.min_new_tokens:
                    stop = stop_ids(q)
                    v["ban_count"][i] = len(stop)
                    v["ban_ids"][i, :len(stop)] = stop
                if self.penalties:
                    v["gen_start"][i], v["presence"][i], v["frequency"][i], v["bias_count"][i] = \
                        len(s.prompt), q.presence_penalty, q.frequency_penalty, len(q.logit_bias)
        return host
