"""Shared inputs and oracles of the presence / frequency penalty and logit_bias tests (test_penalties_cpu.py /
test_penalties_gpu.py), on top of logits_proc_cases.

A case is a logits_proc_cases case plus the keyword arguments of the penalty form of logits_process: gen_start,
presence, frequency, bias_count [B], and the bias tables bias_ids / bias_vals [history rows, width] indexed by the
HISTORY row. Every table cell no active row may read (past a row's bias_count, and the rows of nobody) holds a
poison entry: id POISON with a bias that would show. Oracles:
  * reference(case): the torch backend (what the CPU engine runs and what the kernel must equal bit for bit);
  * counter_row(...): frequency / presence token by token, collections.Counter over the generated span and numpy
    float32 arithmetic in the stated order;
  * chain_row(...): transformers' SequenceBias -> RepetitionPenalty -> counter_row -> NoRepeatNGram ->
    MinNewTokens.
"""
from collections import Counter

import numpy as np
import torch

import logits_proc_cases as C

BIAS_W = 300  # LOGIT_BIAS_MAX
BIAS_POISON = 4096.0
GEN_MAX = 8192  # PENALTY_GEN_MAX
KEYS = ("gen_start", "presence", "frequency", "bias_ids", "bias_vals", "bias_count")


def _per_row(v, B):
    return list(v) if isinstance(v, (list, tuple)) else [v] * B


def make_case(logits, seqs, gen_start, presence, frequency, bias=None, penalty=1.0, ngram=0, bans=None, rows=None,
              decode=False, hist_rows=None, ld=None, vocab_offset=0, bias_w=BIAS_W):
    """seqs / penalty / ngram / bans / rows / decode / hist_rows / ld: as logits_proc_cases.make_case. gen_start,
    presence, frequency: one value or one per row. bias[b]: {id: bias} of row b (None / {}: no bias)."""
    B = logits.shape[0]
    case = C.make_case(logits, seqs, penalty, ngram, bans=bans, rows=rows, decode=decode, hist_rows=hist_rows, ld=ld,
                       vocab_offset=vocab_offset)
    R = case["hist"].shape[0]
    bias_ids = torch.full((R, bias_w), C.POISON, dtype=torch.int32)
    bias_vals = torch.full((R, bias_w), BIAS_POISON, dtype=torch.float32)
    bias_count = torch.zeros(B, dtype=torch.int32)
    g0 = torch.zeros(B, dtype=torch.int32)
    for b, s in enumerate(seqs):
        if s is None:
            continue
        g0[b] = _per_row(gen_start, B)[b]
        d = (bias or [None] * B)[b] or {}
        r = int(case["rows"][b])
        items = sorted(d.items())
        bias_count[b] = len(items)
        if items:
            bias_ids[r, :len(items)] = torch.tensor([t for t, _ in items], dtype=torch.int32)
            bias_vals[r, :len(items)] = torch.tensor([v for _, v in items], dtype=torch.float32)
    case.update(gen_start=g0, presence=torch.tensor(_per_row(presence, B), dtype=torch.float32),
                frequency=torch.tensor(_per_row(frequency, B), dtype=torch.float32), bias_ids=bias_ids,
                bias_vals=bias_vals, bias_count=bias_count)
    return case


def gen_bound(case):
    """The largest generated span of an active row (what a caller passes as gen_bound)."""
    live = case["rows"] >= 0
    if not bool(live.any()):
        return 0
    return int((case["pos"][live] + 1 - case["gen_start"][live]).max())


def reference(case, **kw):
    """(processed logits, history after the call) of the torch backend; the case is left unchanged."""
    from rag_llm_k8s_amd.ops.backend import TorchBackend

    lg, hist = case["logits"].clone(), case["hist"].clone()
    TorchBackend("cpu").logits_process(lg, case["vocab_offset"], case["ids"], case["rows"], case["pos"], hist,
                                       case["penalty"], case["ngram"], case["ban_ids"], case["ban_count"],
                                       **dict({k: case[k] for k in KEYS}, **kw))
    return lg, hist


def counter_row(x, seq, gen_start, frequency, presence):
    """(x - frequency * float(count)) - presence for every distinct generated id: numpy float32, Counter."""
    out = x.clone().numpy()
    f, p = np.float32(frequency), np.float32(presence)
    if f == 0 and p == 0:
        return torch.from_numpy(out)
    with np.errstate(invalid="ignore"):
        for t, c in Counter(seq[gen_start:]).items():
            out[t] = np.float32(np.float32(out[t] - np.float32(f * np.float32(c))) - p)
    return torch.from_numpy(out)


def chain_row(x, seq, gen_start, bias, penalty, frequency, presence, n, min_new_tokens, stop_ids):
    """transformers' processors around the Counter oracle, on one fp32 row, in the engine's order."""
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor,
                                                        SequenceBiasLogitsProcessor)

    ids = torch.tensor([seq], dtype=torch.long)
    s = x.clone()[None]
    if bias:
        s = SequenceBiasLogitsProcessor([[[int(t)], float(v)] for t, v in sorted(bias.items())])(ids, s)
    if penalty != 1.0:
        s = RepetitionPenaltyLogitsProcessor(penalty=float(penalty))(ids, s)
    s = counter_row(s[0], seq, gen_start, frequency, presence)[None]
    if n > 0:
        s = NoRepeatNGramLogitsProcessor(n)(ids, s)
    if min_new_tokens > 0 and stop_ids:
        s = MinNewTokensLengthLogitsProcessor(gen_start, min_new_tokens, list(stop_ids), device="cpu")(ids, s)
    return s[0]


def table_hash(t, slots):
    """The slot the kernel's counting table probes first for local id t (csrc/kernels/logits_proc.hip lp_hash):
    the top log2(slots) bits of t * 2654435761 mod 2^32."""
    return ((t * 2654435761) & 0xFFFFFFFF) >> (32 - (slots.bit_length() - 1))


def table_slots(span):
    """Slots of the table a row with `span` generated tokens gets: the power of two >= 2 * span, 64..16384."""
    s = 64
    while s < 2 * span and s < 2 * GEN_MAX:
        s *= 2
    return s


def colliding_ids(V, slots, count, start=2):
    """`count` ids below V whose first probes fall on the last two slots of a `slots`-slot table and then, wrapped,
    on its first ones: one probe run as long as the span that crosses the table's end."""
    by = {}
    for t in range(start, V):
        by.setdefault(table_hash(t, slots), []).append(t)
    out, h = [], slots - 2
    while len(out) < count:
        out += by.get(h, [])
        h = (h + 1) % slots
        assert h != slots - 2, "not enough ids"
    return out[:count]
