"""Shared inputs and oracles of the logit-processor tests (test_logits_proc_cpu.py / test_logits_proc_gpu.py).

A case is a dict of CPU tensors with the arguments of ops.backend.TorchBackend.logits_process: logits [B, V] fp32,
ids ([B] int32 or None), rows / pos [B] int32, hist [R, ld] int32, penalty [B] fp32, ngram [B] int32, ban_ids
[B, W] int32, ban_count [B] int32, vocab_offset. Three oracles:
  * reference(case): the torch backend (what the CPU engine runs and what the kernels must equal bit for bit);
  * hf_row(...): transformers' own three processors, chained in generate()'s order;
  * python_row(...): the definitions spelled out token by token in Python with numpy float32 arithmetic.
"""
import numpy as np
import torch

POISON = 1  # id that fills history rows / cells no active row may read; no test history holds it
BAN_W = 16


def make_logits(B, V, seed):
    """fp32 rows with positive, negative, exactly-zero and -inf entries."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, V, generator=g) * 4.0
    kind = torch.randint(0, 10, (B, V), generator=g)
    x[kind == 0] = 0.0
    x[kind == 1] = float("-inf")
    return x


def make_case(logits, seqs, penalty, ngram, bans=None, rows=None, decode=False, hist_rows=None, ld=None,
              vocab_offset=0):
    """seqs[b]: the token history of row b (None: a row without processors, history row -1). With decode the
    last token of each history is NOT in `hist` yet: it is passed as ids[b] and the op stores it."""
    B = logits.shape[0]
    rows = list(range(B)) if rows is None else list(rows)
    R = hist_rows or (max(rows) + 2)
    ld = ld or max(8, max(len(s) for s in seqs if s is not None) + 3)
    hist = torch.full((R, ld), POISON, dtype=torch.int32)
    pos = torch.zeros(B, dtype=torch.int32)
    ids = torch.zeros(B, dtype=torch.int32)
    r = torch.full((B,), -1, dtype=torch.int32)
    for b, s in enumerate(seqs):
        if s is None:
            continue
        r[b] = rows[b]
        n = len(s) - 1 if decode else len(s)
        hist[rows[b], :n] = torch.tensor(s[:n], dtype=torch.int32)
        pos[b] = len(s) - 1
        ids[b] = s[-1]
    ban_ids = torch.zeros((B, BAN_W), dtype=torch.int32)
    ban_count = torch.zeros(B, dtype=torch.int32)
    for b, bl in enumerate(bans or []):
        ban_count[b] = len(bl)
        ban_ids[b, :len(bl)] = torch.tensor(bl, dtype=torch.int32)
    pen = torch.tensor([float(p) for p in (penalty if isinstance(penalty, (list, tuple)) else [penalty] * B)],
                       dtype=torch.float32)
    ng = torch.tensor(ngram if isinstance(ngram, (list, tuple)) else [ngram] * B, dtype=torch.int32)
    return dict(logits=logits.clone(), ids=ids if decode else None, rows=r, pos=pos, hist=hist, penalty=pen,
                ngram=ng, ban_ids=ban_ids, ban_count=ban_count, vocab_offset=vocab_offset)


def reference(case):
    """(processed logits, history after the call) of the torch backend; the case is left unchanged."""
    from rag_llm_k8s_amd.ops.backend import TorchBackend

    lg, hist = case["logits"].clone(), case["hist"].clone()
    TorchBackend("cpu").logits_process(lg, case["vocab_offset"], case["ids"], case["rows"], case["pos"], hist,
                                       case["penalty"], case["ngram"], case["ban_ids"], case["ban_count"])
    return lg, hist


def hf_row(x, seq, penalty, n, min_new_tokens, generated, stop_ids):
    """transformers' processors on one fp32 row in generate()'s order (repetition penalty, n-gram ban,
    min_new_tokens); `generated` of the len(seq) tokens are new."""
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)

    ids = torch.tensor([seq], dtype=torch.long)
    s = x.clone()[None]
    if penalty != 1.0:
        s = RepetitionPenaltyLogitsProcessor(penalty=float(penalty))(ids, s)
    if n > 0:
        s = NoRepeatNGramLogitsProcessor(n)(ids, s)
    if min_new_tokens > 0 and stop_ids:
        s = MinNewTokensLengthLogitsProcessor(len(seq) - generated, min_new_tokens, list(stop_ids), device="cpu")(ids, s)
    return s[0]


def python_row(x, seq, penalty, n, bans):
    """The definitions, token by token: numpy float32 scalars, Python sets."""
    out = x.clone().numpy()
    p = np.float32(penalty)
    if penalty != 1.0:
        for t in set(seq):
            v = np.float32(x[t])
            out[t] = v * p if v < 0 else v / p
    L = len(seq)
    if n > 0 and L + 1 >= n:
        tail = tuple(seq[L - n + 1:]) if n > 1 else ()
        for j in range(0, L - n + 1):
            if tuple(seq[j:j + n - 1]) == tail:
                out[seq[j + n - 1]] = -np.inf
    for t in bans:
        out[t] = -np.inf
    return torch.from_numpy(out)


def ngram_histories(n, L, vocab=50, seed=0):
    """Histories of length L for the n-gram ban: one id repeated (the suffix matches at every j, so at j = 0, at
    the last legal j = L - n and at overlapping positions), a period-2 and a period-3 pattern (overlapping
    matches), and a random history whose first n-1 tokens are a planted copy of its last n-1 (a match at j = 0
    alone when L allows)."""
    g = torch.Generator().manual_seed(seed * 131 + n * 17 + L)
    out = [[7] * L, [(11, 12)[i % 2] for i in range(L)], [(21, 22, 23)[i % 3] for i in range(L)]]
    r = torch.randint(2, vocab, (L,), generator=g).tolist()
    if n > 1 and L >= 2 * (n - 1) + 1:
        r[:n - 1] = r[L - n + 1:]
    out.append(r)
    return out


def no_ngram_repeats(tokens, n, start=0):
    """True if no n-gram that ends at index >= start occurs earlier in `tokens` too (start = prompt length: what
    the ban promises for a prompt that repeats n-grams itself; 0: no n-gram occurs twice at all)."""
    seen = set()
    for i in range(len(tokens) - n + 1):
        g = tuple(tokens[i:i + n])
        if g in seen and i + n - 1 >= start:
            return False
        seen.add(g)
    return True
