"""Shared inputs, oracles and the checker of the logprob tests (test_logprobs_cpu.py / test_logprobs_gpu.py).

A backend here is anything with lse_partials(logits, chunks, out=) and logprobs_finish(part, cand_v, cand_i,
list_len, tok, nlp, out_lse, out_tok_lp, out_top_lp, out_top_id): ops.backend.TorchBackend on CPU tensors (what
the CPU engine runs) or ops.native on GPU tensors (the kernels of csrc/kernels/logprobs.hip). check_case() runs
one case through both launches inside canary frames.

Oracles:
  * lse: float64 torch.logsumexp of the same fp32 row. Bound per row
        max(8 * |fp32 torch.logsumexp on the CPU - float64|, 2**-22 * max(1, |lse|))
    -- the project's usual 8x the fp32-torch error, with a floor of two fp32 ulps of the result for rows where
    torch's fp32 result happens to be exact.
  * ids: a stable descending sort of the fp32 row (value desc, id asc), torch.equal.
  * logprobs: x[id] - out_lse in fp32 torch from the backend's own out_lse, torch.equal.
  * candidate lists: per vocab chunk a stable descending sort cut to K (what topk_candidates yields, ties to the
    lower id), built here so that the CPU and GPU tests feed the finish step the same bytes.

Largest observed |lse - float64| / bound over all cases: 0.28 (GPU kernels), 0.15 (torch backend); the tests
print the ratio per case.
"""
import torch

from rag_llm_k8s_amd.ops.reference import LOGPROBS_MAX, lse_chunk_width

NEG = float("-inf")
GAP = 3.0e30  # fills the gaps of strided logits views: one gap entry read as a logit wrecks the row's lse
CANARY_F = 12345.5
CANARY_I = -777


def lse_oracle(x):
    """(float64 lse [B], bound [B]) of fp32 rows x."""
    l64 = torch.logsumexp(x.double(), 1)
    l32 = torch.logsumexp(x.float(), 1).double()
    bound = torch.maximum(8 * (l32 - l64).abs(), 2.0 ** -22 * l64.abs().clamp(min=1.0))
    return l64, bound


def chunk_candidates(x, chunks, K, vocab_offset=0):
    """[B, chunks * K] (values, global ids): per chunk (the top-k's chunk width) the first K of a stable
    descending sort, padded with (-inf, -1)."""
    B, V = x.shape
    Vc = lse_chunk_width(V, chunks)
    cv = torch.full((B, chunks, K), NEG)
    ci = torch.full((B, chunks, K), -1, dtype=torch.int32)
    for c in range(chunks):
        lo, hi = min(c * Vc, V), min((c + 1) * Vc, V)
        if hi == lo:
            continue
        v, i = torch.sort(x[:, lo:hi], dim=1, descending=True, stable=True)
        k = min(K, hi - lo)
        cv[:, c, :k] = v[:, :k]
        ci[:, c, :k] = (i[:, :k] + lo + vocab_offset).int()
    return cv.reshape(B, -1), ci.reshape(B, -1)


def make_rows(V, chunks, special, seed):
    """Five fp32 rows: randn * 5; the same + 100 and - 100 (overflow / vanish without the max subtraction);
    whole chunks of -inf; and one special row:
      one_finite: a single finite entry; all_equal: every entry the same value; ties: the row maximum four
      times, straddling the boundary of chunks 0 and 1 (or mid-row with one chunk)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(V, generator=g) * 5
    Vc = lse_chunk_width(V, chunks)
    holes = base.clone()
    holes[torch.randint(0, 10, (V,), generator=g) == 0] = NEG
    for c in ({0, chunks // 2, chunks - 1} if chunks > 3 else {0} if chunks > 1 else ()):
        holes[min(c * Vc, V):min((c + 1) * Vc, V)] = NEG  # (a trailing chunk may be empty: past V)
    if special == "one_finite":
        sp = torch.full((V,), NEG)
        sp[(7 * V) // 11] = -3.25
    elif special == "all_equal":
        sp = torch.full((V,), 1.75)
    else:
        sp = torch.randn(V, generator=g) * 5
        mid = Vc if chunks > 1 and Vc + 2 <= V else V // 2
        sp[mid - 2:mid + 2] = float(sp.max()) + 1.0
    return torch.stack([base, base + 100.0, base - 100.0, holes, sp])


NLP_PATTERNS = ([20, 5, 1, 0, 20], [1, -1, 20, 5, 20], [-1, 20, 0, -1, 5])


def kernel_cases():
    """(name, dict): V = 1001 / 4099 over chunks 1 / 3 / 31 / 64, contiguous rows and strided views, the three
    special rows and the three nlp patterns rotating; one Llama-3-sized case (V = 128256, B = 2)."""
    out = []
    k = 0
    for V in (1001, 4099):
        for chunks in (1, 3, 31, 64):
            for strided in (False, True):
                special = ("one_finite", "all_equal", "ties")[k % 3]
                out.append(("V%d-c%d-%s-%s" % (V, chunks, "strided" if strided else "contig", special),
                            dict(V=V, chunks=chunks, strided=strided, special=special, nlp=NLP_PATTERNS[k % 3],
                                 seed=100 + k, list_len=64 if k % 4 else LOGPROBS_MAX)))
                k += 1
    out.append(("V128256-c31-contig", dict(V=128256, chunks=31, strided=False, special="ties", nlp=[20, 5], seed=9,
                                           list_len=64, rows=2)))
    return out


def build(case):
    """The case's CPU tensors: x [B, V], candidate lists, sampled tokens, nlp."""
    x = make_rows(case["V"], case["chunks"], case["special"], case["seed"])[:case.get("rows", 5)]
    B = x.shape[0]
    K = case["list_len"]
    tk = max(1, min(case["chunks"], 31, 2048 // K))  # candidate lists: at most 2048 entries per row
    cv, ci = chunk_candidates(x, tk, K)
    # sampled tokens: the best candidate, the last entry of the last list (when it is a real one), one from
    # the middle of a list -- always a member of the lists, as on the in-graph path
    tok = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        pick = (0, cv.shape[1] - 1, min(7, K - 1), K - 1, 0)[b % 5]
        if ci[b, pick] < 0:
            pick = 0
        tok[b] = ci[b, pick]
    return x, cv, ci, tok, torch.tensor(case["nlp"][:B], dtype=torch.int32)


def frame(x, strided):
    """The rows as a contiguous tensor, or as a view into a wider buffer whose gaps hold GAP: pitch V + 13 and a
    column offset of 3, so row starts are misaligned and differ in alignment from row to row."""
    if not strided:
        return x.clone()
    B, V = x.shape
    buf = torch.full((B + 2, V + 13), GAP)
    buf[1:1 + B, 3:3 + V] = x
    return buf


def view(buf, x, strided):
    B, V = x.shape
    return buf[1:1 + B, 3:3 + V] if strided else buf


def run_lse_partials(be, dev, x, chunks, strided):
    """part [B, chunks, 2] (CPU) from the backend, written inside a canary frame that must stay intact."""
    B = x.shape[0]
    n = B * chunks * 2
    flat = torch.full((n + 2 * 37,), CANARY_F).to(dev)
    buf = frame(x, strided).to(dev)
    before = buf.clone()
    be.lse_partials(view(buf, x, strided), chunks, out=flat[37:37 + n].view(B, chunks, 2))
    got = flat.cpu()
    assert torch.equal(buf, before)  # the logits are only read
    assert (got[:37] == CANARY_F).all() and (got[37 + n:] == CANARY_F).all()
    return got[37:37 + n].view(B, chunks, 2).clone()


def run_finish(be, dev, part, cv, ci, list_len, tok, nlp):
    """(lse, tok_lp, top_lp, top_id) on the CPU; the buffers arrive filled with canaries."""
    B = cv.shape[0]
    outs = [torch.full((B,), CANARY_F), torch.full((B,), CANARY_F), torch.full((B, LOGPROBS_MAX), CANARY_F),
            torch.full((B, LOGPROBS_MAX), CANARY_I, dtype=torch.int32)]
    outs = [o.to(dev) for o in outs]
    be.logprobs_finish(part.to(dev), cv.to(dev), ci.to(dev), list_len, tok.to(dev), nlp.to(dev), *outs)
    return [o.cpu() for o in outs]


def check_partials(part, x, chunks):
    """Every (m, s): m exactly the chunk maximum, s >= 1 and finite or (-inf, 0), never NaN."""
    B, V = x.shape
    Vc = lse_chunk_width(V, chunks)
    assert not torch.isnan(part).any()
    for c in range(chunks):
        seg = x[:, min(c * Vc, V):min((c + 1) * Vc, V)]
        m = seg.max(1).values if seg.shape[1] else torch.full((B,), NEG)
        assert torch.equal(part[:, c, 0], m), c
        dead = m == NEG
        assert (part[dead, c, 1] == 0).all()
        live = part[~dead, c, 1]
        assert (live >= 1.0).all() and (live <= max(1, seg.shape[1])).all()


def check_finish(outs, x, tok, nlp, lse64, bound):
    """The finish outputs of rows x against the oracles; returns the largest |lse - float64| / bound."""
    lse, tok_lp, top_lp, top_id = outs
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    worst = 0.0
    for b in range(x.shape[0]):
        N = int(nlp[b])
        if N < 0:  # a row without logprobs: nothing of it is written
            assert lse[b] == CANARY_F and tok_lp[b] == CANARY_F
            assert (top_lp[b] == CANARY_F).all() and (top_id[b] == CANARY_I).all()
            continue
        err = abs(float(lse[b].double() - lse64[b]))
        assert err <= float(bound[b]), (b, err, float(bound[b]))
        worst = max(worst, err / float(bound[b]))
        assert tok_lp[b] == x[b, int(tok[b])] - lse[b], b  # fp32 subtraction, bit for bit
        assert torch.equal(top_id[b, :N].long(), order[b, :N]), (b, top_id[b, :N], order[b, :N])
        assert torch.equal(top_lp[b, :N], x[b, order[b, :N]] - lse[b]), b
        assert (top_lp[b, N:] == CANARY_F).all() and (top_id[b, N:] == CANARY_I).all()  # slots >= N untouched
    return worst


def check_case(be, dev, case):
    """One kernel case through both launches. Returns the largest lse error-to-bound ratio."""
    x, cv, ci, tok, nlp = build(case)
    chunks = case["chunks"]
    part = run_lse_partials(be, dev, x, chunks, case["strided"])
    check_partials(part, x, chunks)
    assert torch.equal(run_lse_partials(be, dev, x, chunks, case["strided"]), part)  # two launches: identical bits
    lse64, bound = lse_oracle(x)
    outs = run_finish(be, dev, part, cv, ci, case["list_len"], tok, nlp)
    worst = check_finish(outs, x, tok, nlp, lse64, bound)
    again = run_finish(be, dev, part, cv, ci, case["list_len"], tok, nlp)
    assert all(torch.equal(a, b) for a, b in zip(outs, again))
    lse, tok_lp, top_lp, top_id = outs
    if case["special"] == "one_finite" and nlp[4:].numel() and nlp[4] >= 0:
        j = (7 * case["V"]) // 11
        assert lse[4] == x[4, j]  # the lse of one finite entry is that entry, exactly
        if tok[4] == j:
            assert tok_lp[4] == 0.0
        N = int(nlp[4])
        if N > 0:
            assert top_id[4, 0] == j and top_lp[4, 0] == 0.0 and (top_lp[4, 1:N] == NEG).all()
    if case["special"] == "all_equal" and nlp[4:].numel() and nlp[4] > 0:
        assert top_id[4, :int(nlp[4])].tolist() == list(range(int(nlp[4])))
    return worst


def check_two_shards(be, dev, V=4099, chunks=3, seed=5):
    """Two simulated vocab shards of padded width W (the second one narrower: V - W valid columns): partials and
    candidate lists concatenated rank-major, global ids via vocab_offset. Ids equal the unsharded result, the lse
    is within the bound. Returns the largest lse error-to-bound ratio."""
    x = make_rows(V, chunks, "ties", seed)
    W = (((V + 1) // 2) + 7) & ~7
    nlp = torch.tensor([20, 5, 1, 20, 20], dtype=torch.int32)
    K = 64
    parts, cvs, cis = [], [], []
    for off in (0, W):
        sh = x[:, off:min(off + W, V)].contiguous()
        # the chunk count comes from the padded width, so both ranks produce the same number of partials
        p = run_lse_partials(be, dev, sh, chunks, False)
        v, i = chunk_candidates(sh, chunks, K, vocab_offset=off)
        parts.append(p), cvs.append(v), cis.append(i)
    part, cv, ci = torch.cat(parts, 1), torch.cat(cvs, 1), torch.cat(cis, 1)
    tok = ci[:, 2 * K + 1].clone()  # a candidate of the second list
    lse64, bound = lse_oracle(x)
    outs = run_finish(be, dev, part, cv, ci, K, tok, nlp)
    worst = check_finish(outs, x, tok, nlp, lse64, bound)
    # against the unsharded run of the same rows
    p1 = run_lse_partials(be, dev, x, chunks, False)
    v1, i1 = chunk_candidates(x, chunks, K)
    one = run_finish(be, dev, p1, v1, i1, K, tok, nlp)
    assert torch.equal(outs[3], one[3])
    return worst
