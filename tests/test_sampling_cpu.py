"""The sampler's reference (sampling_cases.py) checked without a GPU: the generator against its published value and
for uniformity, the total order against a stable sort, sample_ref against ops.reference, an fp32 emulation of the
kernel's formulas against the band, and the share of ambiguous rows in every table."""
import math

import numpy as np
import pytest
import torch

import sampling_cases as S
from rag_llm_k8s_amd.ops import reference as R

F32 = np.float32
AMBIGUOUS_CAP = 0.02


# ----------------------------------------------------------------------------- the generator
def test_splitmix64_published_value():
    assert S.splitmix64(0) == 0xE220A8397B1DCDAF
    # the sequence x_{n+1} = splitmix64 of the advancing state: second and third published outputs
    assert S.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert S.splitmix64(2 * 0x9E3779B97F4A7C15 & S.MASK64) == 0x06C45D188009454F


def test_uniform_range_resolution_and_argument_widths():
    us = [S.uniform(s, t) for s in (0, 1, -1, 2 ** 63 - 1, -2 ** 63) for t in (0, 1, 2 ** 31 - 1, -1)]
    assert all(0.0 <= u < 1.0 and u * 2 ** 24 == int(u * 2 ** 24) for u in us)
    assert S.uniform(-1, 5) == S.uniform(2 ** 64 - 1, 5)  # seeds modulo 2**64
    assert S.uniform(3, -1) == S.uniform(3, 2 ** 64 - 1) != S.uniform(3, 2 ** 32 - 1)  # int32 step, sign extended
    assert len(set(us)) == len(us)


def _chi2(counts, expected):
    return float(((np.asarray(counts, dtype=np.float64) - expected) ** 2 / expected).sum())


def test_uniform_is_uniform_over_seeds_and_steps():
    """Deciles of u over a fixed 200 x 200 seeds x steps grid, along 40 000 consecutive steps of one seed and along
    40 000 consecutive seeds of one step (chi-square, 9 degrees of freedom), and the 10 x 10 table of consecutive
    (u_t, u_t+1) pairs along the steps (99 degrees of freedom). Significance level 0.001 each: critical values
    27.88 and 148.23. The inputs are fixed, so the test is deterministic."""
    rng = np.random.default_rng(2024)
    seeds = [int(s) for s in rng.integers(-(1 << 63), 1 << 63, 200, dtype=np.int64)]
    steps = [int(s) for s in rng.integers(0, 1 << 31, 200, dtype=np.int64)]
    grid = np.array([[S.uniform(s, t) for t in steps] for s in seeds])
    n = grid.size
    for name, u in (("grid", grid.ravel()), ("steps", np.array([S.uniform(seeds[0], t) for t in range(n)])),
                    ("seeds", np.array([S.uniform(s, steps[0]) for s in range(n)]))):
        counts = np.bincount((u * 10).astype(int), minlength=10)
        print(name, "decile counts", counts.min(), "..", counts.max(), "chi2 %.2f" % _chi2(counts, n / 10))
        assert _chi2(counts, n / 10) < 27.88, name
        if name == "steps":
            d = (u * 10).astype(int)
            pairs = np.bincount(d[:-1] * 10 + d[1:], minlength=100)
            assert _chi2(pairs, (n - 1) / 100) < 148.23
    # rows and columns of the grid: no seed and no step with a degenerate stream (200 draws each, mean 0.5 with
    # standard deviation 0.0204: six sigma)
    assert np.abs(grid.mean(0) - 0.5).max() < 0.123 and np.abs(grid.mean(1) - 0.5).max() < 0.123


# ----------------------------------------------------------------------------- the total order
def test_merge_is_the_stable_sort_by_value_unsigned_id_position():
    rng = np.random.default_rng(5)
    for trial in range(50):
        n = int(rng.integers(1, 200))
        v = rng.choice(np.array([3.0, 1.5, 0.0, -0.0, -2.0, S.NEG], dtype=F32), n)
        i = rng.choice(np.array([-1, 0, 1, 7, 7, 2 ** 31 - 1, 90000], dtype=np.int32), n)
        mv, mi = S.merge(v, i)
        key = sorted(range(n), key=lambda j: (-float(v[j]) + 0.0, int(i[j]) % 2 ** 32, j))  # (-0.0 + 0.0 = 0.0)
        assert np.array_equal(mv.view(np.uint32), v[key].view(np.uint32))
        assert mi.tolist() == [int(i[j]) for j in key]
    mv, mi = S.merge([1.0, S.NEG, 1.0, S.NEG, 1.0], [5, -1, -1, 3, 2])
    assert mi.tolist() == [2, 5, -1, 3, -1] and mv.tolist() == [1.0, 1.0, 1.0, S.NEG, S.NEG]


def test_topk_ref_and_kernel_rule():
    v, i = S.topk_ref(np.array([1.0, 3.0, 3.0, -1.0, 3.0], dtype=F32), 4, vocab_offset=10)
    assert v.tolist() == [3.0, 3.0, 3.0, 1.0] and i.tolist() == [11, 12, 14, 10]
    v, i = S.topk_ref(np.array([2.0, S.NEG], dtype=F32), 4)
    assert v.tolist() == [2.0, S.NEG, S.NEG, S.NEG] and i.tolist() == [0, 1, -1, -1]
    cases = S.topk_cases()
    assert len({n for n, _ in cases}) == len(cases)
    for name, c in cases:
        assert S.topk_kernel(c["V"], c["chunks"], c["K"]) == c["kernel"], name
        assert c["ld"] >= c["V"]
    assert {c["kernel"] for _, c in cases} == {"wave", "lds", "generic"}
    # every K on every kernel that takes it; the wave kernel's shape with K > 64 is the LDS kernel's
    for kern, ks in (("wave", {1, 50, 64}), ("lds", {1, 50, 64, 65, 256}), ("generic", {1, 50, 64, 65, 256})):
        assert ks <= {c["K"] for _, c in cases if c["kernel"] == kern}
    assert S.topk_kernel(5000, 8, 64) == "wave" and S.topk_kernel(5000, 8, 65) == "lds"
    assert S.topk_kernel(24576, 1, 50) == "lds" and S.topk_kernel(24577, 1, 50) == "generic"
    assert any(c["ld"] > c["V"] for _, c in cases) and any(c["vocab_offset"] for _, c in cases)
    assert any(c["V"] < c["K"] for _, c in cases)
    for _, c in cases[:3] + cases[-5:]:
        x = S.topk_rows(c)
        assert x.shape == (len(S.CONTENTS), c["V"]) and x.dtype == F32 and not np.isnan(x).any()


def test_run_at_kth_rows_straddle_the_kth_place():
    """The tie rows do what they are for: in a chunk that holds the run, fewer than K values lie above the run and
    more than K - that many run entries are in the chunk."""
    for _, c in S.topk_cases():
        V, chunks, K = c["V"], c["chunks"], c["K"]
        if min(V, S.chunk_width(V, chunks)) < 2 * K + 2 or K < 2:  # (chunks shorter than the run; K = 1)
            continue
        x = S.topk_rows(c)[S.CONTENTS.index("run-at-kth")]
        Vc = S.chunk_width(V, chunks)
        hit = 0
        for ch in range(chunks):
            sl = x[ch * Vc:(ch + 1) * Vc]
            run, above = int((sl == 1.0).sum()), int((sl > 1.0).sum())
            if run and above < K < above + run:
                hit += 1
        assert hit >= 1, c


# ----------------------------------------------------------------------------- sample_ref
def test_sample_ref_known_rows():
    # p = (0.5, 0.25, 0.25) at T = 1: values log 2 apart are not exact, so use the EXACT row instead: 4 x 0.25
    t = S.exact_table(per=1)
    for b in range(t["cv"].shape[0]):
        tok, lp, band, alts = S.sample_ref(t["cv"][b], t["ci"][b], t["T"][b], int(t["top_k"][b]), t["top_p"][b],
                                           int(t["seed"][b]), int(t["step"][b]), exact=True)
        keep = int(round(float(t["top_p"][b]) * 4))  # i / 4 < top_p  <=>  i < 4 top_p
        u = S.uniform(int(t["seed"][b]), int(t["step"][b]))
        assert tok == [20, 21, 300, 100000][min(int(u * keep), keep - 1)] and not alts
        assert lp == -math.log(keep)
        # without `exact` the same row is ambiguous: the comparison sits on the boundary
        assert S.sample_ref(t["cv"][b], t["ci"][b], t["T"][b], int(t["top_k"][b]), t["top_p"][b], int(t["seed"][b]),
                            int(t["step"][b]))[3]
    # K: disabled when <= 0 or > n_cand; a banned token ends the valid run
    v, i = np.array([2.0, 1.0, S.NEG, 0.5], dtype=F32), np.array([4, 5, 6, 7], dtype=np.int32)
    for k in (0, -1, 9, 4, 3):
        u = S.uniform(1, 2)
        tok, lp, _, _ = S.sample_ref(v, i, 1.0, k, 1.0, 1, 2)
        p = np.exp([2.0, 1.0, 0.5])
        p /= p.sum()  # (-inf sorts last: the three finite candidates lead)
        j = int(np.searchsorted(np.cumsum(p), u, side="right"))
        assert tok == [4, 5, 7][j] and abs(lp - math.log(p[j])) < 1e-12


def test_edges_are_unambiguous_and_as_stated():
    names = [e["name"] for e in S.edges()]
    assert len(set(names)) == len(names)
    for e in S.edges():
        tok, lp, band, alts = S.sample_ref(e["cv"], e["ci"], e["T"], e["top_k"], e["top_p"], e["seed"], e["step"])
        assert not alts, e["name"]
        if "token" in e:
            assert tok == e["token"], e["name"]
        if "logprob" in e:
            assert lp == e["logprob"], e["name"]
        for L in e["list_lens"]:
            assert L is None or e["cv"].size % L == 0
    want = {"all-padding", "greedy-T0-tie", "greedy-T-neg-tie", "greedy-T-nan-tie", "top_p-0-tie", "top_p-1",
            "top_k-1-tie", "top_k-64", "top_k-65", "few-valid", "banned-in-top-k", "padded-list-ends",
            "ties-across-lists", "one-hot-T0.01"}
    assert want <= set(names)
    by = {e["name"]: e for e in S.edges()}
    a, b = by["top_k-64"], by["top_k-65"]
    assert np.array_equal(a["cv"], b["cv"]) and a["seed"] == b["seed"]  # the same candidates and draw


def test_sample_ref_agrees_with_ops_reference():
    """With the same u, sample_ref picks the token of R.sample_from_logits_candidates (fp32 torch) on unambiguous
    rows."""
    rng = np.random.default_rng(31)
    B, n = 400, 96
    v, i = S.random_candidates(rng, B, n)
    p = S.draw_params(rng, B, rng.integers(1, n + 1, B))
    checked = 0
    for b in range(B):
        tok, _, _, alts = S.sample_ref(v[b], i[b], p["T"][b], int(p["top_k"][b]), p["top_p"][b], int(p["seed"][b]),
                                       int(p["step"][b]))
        if alts:
            continue
        mv, mi = S.merge(v[b], i[b])
        k = int(p["top_k"][b])
        ok = (mv[:k] > S.NEG) & (mi[:k] >= 0)
        k = k if ok.all() else int(np.argmin(ok))
        u = S.uniform(int(p["seed"][b]), int(p["step"][b]))
        _, _, pick = R.sample_from_logits_candidates(torch.from_numpy(mv[:k].copy()), torch.from_numpy(mi[:k].copy()),
                                                     float(p["T"][b]), float(p["top_p"][b]), u)
        assert pick == tok, b
        checked += 1
    assert checked > 0.95 * B


# ----------------------------------------------------------------------------- the fp32 emulation
def _expf(x):
    """__expf as the hardware forms it: exp2 of the fp32 product with log2(e)."""
    with np.errstate(invalid="ignore"):
        return np.exp2((x * F32(1.4426950408889634)).astype(F32)).astype(F32)


def _butterfly_sum(x):
    x = x.copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = (x + x[:, lane ^ o]).astype(F32)
    return x[:, 0]


def _lane_scan(x):
    x = x.copy()
    for o in (1, 2, 4, 8, 16, 32):
        y = x.copy()
        y[:, o:] = (x[:, o:] + x[:, :-o]).astype(F32)
        x = y
    return x


def _emulate(v, valid, T, top_p, u, wave):
    """The kernel's formulas in numpy float32, same order of operations: the wave path (one candidate per lane,
    butterfly sums and shuffle scans) or the serial tail. v [N, n] sorted, valid [N]. Returns (pick, keep, the
    normalised cum_before and cumulative sums as the kernel compares them)."""
    N, n = v.shape
    idx = np.arange(n)[None, :]
    live = idx < valid[:, None]
    inv_t = (F32(1.0) / T).astype(F32)
    m = (v[:, 0] * inv_t).astype(F32)
    arg = ((v * inv_t[:, None]).astype(F32) - m[:, None]).astype(F32)
    e = np.where(live, _expf(arg), F32(0.0)).astype(F32)
    if wave:
        Z = _butterfly_sum(e)
        q = (((_lane_scan(e) - e).astype(F32)) / Z[:, None]).astype(F32)
    else:
        Z = np.cumsum(e, axis=1, dtype=F32)[:, -1]
        cum = np.cumsum((e / Z[:, None]).astype(F32), axis=1, dtype=F32)
        q = np.concatenate([np.zeros((N, 1), dtype=F32), cum[:, :-1]], axis=1)
    kept = live & ((top_p >= 1)[:, None] | (idx == 0) | (q < top_p[:, None]))
    if not wave:  # the tail stops at the first candidate whose mass above reaches top_p
        kept = np.cumprod(kept, axis=1).astype(bool)
    keep = kept.sum(1)
    ek = np.where(kept, e, F32(0.0)).astype(F32)
    if wave:
        Zk, ck = _butterfly_sum(ek), _lane_scan(ek)
    else:
        ck = np.cumsum(ek, axis=1, dtype=F32)
        Zk = ck[np.arange(N), keep - 1]
    uf = (u.astype(F32) * Zk).astype(F32)
    hit = kept & (uf[:, None] < ck)
    last = n - 1 - np.argmax(kept[:, ::-1], axis=1)
    pick = np.where(hit.any(1), np.argmax(hit, axis=1), last)
    return pick, keep, q, (ck / Zk[:, None]), kept


@pytest.mark.parametrize("form,n,N", [("wave", 64, 12000), ("tail", 512, 12000)])
def test_fp32_emulation_stays_inside_the_band(form, n, N):
    """12 000 random rows per form (24 000 in all): the fp32 pick equals the float64 pick on unambiguous rows and
    is one of the alternatives otherwise; the fp32 normalised sums stay within the band of the float64 ones
    (printed: the worst deviation in units of the band)."""
    rng = np.random.default_rng(90 + n)
    v = -np.sort(-(rng.standard_normal((N, n)) * 3).astype(F32), axis=1)
    ids = np.arange(n, dtype=np.int32)
    top_k = rng.integers(1, 65, N) if form == "wave" else rng.integers(65, n + 1, N)
    p = S.draw_params(rng, N, top_k)
    u = np.array([S.uniform(int(s), int(t)) for s, t in zip(p["seed"], p["step"])])
    valid = p["top_k"].astype(np.int64)
    pick, keep, q, cdf, kept = _emulate(v, valid, p["T"], p["top_p"], u, form == "wave")
    # float64, vectorised, for the deviations
    inv_t = (F32(1.0) / p["T"]).astype(np.float64)
    live = np.arange(n)[None, :] < valid[:, None]
    x = v.astype(np.float64) * inv_t[:, None]
    e = np.where(live, np.exp(x - x[:, :1]), 0.0)
    c = np.cumsum(e, axis=1)
    band = 4.0 * (2.0 ** -22 * (1.0 + np.where(live, np.abs(x), 0.0).max(1)) + valid * 2.0 ** -24)
    dev_q = (np.where(live, np.abs(q - (c - e) / c[:, -1:]), 0.0).max(1) / band).max()
    n_amb, dev_c = 0, 0.0
    for b in range(N):
        tok, _, bd, alts = S.sample_ref(v[b], ids, p["T"][b], int(p["top_k"][b]), p["top_p"][b], int(p["seed"][b]),
                                        int(p["step"][b]))
        assert abs(bd - band[b]) <= 1e-12 * band[b]
        if alts:
            n_amb += 1
            assert int(pick[b]) in alts, (b, int(pick[b]), alts)
            continue
        assert int(pick[b]) == tok, (b, int(pick[b]), tok)
        k = int(keep[b])  # same token and unambiguous: the same kept prefix
        dev_c = max(dev_c, float(np.abs(cdf[b, :k] - c[b, :k] / c[b, k - 1]).max() / band[b]))
    print("%s form: worst |fp32 - float64| / band: cum_before/Z %.3f, c/Zk %.3f; ambiguous rows %d of %d"
          % (form, dev_q, dev_c, n_amb, N))
    assert dev_q < 1.0 and dev_c < 1.0


# ----------------------------------------------------------------------------- the tables
def _share(alts):
    return sum(1 for a in alts if a) / len(alts)


def test_tables_have_few_ambiguous_rows_and_independent_parameters():
    t = S.routes_table()
    B = t["T"].size
    assert B <= 512 and S.ROUTES_N <= 2048
    for key in ("T", "top_k", "seed", "step"):  # no two neighbouring rows share a value
        assert (t[key][1:] != t[key][:-1]).all(), key
    assert (t["top_p"][1:] != t["top_p"][:-1]).mean() > 0.6 and set(t["top_p"].tolist()) == {F32(p) for p in S.TOP_PS}
    assert (t["seed"] < 0).any() and (t["seed"] > 0).any() and t["step"].max() == 2 ** 31 - 1
    assert 0.2 <= t["T"].min() and t["T"].max() <= 2.0
    ks = set(t["top_k"].tolist())
    assert {65, 128, 256, S.ROUTES_N, 0, -1} <= ks and min(k for k in ks if k > 0) <= 4
    assert ((t["top_k"] > 0) & (t["top_k"] <= 64)).sum() >= B // 2
    shares = {}
    refs = []
    for name, (cv, ci, L) in t["shapes"].items():
        if L:  # every list in the total order, as the list merges assume
            for b in range(0, B, 37):
                assert all(np.array_equal(S.merge(cv[b, g:g + L], ci[b, g:g + L])[1], ci[b, g:g + L])
                           for g in range(0, cv.shape[1], L))
        refs.append(S.ref_rows(cv, ci, t["T"], t["top_k"], t["top_p"], t["seed"], t["step"]))
    for r in refs[1:]:  # the shaping does not change the reference
        assert np.array_equal(r[0], refs[0][0]) and np.array_equal(r[1], refs[0][1])
    shares["ROUTES"] = _share(refs[0][3])
    for name, s in S.steps_tables().items():
        r = S.ref_rows(s["cv"], s["ci"], s["T"], s["top_k"], s["top_p"], s["seed"], s["step"])
        shares["STEPS " + name] = _share(r[3])
        assert len(set(r[0].tolist())) >= 8, name  # the argument under test moves the token
    for name, V, chunks, K, kmax in S.END_TO_END:
        x, p = S.end_to_end_table(V, chunks, K, kmax)
        cv, ci = S.topk_lists_ref(x, chunks, K)
        r = S.ref_rows(cv, ci, p["T"], p["top_k"], p["top_p"], p["seed"], p["step"])
        shares["END_TO_END " + name] = _share(r[3])
    print(" ".join("%s %.2f%%" % (k, 100 * v) for k, v in shares.items()))
    for k, v in shares.items():
        assert v <= AMBIGUOUS_CAP, (k, v)
    e = S.exact_table()
    assert not any(S.ref_rows(e["cv"], e["ci"], e["T"], e["top_k"], e["top_p"], e["seed"], e["step"], exact=True)[3])
