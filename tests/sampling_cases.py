"""Reference and case tables of the sampler tests (test_sampling_cpu.py / test_sampling_gpu.py): plain Python and
numpy, importable without a GPU.

The sampler (csrc/kernels/sampling.hip) is deterministic: per row u = top 24 bits of
splitmix64(seed ^ splitmix64(step + 0x51ED270B)) / 2**24, the candidates in the total order (value desc, id asc as
unsigned, position asc), temperature, top-k, top-p (candidate i kept iff i == 0, top_p >= 1, or the mass ranked
strictly above it, over Z, is < top_p), then the inverse CDF over the kept ones. sample_ref() does exactly this in
float64 and so says which token every row must produce.

The band. fp32 on the GPU cannot follow float64 where u * Zk or top_p falls within rounding of a cumulative sum.
Per row, in units of normalised probability,

    band = 4 * (2**-22 * (1 + max_i |v_i * inv_t|) + n_valid * 2**-24)

  * 2**-22 * (1 + max |x|): x = v * inv_t - m is formed in fp32 from two roundings of numbers of size <= max |x|
    (2 * 2**-24 * max |x| absolute), __expf multiplies by log2(e) (another 2**-24 * |x|) and returns an fp32 (2**-24
    relative, with the 1 + standing for the hardware exp2's own ulp): an absolute error in the exponent is a
    relative error in the term, so every term, and with it every normalised sum of terms, moves by at most
    about 2**-22 * (1 + max |x|);
  * n_valid * 2**-24: each of the at most n_valid - 1 fp32 additions of a cumulative sum rounds by 2**-24 of a
    partial sum that is at most the total, so a normalised cumulative sum moves by at most n_valid * 2**-24 (the
    serial tail; the shuffle scans of the wave path have depth 6);
  * the factor 4 is margin (the division by Z, the product u * Zk, Z and Zk themselves moving).

A row is ambiguous when |cum_before_i / Z - top_p| < band for some i >= 1 (top_p < 1), or |c_i / Zk - u| < band for
some kept i; its `alternatives` are the tokens reached by resolving each such comparison either way. The bound is
set against an fp32 emulation of the kernel's formulas on the CPU (test_sampling_cpu.py), never against a GPU.

Measured there over 24 000 random rows (12 000 per form, parameter ranges of the tables): the largest
|fp32 - float64| / band is 0.044 (cum_before / Z) and 0.034 (c / Zk) for the wave-path form (one candidate per
lane, butterfly sums and shuffle scans), 0.034 and 0.030 for the serial-tail form (K > 64, up to 512 candidates);
no emulated pick left the alternatives, so the factor 4 stands. Of those rows 0.13 % (wave form) and 5.0 % (tail
form: the band and the number of comparisons both grow with the candidate count) are ambiguous.
Ambiguous rows by table (reference alone): ROUTES 1.56 % (6 of 384, all of them serial-tail rows), STEPS 0 % / 0 %,
END_TO_END 0 % in all five, EDGES and EXACT none (asserted).
"""
import math

import numpy as np

NEG = float("-inf")
MASK64 = (1 << 64) - 1
SENT_TOK = -12345  # the output buffers of the GPU tests arrive filled with this token / NaN


# ----------------------------------------------------------------------------- the draw
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def uniform(seed, step):
    """u in [0, 1), 24 bits. seed: any int, taken modulo 2**64; step: an int32, widened to unsigned 64 as the
    kernel's (unsigned long long)steps[b] does (sign extension)."""
    r = splitmix64((int(seed) & MASK64) ^ splitmix64((int(step) & MASK64) + 0x51ED270B))
    return (r >> 40) / 16777216.0


# ----------------------------------------------------------------------------- the sampler
def merge(cand_v, cand_i):
    """The candidates of one row in the sampler's total order: value descending (float comparison, so +0 == -0),
    id ascending as unsigned (padding id -1 last), position ascending."""
    v = np.asarray(cand_v, dtype=np.float32)
    i = np.asarray(cand_i, dtype=np.int32)
    order = np.lexsort((np.arange(v.size), i.astype(np.int64) & 0xFFFFFFFF, -v))
    return v[order], i[order]


def sample_ref(cand_v, cand_i, T, top_k, top_p, seed, step, exact=False):
    """(token, logprob, band, alternatives) of one row, in float64. `alternatives` is empty for an unambiguous row
    and otherwise holds every token an fp32 evaluation may return (the float64 one among them). exact: the row's
    arithmetic is exact in fp32 as well (the EXACT table), so no comparison is ambiguous however close."""
    v, ids = merge(cand_v, cand_i)
    n = v.size
    K = n if (top_k <= 0 or top_k > n) else int(top_k)
    ok = (v[:K] > NEG) & (ids[:K] >= 0)
    valid = K if ok.all() else int(np.argmin(ok))
    if valid == 0:
        return 0, NEG, 0.0, set()
    T = np.float32(T)
    if not (T > 0):  # greedy, NaN included
        return int(ids[0]), 0.0, 0.0, set()
    inv_t = float(np.float32(1.0) / T)
    x = v[:valid].astype(np.float64) * inv_t
    m = x[0]
    e = np.exp(x - m)
    c = np.cumsum(e)
    Z = c[-1]
    band = 4.0 * (2.0 ** -22 * (1.0 + float(np.abs(x).max())) + valid * 2.0 ** -24)
    near_band = 0.0 if exact else band
    p = float(np.float32(top_p))
    keep, keeps = valid, {valid}
    ambiguous = False
    if p < 1.0:
        q = (c - e)[1:] / Z  # mass ranked strictly above candidates 1 ..
        over = np.nonzero(q >= p)[0]
        keep = int(over[0]) + 1 if over.size else valid
        near = np.nonzero(np.abs(q - p) < near_band)[0] + 1
        keeps = {keep}
        if near.size:
            ambiguous = True
            keeps |= set(range(int(near[0]), int(near[-1]) + 2))
    u = uniform(seed, step)

    def draw(k):
        Zk = c[k - 1]
        hit = np.nonzero(u * Zk < c[:k])[0]
        pick = int(hit[0]) if hit.size else k - 1
        return pick, Zk, np.nonzero(np.abs(c[:k] / Zk - u) < near_band)[0]

    pick, Zk, near_u = draw(keep)
    ambiguous = ambiguous or near_u.size > 0
    alts = set()
    if ambiguous:
        for k in keeps:
            pk, _, nu = draw(k)
            alts.add(int(ids[pk]))
            for j in nu:
                alts.add(int(ids[j]))
                alts.add(int(ids[min(int(j) + 1, k - 1)]))
    return int(ids[pick]), float(x[pick] - m - math.log(Zk)), band, alts


def ref_rows(cv, ci, T, top_k, top_p, seed, step, exact=False):
    """sample_ref over the rows of a table: (tok int64 [B], lp float64 [B], band float64 [B], alternatives list)."""
    out = [sample_ref(cv[b], ci[b], T[b], int(top_k[b]), top_p[b], int(seed[b]), int(step[b]), exact)
           for b in range(cv.shape[0])]
    return (np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out], dtype=np.float64),
            np.array([o[2] for o in out], dtype=np.float64), [o[3] for o in out])


# ----------------------------------------------------------------------------- the candidate top-k
TK_VMAX, TW_VMAX = 24576, 6144  # chunk widths the LDS kernel / the wave kernel take (sampling.hip)


def chunk_width(V, chunks):
    return ((V + chunks - 1) // chunks + 7) & ~7


def topk_kernel(V, chunks, K):
    """Which kernel ragk_topk_candidates launches for this shape."""
    Vc = chunk_width(V, chunks)
    if K <= 64 and Vc <= TW_VMAX and chunks >= 8:
        return "wave"
    return "lds" if Vc <= TK_VMAX else "generic"


def topk_ref(row, K, vocab_offset=0):
    """(values [K], ids [K]) of one chunk's slice: value descending, ties lowest id first, padded (-inf, -1)."""
    row = np.asarray(row, dtype=np.float32)
    order = np.lexsort((np.arange(row.size), -row))[:K]
    v = np.full(K, NEG, dtype=np.float32)
    i = np.full(K, -1, dtype=np.int32)
    v[:order.size] = row[order]
    i[:order.size] = order + vocab_offset
    return v, i


def topk_lists_ref(x, chunks, K, vocab_offset=0):
    """[B, chunks * K] (values, ids): topk_ref of every chunk of every row of x [B, V]."""
    B, V = x.shape
    Vc = chunk_width(V, chunks)
    cv = np.full((B, chunks, K), NEG, dtype=np.float32)
    ci = np.full((B, chunks, K), -1, dtype=np.int32)
    for c in range(chunks):
        lo, hi = min(c * Vc, V), min((c + 1) * Vc, V)
        for b in range(B):
            cv[b, c], ci[b, c] = topk_ref(x[b, lo:hi], K, vocab_offset + lo)
    return cv.reshape(B, -1), ci.reshape(B, -1)


# ----------------------------------------------------------------------------- tables: parameters
TOP_PS = (0.1, 0.5, 0.9, 0.95, 1.0)


def draw_params(rng, B, top_k):
    """Independent per-row parameters: T in [0.2, 2], top_p of TOP_PS, signed 64-bit seeds, steps up to 2**31 - 1
    (the first two rows hold the extremes)."""
    step = rng.integers(0, 1 << 31, B, dtype=np.int64)
    step[:2] = ((1 << 31) - 1, 0)[:B]
    return dict(T=rng.uniform(0.2, 2.0, B).astype(np.float32), top_k=np.asarray(top_k, dtype=np.int32),
                top_p=rng.choice(np.array(TOP_PS, dtype=np.float32), B),
                seed=rng.integers(-(1 << 63), 1 << 63, B, dtype=np.int64), step=step.astype(np.int32))


def shape_lists(v, i, L):
    """The row's candidates as n / L lists of L (consecutive groups), each in the total order."""
    ov, oi = np.empty_like(v), np.empty_like(i)
    for g in range(0, v.size, L):
        ov[g:g + L], oi[g:g + L] = merge(v[g:g + L], i[g:g + L])
    return ov, oi


def random_candidates(rng, B, n, vocab=131072):
    """[B, n] random values (randn * 3) with distinct ids ascending along the row, so that consecutive groups are
    vocabulary chunks. Every 8th row has quantised values (exact ties across lists), every other 8th row ends each
    group of 32 in (-inf, -1) padding and holds banned tokens (-inf with a real id)."""
    v = (rng.standard_normal((B, n)) * 3).astype(np.float32)
    i = np.empty((B, n), dtype=np.int32)
    for b in range(B):
        i[b] = np.sort(rng.choice(vocab, n, replace=False))
        if b % 8 == 3:
            v[b] = np.round(v[b] * 2) / 2
        if b % 8 == 5:
            for g in range(0, n, 32):
                pad = int(rng.integers(0, 9))
                v[b, g + 32 - pad:g + 32] = NEG
                i[b, g + 32 - pad:g + 32] = -1
            ban = rng.choice(n, 6, replace=False)
            v[b, ban] = NEG
    return v, i


# ROUTES: the same rows shaped for each branch of sample_candidates_kernel. n = 320 candidates (with 512 the serial
# tail's band, which grows with the candidate count, makes 3 to 4 % of the rows ambiguous whatever the seed):
#   "sort":  no list_len -- bitonic sort, then the wave path;
#   "rank":  5 lists of 64 -- rank merge by binary search;
#   "lanes": 10 lists of 32 -- lane-network merge;
# and whatever the shaping, rows with K > 64 (half of them: 65, 128, 256, n, 0, -1 and random) sort and take the
# serial tail.
ROUTES_N = 320
ROUTE_SHAPES = (("sort", None), ("rank", 64), ("lanes", 32))
ROUTES_SEED = 20260


def routes_table(B=384, seed=ROUTES_SEED):
    rng = np.random.default_rng(seed)
    n = ROUTES_N
    v, i = random_candidates(rng, B, n)
    wide = (65, 128, 256, n, 0, -1)
    top_k = [int(rng.integers(1, 65)) if b % 2 == 0 else
             wide[(b // 2) % 12] if (b // 2) % 12 < 6 else int(rng.integers(65, n + 1)) for b in range(B)]
    t = dict(draw_params(rng, B, top_k), shapes={})
    for name, L in ROUTE_SHAPES:
        sv, si = np.empty_like(v), np.empty_like(i)
        for b in range(B):
            sv[b], si[b] = shape_lists(v[b], i[b], L or 32)
        t["shapes"][name] = (sv, si, L)
    return t


# STEPS: one row of candidates 256 times; one seed with steps 0..255, then one step with seeds 0..255.
def steps_tables(seed=77):
    rng = np.random.default_rng(seed)
    v, i = random_candidates(rng, 1, 128)
    v, i = shape_lists(v[0], i[0], 64)
    B = 256
    base = dict(cv=np.tile(v, (B, 1)), ci=np.tile(i, (B, 1)), list_len=64, T=np.full(B, 2.0, dtype=np.float32),
                top_k=np.full(B, 50, dtype=np.int32), top_p=np.full(B, 0.95, dtype=np.float32))
    by_step = dict(base, seed=np.full(B, -0x1234567890ABCDEF, dtype=np.int64), step=np.arange(B, dtype=np.int32))
    by_seed = dict(base, seed=np.arange(B, dtype=np.int64), step=np.full(B, 1 << 20, dtype=np.int32))
    return {"by_step": by_step, "by_seed": by_seed}


# ----------------------------------------------------------------------------- EDGES
def _edge_lists(rng, R, L, n_valid=None):
    """R lists of L random candidates in the total order; with n_valid, each list keeps n_valid real entries and
    ends in (-inf, -1) padding."""
    v, i = random_candidates(rng, 1, R * L)
    v, i = v[0].copy(), i[0].copy()
    if n_valid is not None:
        for g in range(0, R * L, L):
            v[g + n_valid:g + L] = NEG
            i[g + n_valid:g + L] = -1
    return shape_lists(v, i, L)


def _unambiguous(e, want=None):
    """Advance the edge's seed until the reference is unambiguous (and u satisfies `want`)."""
    while True:
        ok = want is None or want(uniform(e["seed"], e["step"]))
        if ok and not sample_ref(e["cv"], e["ci"], e["T"], e["top_k"], e["top_p"], e["seed"], e["step"])[3]:
            return e
        e["seed"] += 1


def edges():
    """One row each: dict(name, cv, ci, list_lens (the shapings to run, None = no list_len), T, top_k, top_p, seed,
    step, and where the outcome is known without the reference, token / logprob -- a logprob only for greedy and
    empty rows, which are exact; a sampled row's lone kept candidate gives x - m - log(1) in fp32, zero only up to
    the rounding of m)."""
    rng = np.random.default_rng(4242)
    out = []

    def add(name, cv, ci, list_lens, T, top_k, top_p, seed=12345, step=7, want=None, **known):
        e = dict(name=name, cv=np.asarray(cv, dtype=np.float32), ci=np.asarray(ci, dtype=np.int32),
                 list_lens=list_lens, T=np.float32(T), top_k=top_k, top_p=np.float32(top_p), seed=seed, step=step,
                 **known)
        out.append(_unambiguous(e, want))

    n = 128
    both = (None, 64, 8)  # sort, rank merge (2 lists of 64), lane network (16 lists of 8)
    add("all-padding", np.full(n, NEG), np.full(n, -1), both, 0.7, 50, 0.9, token=0, logprob=NEG)
    add("all-banned", np.full(n, NEG), np.arange(n), both, 0.7, 50, 0.9, token=0, logprob=NEG)
    add("all-padding-tail", np.full(n, NEG), np.full(n, -1), both, 0.7, 100, 0.9, token=0, logprob=NEG)
    # the row maximum twice, the lower id in the later list: the lower id leads the total order
    v, i = _edge_lists(rng, 2, 64)
    top = float(v.max()) + 1.0
    v[0], v[64] = top, top
    i[0], i[64] = 900000, 17
    for name, T in (("greedy-T0", 0.0), ("greedy-T-neg", -1.0), ("greedy-T-nan", float("nan"))):
        add(name + "-tie", v, i, (None, 64), T, 50, 0.9, token=17, logprob=0.0)
        add(name + "-tie-tail", v, i, (None, 64), T, 100, 0.9, token=17, logprob=0.0)
    add("top_p-0-tie", v, i, (None, 64), 1.0, 50, 0.0, token=17)
    add("top_p-0-tie-tail", v, i, (None, 64), 1.0, 0, 0.0, token=17)
    add("top_k-1-tie", v, i, (None, 64), 1.3, 1, 1.0, token=17)
    v, i = _edge_lists(rng, 16, 8)
    add("top_p-1", v, i, both, 0.9, 50, 1.0, want=lambda u: u > 0.5)
    add("top_p-1-tail", v, i, both, 0.9, -1, 1.0, want=lambda u: u > 0.5)
    add("top_k-64", v, i, both, 1.5, 64, 1.0, want=lambda u: u > 0.98)  # the wave path's last lanes
    add("top_k-65", v, i, both, 1.5, 65, 1.0, seed=out[-1]["seed"], want=lambda u: u > 0.98)  # the serial tail
    # fewer valid candidates than top_k: 16 lists of 8 with 1 real entry each, padding interleaved at list ends
    v, i = _edge_lists(rng, 16, 8, n_valid=1)
    add("few-valid", v, i, both, 2.0, 50, 1.0, want=lambda u: u > 0.9)
    add("few-valid-tail", v, i, both, 2.0, 100, 1.0, want=lambda u: u > 0.9)
    v, i = _edge_lists(rng, 16, 8, n_valid=5)
    add("padded-list-ends", v, i, both, 1.0, 60, 0.95)
    add("padded-list-ends-tail", v, i, both, 1.0, 0, 0.95)
    # banned tokens (-inf, real id) inside the top K: 7 finite candidates, u near 1 -- the last finite one, never a
    # banned one
    v, i = _edge_lists(rng, 16, 8)
    fin = rng.choice(n, 7, replace=False)
    keep = np.zeros(n, dtype=bool)
    keep[fin] = True
    v = np.where(keep, (rng.standard_normal(n) * 0.3).astype(np.float32), np.float32(NEG))
    v, i = shape_lists(v, i, 8)
    last = int(merge(v, i)[1][6])
    add("banned-in-top-k", v, i, both, 2.0, 50, 1.0, want=lambda u: u > 0.97, token=last)
    add("banned-in-top-k-tail", v, i, both, 2.0, 0, 1.0, want=lambda u: u > 0.97, token=last)
    # exact value ties across lists: four values only
    v, i = _edge_lists(rng, 16, 8)
    v = rng.choice(np.array([1.0, 0.5, 0.0, -0.5], dtype=np.float32), n)
    v, i = shape_lists(v, i, 8)
    add("ties-across-lists", v, i, both, 0.8, 40, 0.9)
    add("ties-across-lists-tail", v, i, both, 0.8, 100, 0.9)
    # near one-hot at T = 0.01: every other term underflows
    v, i = _edge_lists(rng, 16, 8)
    v = np.minimum(v, np.float32(9.0))
    j = int(rng.integers(0, n))
    v[j] = 10.0
    tok = int(i[j])
    v, i = shape_lists(v, i, 8)
    add("one-hot-T0.01", v, i, both, 0.01, 50, 0.9, want=lambda u: u < 0.99, token=tok)
    add("one-hot-T0.01-tail", v, i, both, 0.01, 0, 0.9, want=lambda u: u < 0.99, token=tok)
    # an entry with a real value and id -1 tying with the lowest real candidate (no top-k emits one; the total
    # order still places it: after every real id of its value): four close candidates, u near 1 -- the tied one
    v, i = np.full(n, NEG, dtype=np.float32), np.full(n, -1, dtype=np.int32)
    v[[0, 1, 64, 65]] = (1.0, 0.75, 0.875, 0.75)
    i[[0, 1, 64]] = (40, 7, 9)
    v[8:12], i[8:12] = (0.9375, 0.75, 0.75, 0.75), (3, 5, 6, 8)
    add("id-minus-one-tie", v, i, (None, 64, 8), 1.0, 50, 1.0, want=lambda u: u > 0.9, token=8)
    return out


# EXACT: rows whose arithmetic is exact in fp32 and in float64 alike -- four valid candidates of one value (every
# term exp(0) = 1, Z = 4, inv_t = 2), top_p a multiple of 1/4, so cum_before_i / Z == top_p holds exactly where it
# holds at all and u * Zk is a 24-bit number times a power of two. The one place where "< top_p" and "<= top_p"
# differ.
def exact_table(per=16):
    n = 128
    v, i = np.full(n, NEG, dtype=np.float32), np.full(n, -1, dtype=np.int32)
    v[[0, 24, 25, 96]] = 2.5
    i[[0, 24, 25, 96]] = (300, 20, 21, 100000)
    i[[1, 2, 26]] = (301, 302, 22)  # banned tokens behind them
    combos = [(p, k) for p in (0.25, 0.5, 0.75) for k in (50, 0)]
    B = per * len(combos)
    return dict(cv=np.tile(v, (B, 1)), ci=np.tile(i, (B, 1)), list_lens=(None, 64, 8),
                T=np.full(B, 0.5, dtype=np.float32),
                top_k=np.array([combos[b % len(combos)][1] for b in range(B)], dtype=np.int32),
                top_p=np.array([combos[b % len(combos)][0] for b in range(B)], dtype=np.float32),
                seed=np.arange(B, dtype=np.int64) * 7919 - 50, step=np.arange(B, dtype=np.int32) * 3)


# ----------------------------------------------------------------------------- TOPK
CONTENTS = ("random", "all-equal", "run-at-kth", "run-at-max", "mostly-neg-inf", "huge-and-denormal", "zeros",
            "quantised")


def topk_row(kind, rng, V, chunks, K):
    """One fp32 row of the TOPK table."""
    Vc = chunk_width(V, chunks)
    if kind == "random":
        return (rng.standard_normal(V) * 3).astype(np.float32)
    if kind == "all-equal":
        return np.full(V, 1.75, dtype=np.float32)
    if kind == "run-at-kth":
        # 2K equal values (1.0) over negatives, K // 2 larger values in every chunk: the K-th place of the chunks
        # that hold the run falls inside it. The run crosses the first chunk boundary (K entries each side); with
        # one chunk it crosses element 1024 (where the block's threads wrap around) and several multiples of 64.
        row = -rng.uniform(0.5, 1.0, V).astype(np.float32)
        edge = Vc if chunks > 1 and Vc < V else (1024 if V > 1024 + K else V // 2)
        lo, hi = max(0, edge - K), min(V, edge + K)
        run = np.zeros(V, dtype=bool)
        run[lo:hi] = True
        for c in range(chunks):
            free = np.nonzero(~run[c * Vc:(c + 1) * Vc])[0] + c * Vc
            big = rng.choice(free, min(K // 2, free.size), replace=False)
            row[big] = rng.uniform(2.0, 3.0, big.size).astype(np.float32)
        row[run] = 1.0
        return row
    if kind == "run-at-max":
        row = (rng.standard_normal(V) * 3).astype(np.float32)
        lo = max(0, 64 - K)
        row[lo:min(V, lo + 2 * K)] = np.float32(row.max() + 1.0)
        return row
    if kind == "mostly-neg-inf":  # more -inf than V - K: the K-th value is -inf
        row = np.full(V, NEG, dtype=np.float32)
        fin = rng.choice(V, min(V, max(1, K // 2)), replace=False)
        row[fin] = (rng.standard_normal(fin.size) * 3).astype(np.float32)
        return row
    if kind == "huge-and-denormal":
        pool = np.array([-3.0e38, -1.0e30, -1.0e-40, -1.4e-45, 1.4e-45, 1.0e-40, 2.0e-40, -2.5, 1.2e-38],
                        dtype=np.float32)
        return rng.choice(pool, V, p=[.2, .2, .1, .1, .1, .1, .1, .05, .05])
    if kind == "zeros":  # +0.0 and -0.0 around the K-th place: a few positives, many negatives
        row = -rng.uniform(0.5, 1.0, V).astype(np.float32)
        z = rng.choice(V, min(V, 3 * K + 8), replace=False)
        row[z] = np.where(rng.integers(0, 2, z.size) == 0, np.float32(0.0), np.float32(-0.0))
        pos = rng.choice(V, min(V, max(1, K // 3)), replace=False)
        row[pos] = rng.uniform(1.0, 2.0, pos.size).astype(np.float32)
        return row
    assert kind == "quantised"
    return (np.round(rng.standard_normal(V) * 6) / 2).astype(np.float32)


def topk_cases():
    """(name, dict(V, chunks, K, ld, vocab_offset, kernel)): every case is one launch over len(CONTENTS) rows, one
    row per content. Shapes select each kernel by the rules of ragk_topk_candidates; K = 65 and 256 at the wave
    kernel's shape must land on the LDS kernel."""
    out = []
    shapes = ((5000, 8, "wave"), (6200, 1, "lds"), (20000, 3, "lds"), (24600, 1, "generic"))
    k = 0
    for V, chunks, kern in shapes:
        for K in (1, 50, 64, 65, 256):
            want = "lds" if kern == "wave" and K > 64 else kern
            out.append(dict(V=V, chunks=chunks, K=K, ld=V + (13 if k % 2 else 0), vocab_offset=(0, 1000, 70000)[k % 3],
                            kernel=want))
            k += 1
    out += [dict(V=37, chunks=1, K=50, ld=64, vocab_offset=5, kernel="lds"),       # V < K
            dict(V=10, chunks=3, K=64, ld=10, vocab_offset=0, kernel="lds"),       # V < K, an empty chunk
            dict(V=200, chunks=9, K=64, ld=211, vocab_offset=300, kernel="wave"),  # chunks of 24 < K
            dict(V=100, chunks=9, K=50, ld=100, vocab_offset=0, kernel="wave"),    # two empty chunks
            dict(V=49300, chunks=2, K=256, ld=49301, vocab_offset=11, kernel="generic")]  # two chunks of 24656
    return [("V%d-c%d-K%d-%s" % (c["V"], c["chunks"], c["K"], c["kernel"]), c) for c in out]


def topk_rows(case):
    """x [len(CONTENTS), V] of a case (seeded by its shape)."""
    rng = np.random.default_rng(case["V"] * 1000 + case["chunks"] * 300 + case["K"])
    return np.stack([topk_row(kind, rng, case["V"], case["chunks"], case["K"]) for kind in CONTENTS])


# ----------------------------------------------------------------------------- end to end, one per kernel
# (V, chunks, K, largest top_k drawn): topk_candidates, then sample_candidates(list_len=K)
END_TO_END = (("wave-lanes", 5000, 9, 64, 64), ("lds-rank", 20000, 3, 64, 64), ("lds-tail", 6200, 1, 256, 256),
              ("generic-rank", 49300, 2, 50, 50), ("generic-tail", 24600, 1, 256, 256))


def end_to_end_table(V, chunks, K, kmax, B=24, seed=2):
    """(seed: one for which no row of any of the five tables is ambiguous; of the seeds 0..5 that is 2, 4)"""
    rng = np.random.default_rng(V + chunks + K + seed)
    x = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    x[:, 5] = x[:, 9]  # an exact tie across ids
    lo = 65 if kmax > 64 else 1
    return x, draw_params(rng, B, rng.integers(lo, kmax + 1, B))
