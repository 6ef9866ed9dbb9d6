"""Inputs, float64 oracles and case lists shared by tests/test_exact_gpu.py, tests/test_attn_probe_gpu.py and
tests/test_exact_cpu.py. A plain module: importing it needs no GPU and no kernel library.

GEMM family: integer operands, so every product and every partial sum is an integer below 2^24 and the fp32
accumulator is exact in ANY summation order (split-K, cross-wave reductions, MFMA lane order). The expected
output is therefore one float64 product, rounded once where the kernel documents a rounding.

Attention: column-coded V (one-hot at column j % D), so out[i, h, c] is the softmax mass of the visible keys
j = c (mod D): every key owns a share of exactly one output column and a dropped, doubled or early key moves
that column by the key's share."""
import itertools
import math

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ACC_LIMIT = 2 ** 24


# ----------------------------------------------------------------------------------------------- GEMM inputs
def ints(shape, lo, hi, seed):
    """Uniform integers in [lo, hi] as float64 (CPU)."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def gemm_inputs(M, N, K, amp=8, rows=None, seed=None):
    """x [M, K], w [rows or N, K] in [-amp, amp]; bias [N] in [-8, 8]; resid [M, N] in [-64, 64]. float64."""
    seed = (M * 1000003 + N * 1009 + K) if seed is None else seed
    rows = N if rows is None else rows
    return (ints((M, K), -amp, amp, seed), ints((rows, K), -amp, amp, seed + 1), ints((N,), -8, 8, seed + 2),
            ints((M, N), -64, 64, seed + 3))


def acc64(x, w):
    return x.double() @ w.double().t()


def expected(acc, bias, resid, epi, out_f32=False):
    """The documented result of the linear epilogues: fp32 acc (+ bias) (+ resid), ONE round-to-nearest-even
    to bf16 (ops/reference.linear; common.h EPI_RESID: C = resid + acc)."""
    y = acc.double()
    if "bias" in epi:
        y = y + bias.double()
    if "resid" in epi:
        y = y + resid.double()
    assert float(y.abs().max()) < ACC_LIMIT
    y = y.float()  # exact: integers below 2^24
    return y if out_f32 else y.bfloat16()


LINEAR_EPIS = ("none", "bias", "resid", "bias_resid")
ACT_EPIS = ("bias_gelu", "gelu", "bias_gelu_tanh")


def act_expected(pre, epi):
    """float64 activation of the exact pre-activation."""
    pre = pre.double()
    if epi == "bias_gelu_tanh":
        return 0.5 * pre * (1 + torch.tanh(math.sqrt(2 / math.pi) * (pre + 0.044715 * pre ** 3)))
    return 0.5 * pre * (1 + torch.erf(pre / math.sqrt(2)))


def act_tolerance(ref, pre):
    """|y - ref| <= 2^-7 |ref| (one bf16 ulp) + 2^-20 max(1, |pre|) (16 fp32 eps of the argument: the
    cancellation in 0.5 x (1 + erf))."""
    return 2.0 ** -7 * ref.abs() + 2.0 ** -20 * pre.abs().clamp_min(1.0)


def silu_expected(gate, up):
    gate, up = gate.double(), up.double()
    return gate * torch.sigmoid(gate) * up


def silu_tolerance(ref, gate, up):
    """The activation bound of act_tolerance for silu(gate), carried through the exact product with up."""
    return 2.0 ** -7 * ref.abs() + 2.0 ** -20 * gate.abs().clamp_min(1.0) * up.abs().clamp_min(1.0)


def pack_gate_up(gate, up):
    """[I, K] gate / up -> the kernels' packed rows: 128-row tiles of [64 gate | 64 up] (ops/reference)."""
    I, K = gate.shape
    return torch.stack([gate.reshape(I // 64, 64, K), up.reshape(I // 64, 64, K)], 1).reshape(2 * I, K).contiguous()


def silu_inputs(M, N, K, seed=None):
    """x, gate, up in {-1, 0, 1}; gate tile 0 and (with >= 2 tiles) up tile 1 all zero: the paired output
    columns must be exact zeros."""
    seed = (M * 7919 + N * 31 + K) if seed is None else seed
    x, gate, up = ints((M, K), -1, 1, seed), ints((N, K), -1, 1, seed + 1), ints((N, K), -1, 1, seed + 2)
    gate[:64] = 0
    if N >= 128:
        up[64:128] = 0
    return x, gate, up


# strided operands: every view 16-byte aligned (offsets and pitches multiples of 8 bf16 / 4 fp32 / 16 fp8)
SENT = -7.0


def strided(t, off, tail, dtype, device="cpu", fill=SENT):
    """(buffer [rows, off + cols + tail] filled with `fill`, view [:, off:off + cols] holding t)."""
    rows, cols = t.shape
    buf = torch.full((rows, off + cols + tail), fill, dtype=F32).to(dtype).to(device)
    view = buf[:, off:off + cols]
    view.copy_(t.float().to(dtype))
    return buf, view


def gaps_intact(buf, off, cols, fill=SENT):
    """Every column of every row outside [off, off + cols) still holds the sentinel."""
    b = buf.float().cpu()
    return bool(b[:, :off].eq(fill).all()) and bool(b[:, off + cols:].eq(fill).all())


def aligned16(t):
    es = t.element_size()
    return (t.storage_offset() * es) % 16 == 0 and (t.dim() < 2 or (t.stride(0) * es) % 16 == 0) and t.stride(-1) == 1


# ----------------------------------------------------------------------------------------------- GEMM matrix
def _grid(Ms, Ns, Ks):
    return list(itertools.product(Ms, Ns, Ks))


TILE = _grid((65, 129, 200), (8, 136, 264), (128, 384))
SKINNY = _grid((1, 5, 16, 17, 33, 64), (40, 1000), (128, 1024))
PP = _grid((1, 255, 257, 513), (8, 264, 520), (256, 384, 640))
W4_PERSISTENT = (513, 520, 640)
SPLITK = _grid((300, 513), (264,), (512, 1024))
DEC = _grid((1, 17, 64), (40, 136, 1000), (256, 1024, 4096))
STREAM = _grid((1, 17, 64), (768, 1000), (1024, 4096))
PART = _grid((1, 7, 17, 33, 64), (1000, 4096), (512, 1792, 4096))
PART_KS = {4, 8, 14, 16, 28, 32}


def part_legal_ks(M, K):
    """The K-slice widths (in 64-column steps) gemm_part is built for at this shape: its launcher's own rule
    (the slice divides K; the activation slice fits 128 KiB of LDS in whole 8 KiB DMA rounds)."""
    mt = -(-M // 16)
    return [ks for ks in sorted(PART_KS)
            if K % (64 * ks) == 0 and 16 * mt * ks * 128 <= 128 * 1024 and (16 * mt * ks * 128) % 8192 == 0]


STREAM_PART = _grid((5, 16, 17, 64), (1000, 4096), (1024, 1792))
SLABS = (1, 7, 9, 16)
FP8_DEC = _grid((1, 5, 16, 17, 33, 64), (40, 1000), (128, 1024))
FP8_STREAM = (17, 16384, 1024)
FP8_PART = _grid((1, 7, 33, 64), (1000,), (512, 1792, 4096))
FP8_PREFILL = _grid((65, 129), (128, 136), (128, 384, 640, 1152))
# activation epilogues: (route, M, N, K), K <= 384, inputs in {-1, 0, 1}
ACT = [("tile", 129, 136, 384), ("skinny", 17, 40, 384), ("pp", 257, 264, 384), ("w4", 257, 264, 384),
       ("dec", 17, 136, 256), ("stream", 17, 768, 384)]
SILU = [("tile", 129, 192, 384), ("skinny", 17, 128, 384), ("skinny1", 17, 128, 384), ("pp", 257, 256, 384),
        ("w4", 257, 256, 384), ("dec", 17, 128, 256), ("stream", 17, 768, 384)]
# one strided case per kernel (ragged M, ragged N, more than one K step)
STRIDED = {"tile": (129, 136, 384), "skinny": (17, 40, 1024), "skinny1": (17, 40, 1024), "pp": (257, 264, 384),
           "w4": (257, 264, 384), "dec": (17, 136, 1024), "stream": (17, 1000, 1024)}
ALL_GEMM_SHAPES = (TILE + SKINNY + PP + [W4_PERSISTENT] + SPLITK + DEC + STREAM + PART + STREAM_PART + FP8_DEC
                   + [FP8_STREAM] + FP8_PART + FP8_PREFILL + [(4096, 4096, 14336)])


def pow2_scales(n, seed, lo=-2, hi=2):
    g = torch.Generator().manual_seed(int(seed))
    return torch.ldexp(torch.ones(n), torch.randint(lo, hi + 1, (n,), generator=g))


def slab_ints(S, M, H, seed, amp=3000):
    """Integer fp32 slabs: the slab sum is exact in any order and mostly not bf16-representable."""
    return ints((S, M, H), -amp, amp, seed).float()


# ----------------------------------------------------------------------------------------------- attention
PROBE_TOL = 2.0 ** -6  # twice the worst case of a bf16-rounded P (2^-8) plus the bf16-rounded output (2^-8)
MIN_SHARE = 4 * PROBE_TOL
BS = 64  # tokens per cache block
BIG = 2.0 ** 60

PREFILL_LENS = [([37], [37]), ([1], [1]), ([64, 65], [64, 200]), ([5, 70], [513, 70]),
                ([100, 64, 1], [100, 300, 129])]
PREFILL_HEADS_V3 = [(8, 2), (32, 8), (4, 1)]  # 4 query heads per KV head: the pipelined 8-wave kernel
PREFILL_HEADS_GENERIC = [(2, 1), (4, 4)]
ENCODER = [(32, 12), (64, 16)]
ENCODER_LENS = [7, 130, 64]
DECODE_LENS = [1, 63, 64, 65, 300, 513]
# split-K decode, (Hq, Hkv, D): every (D, heads per KV head) the launcher instantiates -- (128, 4), (128, 8),
# (128, 1), (128, 2), (64, 1) (the GPT-2 route) and (64, 4); the fp8 cache takes the D = 128 ones
DECODE_SPLIT = [(8, 2, 128), (4, 1, 128), (8, 1, 128), (2, 2, 128), (4, 2, 128), (4, 4, 64), (4, 1, 64)]
DECODE_HEADS_SINGLE = [(8, 2), (4, 1)]  # the single-partition grid is built for 4 query heads per KV head, D = 128
PREFILL_D64 = [(4, 4), (4, 1)]  # D = 64 paged prefill: 1 and 4 query heads per block


PROBE_SCALES = (0.5, 0.35, 0.25, 0.18)  # of q and K: scores have a standard deviation of scale^2


def probe_inputs(q_lens, kv_lens, Hq, Hkv, D, seed=0, scale=PROBE_SCALES[0]):
    """q [T, Hq*D] bf16; per sequence K [L, Hkv, D] bf16 (scale * randn) and V [L, Hkv, D] one-hot at j % D."""
    g = torch.Generator().manual_seed(1000 + seed)
    q = (scale * torch.randn(sum(q_lens), Hq * D, generator=g)).bfloat16()
    Ks, Vs = [], []
    for L in kv_lens:
        Ks.append((scale * torch.randn(L, Hkv, D, generator=g)).bfloat16())
        v = torch.zeros(L, Hkv, D)
        v[torch.arange(L), :, torch.arange(L) % D] = 1.0
        Vs.append(v.bfloat16())
    return q, Ks, Vs


def probe_oracle(q, Ks, q_lens, kv_lens, Hq, D, causal=True, mult=None):
    """float64 softmax with the causal and kv_len masks -> (ref [T, Hq, D], smallest share any visible key
    holds of its column). Queries are the last q_len positions of each context.
    mult (tests of the check itself): vis [ql, L] bool -> how many times each key counts for each query, to
    model a kernel that drops a key (0), counts it twice (2) or shows it early."""
    T = sum(q_lens)
    ref = torch.zeros(T, Hq, D, dtype=F64)
    min_share, t0 = 1.0, 0
    for ql, L, K in zip(q_lens, kv_lens, Ks):
        rep = Hq // K.shape[1]
        kk = K.double().repeat_interleave(rep, dim=1).transpose(0, 1)  # [Hq, L, D]
        qq = q[t0:t0 + ql].double().reshape(ql, Hq, D).transpose(0, 1)  # [Hq, ql, D]
        att = (qq @ kk.transpose(1, 2)) / math.sqrt(D)
        vis = torch.ones(ql, L, dtype=torch.bool)
        if causal:
            vis = torch.arange(L)[None, :] <= torch.arange(L - ql, L)[:, None]
        p = att.masked_fill(~vis, float("-inf")).softmax(-1)  # [Hq, ql, L]
        if mult is not None:
            e = torch.exp(att - att.max()) * mult(vis).double()
            p = e / e.sum(-1, keepdim=True)
            vis = vis & (mult(vis) > 0)
        nch = -(-L // D)
        pp = torch.zeros(Hq, ql, nch * D, dtype=F64)
        pp[..., :L] = p
        col = pp.reshape(Hq, ql, nch, D).sum(2)  # [Hq, ql, D]
        ref[t0:t0 + ql] = col.transpose(0, 1)
        share = p / col[..., torch.arange(L) % D]
        min_share = min(min_share, float(share[vis.expand_as(share)].min()))
        t0 += ql
    return ref, min_share


def probe_case(q_lens, kv_lens, Hq, Hkv, D, causal=True, seed=0):
    """(q, Ks, Vs, ref, min share) at the largest input scale of PROBE_SCALES whose oracle gives every visible
    key MIN_SHARE of its column (where five keys share a column the 0.5 scale can fall just short); chosen from
    the oracle alone, and the tests assert the condition."""
    for scale in PROBE_SCALES:
        q, Ks, Vs = probe_inputs(q_lens, kv_lens, Hq, Hkv, D, seed, scale)
        ref, share = probe_oracle(q, Ks, q_lens, kv_lens, Hq, D, causal)
        if share >= MIN_SHARE:
            break
    return q, Ks, Vs, ref, share


def probe_check(out, ref):
    """Every element finite and within PROBE_TOL of the oracle, exact zeros where no visible key maps to the
    column. Written so that a NaN (an unwritten element of a NaN-prefilled output, 0 * Inf, exp(-inf + inf))
    fails: NaN compares False with everything."""
    out = out.double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(out).all()), "%d non-finite output elements, first at %s" % (
        int((~torch.isfinite(out)).sum()), (~torch.isfinite(out)).nonzero()[0].tolist())
    zero = ref == 0
    assert bool((out[zero] == 0).all()), "mass in a column no visible key maps to"
    err = (out - ref).abs()
    ok = err <= PROBE_TOL * ref.abs()
    assert bool(ok.all()), "worst |out - ref| / ref = %.4f at %s" % (
        float((err / ref.abs().clamp_min(1e-300))[~zero].max()), (~ok).nonzero()[0].tolist())


def paged_layout(kv_lens, seed=0, extra=3):
    """(block tables [B, maxb + 1] int32, hidden [total, BS] bool, total): permuted live blocks; every entry past
    ceil(kv_len / BS) points at one decoy block (in range, in no sequence's live part); `hidden` marks the slots
    no query may look at: rows past kv_len in a last block, the decoy and the other unused blocks."""
    g = torch.Generator().manual_seed(77 + seed)
    nb_per = [-(-L // BS) for L in kv_lens]
    total = sum(nb_per) + extra
    perm = torch.randperm(total, generator=g)
    decoy = int(perm[sum(nb_per)])
    bt = torch.full((len(kv_lens), max(nb_per) + 1), decoy, dtype=torch.int32)
    hidden = torch.ones(total, BS, dtype=torch.bool)
    i = 0
    for s, (L, nb) in enumerate(zip(kv_lens, nb_per)):
        blocks = perm[i:i + nb]
        i += nb
        bt[s, :nb] = blocks.int()
        for b, blk in enumerate(blocks.tolist()):
            hidden[blk, :max(0, min(BS, L - b * BS))] = False
    return bt, hidden, total


def paged_fill(rows_per_seq, kv_lens, bt, total, Hkv, D, hidden, stale, seed=0, dtype=BF16):
    """Cache [total, Hkv, BS, D]: the live rows from rows_per_seq ([L, Hkv, D] each), every hidden slot zeros
    (stale False) or +-2^60 (stale True)."""
    g = torch.Generator().manual_seed(99 + seed)
    c = torch.zeros(total, Hkv, BS, D)
    if stale:
        c = torch.where(torch.rand(c.shape, generator=g) < 0.5, -BIG, BIG) * torch.ones_like(c)
    for s, (L, rows) in enumerate(zip(kv_lens, rows_per_seq)):
        for b in range(-(-L // BS)):
            n = min(BS, L - b * BS)
            c[int(bt[s, b]), :, :n] = rows[b * BS:b * BS + n].float().transpose(0, 1)
    live = ~hidden[:, None, :, None].expand_as(c)
    assert stale or bool((c[~live] == 0).all())
    return c.to(dtype)


def hidden_scale_bits(shape, seed=0):
    """Arbitrary fp32 words for hidden fp8 scale slots: random bits with NaN, +-Inf, 0 and denormals mixed in."""
    g = torch.Generator().manual_seed(55 + seed)
    w = torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, dtype=torch.int64).to(torch.int32)
    special = torch.tensor([0x7FC00000, 0x7F800000, -8388608, 0, 1, 0x7FFFFFFF], dtype=torch.int64).to(torch.int32)
    pick = torch.randint(0, 12, shape, generator=g)
    return torch.where(pick < 6, special[pick.clamp_max(5)], w).view(F32)


def hidden_fp8_codes(shape, seed=0):
    """Random finite e4m3fn codes (no 0x7F / 0xFF)."""
    g = torch.Generator().manual_seed(66 + seed)
    c = torch.randint(0, 256, shape, generator=g, dtype=torch.int64)
    return torch.where(c % 128 == 127, c - 1, c).to(torch.uint8)
