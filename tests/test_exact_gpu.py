"""Exact-integer tests of the bf16 / fp8 GEMM family: every output element pinned, not a norm.

Operands are small integers (tests/exact_cases.py), so the fp32 accumulator is exact in any summation order and
the result must be torch.equal to one float64 product: fp32 outputs as they are, bf16 outputs after ONE
round-to-nearest-even of acc (+ bias) (+ resid), the rounding point ops/reference.linear and common.h document.
add_partials_rmsnorm and rope_kv_partials document another one (bf16 of the slab sum first), mirrored here.
A wrong edge-tile guard, a lost K step, a slab summed twice or an extra bf16 rounding cannot pass.

The same cases run again with every operand a 16-byte-aligned view of a wider buffer (leading dimensions
different from the row length, sentinel columns between the rows), and misaligned views must be refused by the
Python entry points before anything is launched.

Not covered: ragk_gemm_path path 3 (gemm_gemv_kernel), which nothing in the package calls."""
import pytest
import torch

import exact_cases as X
from rag_llm_k8s_amd.ops import reference as R
from rag_llm_k8s_amd.ops.fp8 import FP8, Fp8Weight

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
PAD = 4096

ROUTES = {"tile": {}, "skinny": {}, "skinny1": {"path": 1}, "pp": {"path": 2}, "w4": {"path": 6}, "dec": {"path": 4},
          "stream": {"path": 5}}


def _d(t, dtype=BF16):
    return t.to(dtype).to(DEV)


def _same(y, exp, what):
    y = y.cpu()
    assert y.dtype == exp.dtype and y.shape == exp.shape, what
    if not torch.equal(y, exp):
        bad = (y.float() != exp.float()).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, expected %r" % (
            what, bad.shape[0], exp.numel(), i, float(y[i]), float(exp[i])))


def _check_linear(native, M, N, K, route, epis=X.LINEAR_EPIS, f32=True, repeat=1):
    x, w, b, r = X.gemm_inputs(M, N, K)
    acc = X.acc64(x, w)
    xd, wd, bd, rd = _d(x), _d(w), _d(b), _d(r)
    kw = ROUTES[route]
    for epi in epis:
        for _ in range(repeat):
            y = native.gemm(xd, wd, bias=bd, resid=rd, epi=epi, **kw)
            _same(y, X.expected(acc, b, r, epi), "%s %s" % (route, epi))
    if f32:
        for epi in ("none", "bias_resid"):
            y = native.gemm(xd, wd, bias=bd, resid=rd, epi=epi, out_f32=True, **kw)
            _same(y, X.expected(acc, b, r, epi, out_f32=True), "%s %s fp32" % (route, epi))


# ----------------------------------------------------------------------------------------------- 1. exact GEMMs
@pytest.mark.parametrize("M,N,K", X.TILE)
def test_tile_exact(native, M, N, K):
    _check_linear(native, M, N, K, "tile")


@pytest.mark.parametrize("M,N,K", X.SKINNY)
def test_skinny_exact(native, M, N, K):
    _check_linear(native, M, N, K, "skinny")
    _check_linear(native, M, N, K, "skinny1", epis=("none", "resid"), f32=False)  # what ragk_gemm_path takes


@pytest.mark.parametrize("route", ["pp", "w4"])
@pytest.mark.parametrize("M,N,K", X.PP)
def test_pp_w4_exact(native, M, N, K, route):
    _check_linear(native, M, N, K, route)


@pytest.mark.parametrize("grid", [-1, 0, 3])
def test_w4_persistent_exact(native, grid):
    """3 x 3 tiles: with 3 blocks every block loops over three tiles (full, ragged-N and ragged-M ones)."""
    native.set_w4_grid(grid)
    try:
        _check_linear(native, *X.W4_PERSISTENT, "w4")
    finally:
        native.set_w4_grid(-1)


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("M,N,K", X.SPLITK)
def test_splitk_exact(native, M, N, K, ns):
    x, w, _, _ = X.gemm_inputs(M, N, K)
    P = native.gemm_splitk(_d(x), _d(w), ns)
    assert P.shape == (ns, M, N)
    Ks = K // ns
    for z in range(ns):
        _same(P[z], X.acc64(x[:, z * Ks:(z + 1) * Ks], w[:, z * Ks:(z + 1) * Ks]).float(), "slab %d" % z)
    _same(P.sum(0), X.acc64(x, w).float(), "slab sum")


@pytest.mark.parametrize("M,N,K", X.DEC)
def test_dec_exact(native, M, N, K):
    """Every call twice: the second one runs on the split-K counters the first one left."""
    if (N, K) == (136, 4096):
        assert native._lib.lib().ragk_gemm_dec_splits(N, K, 0) == 16
    _check_linear(native, M, N, K, "dec", repeat=2)


@pytest.mark.parametrize("M,N,K", X.STREAM)
def test_stream_exact(native, M, N, K):
    _check_linear(native, M, N, K, "stream", repeat=2)


def test_stream_pinned_split_exact(native, monkeypatch):
    monkeypatch.setattr(native, "STREAM_S_OVERRIDE", 4)
    _check_linear(native, 17, 1000, 1024, "stream", repeat=2)


def _part_cases():
    return [(M, N, K, ks) for M, N, K in X.PART for ks in X.part_legal_ks(M, K)]


def test_part_cases_cover_every_slice_width():
    assert {ks for _, _, _, ks in _part_cases()} == X.PART_KS


@pytest.mark.parametrize("M,N,K", X.PART)
def test_part_exact(native, M, N, K, monkeypatch):
    """gemm_part with the slice width its picker chooses and with every other width the kernel is built for at
    this shape (the picker alone reaches only 4 and 8 steps on these small N): each slab against its own K
    range, and the slab sum."""
    monkeypatch.setattr(native, "STREAM_PART", False)
    x, w, _, _ = X.gemm_inputs(M, N, K)
    xd, wd = _d(x), _d(w)
    chosen, _ = native.gemm_part_slabs(M, N, K)
    assert chosen in X.part_legal_ks(M, K)
    for ks in [None] + X.part_legal_ks(M, K):
        P = native.gemm_part(xd, wd, ks=ks)
        KS = 64 * (ks or chosen)
        assert P.shape == (K // KS, M, N)
        for z in range(K // KS):
            _same(P[z], X.acc64(x[:, z * KS:(z + 1) * KS], w[:, z * KS:(z + 1) * KS]).float(), "ks %s slab %d" % (ks, z))
        _same(P.sum(0), X.acc64(x, w).float(), "ks %s slab sum" % ks)


@pytest.mark.parametrize("rows", [64, 128])
@pytest.mark.parametrize("M,N,K", X.STREAM_PART)
def test_stream_part_exact(native, M, N, K, rows):
    x, w, _, _ = X.gemm_inputs(M, N, K)
    S = 2  # 8 and 14 K-steps per block
    P = native.gemm_stream_part(_d(x), _d(w), rows=rows, S=S)
    assert P.shape == (S, M, N)
    Ks = K // S
    for z in range(S):
        _same(P[z], X.acc64(x[:, z * Ks:(z + 1) * Ks], w[:, z * Ks:(z + 1) * Ks]).float(), "slab %d" % z)
    _same(P.sum(0), X.acc64(x, w).float(), "slab sum")


def _h_expected(P, h):
    """add_partials_rmsnorm's documented update: h <- bf16(h + bf16(sum of the slabs)) (HF: the bf16 linear
    output, then the bf16 residual add) -- two roundings, not the GEMM epilogues' one."""
    return (h.double() + P.double().sum(0).float().bfloat16().double()).float().bfloat16()


@pytest.mark.parametrize("H", [1000, 4104])  # 125 vectors; 513: the second register set holds one
@pytest.mark.parametrize("S", X.SLABS)
def test_add_partials_rmsnorm_h_exact(native, S, H):
    M = 5
    P = X.slab_ints(S, M, H, seed=S + H)
    h = X.ints((M, H), -64, 64, S).bfloat16()
    g = torch.ones(H).bfloat16()
    hd = h.to(DEV)
    native.add_partials_rmsnorm(P.to(DEV), hd, g.to(DEV), 1e-5)
    _same(hd, _h_expected(P, h), "h")


@pytest.mark.parametrize("S", X.SLABS)
def test_rope_kv_partials_v_rows_exact(native, S):
    """v = bf16(sum of the slabs) goes to the cache unrotated: exact. Token 2 has no slot: nothing written."""
    T, Hq, Hkv, D = 5, 4, 2, 128
    W = (Hq + 2 * Hkv) * D
    P = X.slab_ints(S, T, W, seed=100 + S)
    slots = torch.tensor([64, 127, -1, 5, 130], dtype=torch.int32)
    kc = torch.full((4, Hkv, 64, D), X.SENT, device=DEV).bfloat16()
    vc = torch.full_like(kc, X.SENT)
    cos, sin = R.rope_tables(D, 64)
    flat, qbuf, q = _out_view(T, Hq * D, BF16)  # q_out strided: its row gaps and guards must survive
    native.rope_kv_partials(P.to(DEV), q, torch.arange(T, dtype=torch.int32, device=DEV), cos.to(DEV), sin.to(DEV),
                            slots.to(DEV), kc, vc, Hq, Hkv, D)
    torch.cuda.synchronize()
    assert X.gaps_intact(qbuf, 8, Hq * D) and _guards_intact(flat)
    # position 0 rotates by cos = 1, sin = 0: token 0's q row is the rounded slab sum
    _same(q[0], P.double().sum(0).float().bfloat16()[0, :Hq * D], "q row at position 0")
    want = torch.full((4, Hkv, 64, D), X.SENT).bfloat16()
    v = P.double().sum(0).float().bfloat16()[:, (Hq + Hkv) * D:].reshape(T, Hkv, D)
    for t, s in enumerate(slots.tolist()):
        if s >= 0:
            want[s // 64, :, s % 64] = v[t]
    _same(vc, want, "v cache")
    # position 0 rotates by cos = 1, sin = 0: token 0's k row is the rounded slab sum as well
    k0 = P.double().sum(0).float().bfloat16()[0, Hq * D:(Hq + Hkv) * D].reshape(Hkv, D)
    _same(kc[1, :, 0], k0, "k row at position 0")


# ----------------------------------------------------------------------------------------------- fp8 weights
def _fp8_weight(w, seed):
    """Integer e4m3 rows (exact up to 16) with power-of-two row scales -> (Fp8Weight on the GPU, dequantized float64)."""
    s = X.pow2_scales(w.shape[0], seed)
    return Fp8Weight(w.float().to(FP8).to(DEV), s.to(DEV)), w.double() * s.double()[:, None]


def _check_fp8(native, M, N, K, act=False):
    x, w, b, r = X.gemm_inputs(M, N, K)
    wq, wd = _fp8_weight(w, M + N + K)
    sa = X.pow2_scales(M, K + 1)
    kw = dict(act=(x.float().to(FP8).to(DEV), sa.to(DEV))) if act else {}
    xe = x.double() * sa.double()[:, None] if act else x
    acc = X.acc64(xe, wd)
    xd, bd, rd = (None if act else _d(x)), _d(b), _d(r)
    for epi in X.LINEAR_EPIS:
        y = native.gemm_fp8(xd, wq, bias=bd, resid=rd, epi=epi, **kw)
        _same(y, X.expected(acc, b, r, epi), "fp8 %s" % epi)
    y = native.gemm_fp8(xd, wq, out_f32=True, **kw)
    _same(y, X.expected(acc, b, r, "none", out_f32=True), "fp8 fp32")


@pytest.mark.parametrize("M,N,K", X.FP8_DEC + [X.FP8_STREAM])
def test_fp8_decode_exact(native, M, N, K):
    assert native.use_stream(M, N, K, "none", fp8=True) == ((M, N, K) == X.FP8_STREAM)
    _check_fp8(native, M, N, K)


@pytest.mark.parametrize("M,N,K", X.FP8_PREFILL)
def test_fp8_prefill_exact(native, M, N, K):
    """W8A8 with integer e4m3 activations and power-of-two row scales handed in through act=."""
    _check_fp8(native, M, N, K, act=True)


def test_fp8_act_runs_prefill_kernel_at_small_m(native):
    _check_fp8(native, 17, 136, 384, act=True)


@pytest.mark.parametrize("M,N,K", X.FP8_PART)
def test_fp8_part_exact(native, M, N, K):
    x, w, _, _ = X.gemm_inputs(M, N, K)
    wq, wd = _fp8_weight(w, M + K)
    for ks in [None] + X.part_legal_ks(M, K):  # all even, as ragk_gemm_part_fp8 requires
        P = native.gemm_part(_d(x), wq, ks=ks)
        _same(P.sum(0), X.acc64(x, wd).float(), "fp8 slab sum ks %s" % ks)


# ----------------------------------------------------------------------------------------------- activations
@pytest.mark.parametrize("route,M,N,K", X.ACT)
def test_activation_epilogues(native, route, M, N, K):
    x, w = X.ints((M, K), -1, 1, M + K), X.ints((N, K), -1, 1, N + K)
    b = X.ints((N,), -2, 2, N)
    acc = X.acc64(x, w)
    for epi in X.ACT_EPIS:
        pre = acc + b if "bias" in epi else acc
        ref = X.act_expected(pre, epi)
        y = native.gemm(_d(x), _d(w), bias=_d(b), epi=epi, **ROUTES[route]).cpu().double()
        over = (y - ref).abs() - X.act_tolerance(ref, pre)
        assert float(over.max()) <= 0, "%s %s: %d elements out of tolerance, worst by %.3e at pre = %r" % (
            route, epi, int((over > 0).sum()), float(over.max()), float(pre.flatten()[over.argmax()]))


@pytest.mark.parametrize("route,M,N,K", X.SILU)
def test_silu_mul_epilogue(native, route, M, N, K):
    x, gate, up = X.silu_inputs(M, N, K)
    g, u = X.acc64(x, gate), X.acc64(x, up)
    ref = X.silu_expected(g, u)
    y = native.gemm(_d(x), _d(X.pack_gate_up(gate, up)), epi="silu_mul", **ROUTES[route]).cpu().double()
    assert y.shape == (M, N)
    assert bool((y[:, :64] == 0).all()), "zero gate tile"
    assert bool((y[:, 64:128] == 0).all()), "zero up tile"
    over = (y - ref).abs() - X.silu_tolerance(ref, g, u)
    assert float(over.max()) <= 0, "%s: worst by %.3e" % (route, float(over.max()))


# ----------------------------------------------------------------------------------------------- 2. leading dimensions
def _guarded(rows, width, dtype):
    """(flat buffer with PAD sentinels before and after, its [rows, width] middle as a matrix)."""
    flat = torch.full((2 * PAD + rows * width,), X.SENT, dtype=dtype, device=DEV)
    return flat, flat[PAD:PAD + rows * width].view(rows, width)


def _guards_intact(flat):
    return bool(flat[:PAD].eq(X.SENT).all()) and bool(flat[-PAD:].eq(X.SENT).all())


def _out_view(M, N, dtype):
    flat, buf = _guarded(M, N + 16, dtype)
    return flat, buf, buf[:, 8:8 + N]


def _strided_inputs(x, w, r):
    _, xv = X.strided(x, 8, 16, BF16, DEV)  # [M, K + 24]
    _, wv = X.strided(w, 8, 0, BF16, DEV)  # [N, K + 8]
    rbuf, rv = X.strided(r, 16, 24, BF16, DEV)  # [M, N + 40]: a third leading dimension
    for v in (xv, wv, rv):
        assert X.aligned16(v) and not v.is_contiguous()
    return xv, wv, rbuf, rv


@pytest.mark.parametrize("route", sorted(X.STRIDED))
def test_gemm_leading_dimensions(native, route):
    M, N, K = X.STRIDED[route]
    x, w, b, r = X.gemm_inputs(M, N, K)
    acc = X.acc64(x, w)
    xv, wv, rbuf, rv = _strided_inputs(x, w, r)
    # ragk_gemm_path (the forced skinny kernel) takes the none / resid epilogues with bf16 outputs only
    runs = [("resid", False), ("none", False)] if route == "skinny1" else [("bias_resid", False), ("none", True)]
    for epi, f32 in runs:
        flat, buf, out = _out_view(M, N, F32 if f32 else BF16)
        native.gemm(xv, wv, bias=_d(b), resid=rv, epi=epi, out=out, out_f32=f32, **ROUTES[route])
        torch.cuda.synchronize()
        _same(out, X.expected(acc, b, r, epi, out_f32=f32), "%s %s strided" % (route, epi))
        assert X.gaps_intact(buf, 8, N) and _guards_intact(flat), "sentinel columns of out"
        assert X.gaps_intact(rbuf, 16, N), "sentinel columns of resid"
    h = rv  # in place: resid aliases out, both strided
    native.gemm(xv, wv, resid=h, epi="resid", out=h, **ROUTES[route])
    _same(h, X.expected(acc, b, r, "resid"), "%s in-place resid" % route)
    assert X.gaps_intact(rbuf, 16, N)


def test_slab_kernels_leading_dimensions(native, monkeypatch):
    """The slab outputs are contiguous by contract: only x and w are strided."""
    monkeypatch.setattr(native, "STREAM_PART", False)
    for name, (M, N, K), run in [
            ("splitk", (300, 264, 512), lambda a, b: native.gemm_splitk(a, b, 2)),
            ("part", (17, 1000, 1792), lambda a, b: native.gemm_part(a, b)),
            ("stream_part", (17, 1000, 1792), lambda a, b: native.gemm_stream_part(a, b, rows=64, S=2))]:
        x, w, _, r = X.gemm_inputs(M, N, K)
        xv, wv, _, _ = _strided_inputs(x, w, r)
        _same(run(xv, wv).sum(0), X.acc64(x, w).float(), name)


def test_fp8_leading_dimensions(native):
    M, N, K = 17, 40, 1024
    x, w, b, r = X.gemm_inputs(M, N, K)
    wq, wd = _fp8_weight(w, 3)
    xv, _, rbuf, rv = _strided_inputs(x, w, r)
    flat, buf, out = _out_view(M, N, BF16)
    native.gemm_fp8(xv, wq, bias=_d(b), resid=rv, epi="bias_resid", out=out)
    torch.cuda.synchronize()
    _same(out, X.expected(X.acc64(x, wd), b, r, "bias_resid"), "fp8 decode strided")
    assert X.gaps_intact(buf, 8, N) and _guards_intact(flat) and X.gaps_intact(rbuf, 16, N)
    # gemm_part takes the weight's leading dimension (bytes)
    M, N, K = 17, 1000, 1792
    x, w, _, _ = X.gemm_inputs(M, N, K)
    s = X.pow2_scales(N, 5)
    _, w8 = X.strided(w, 16, 16, FP8, DEV, fill=0.0)
    assert X.aligned16(w8)
    _, xv = X.strided(x, 8, 16, BF16, DEV)
    P = native.gemm_part(xv, Fp8Weight(w8, s.to(DEV)))
    _same(P.sum(0), X.acc64(x, w.double() * s.double()[:, None]).float(), "fp8 part strided")
    # W8A8 prefill: strided quantized activations, strided resid and out
    M, N, K = 129, 136, 384
    x, w, b, r = X.gemm_inputs(M, N, K)
    wq, wd = _fp8_weight(w, 7)
    sa = X.pow2_scales(M, 9)
    _, qv = X.strided(x, 16, 16, FP8, DEV, fill=0.0)
    _, _, rbuf, rv = _strided_inputs(x, w, r)
    flat, buf, out = _out_view(M, N, BF16)
    native.gemm_fp8(None, wq, bias=_d(b), resid=rv, epi="bias_resid", out=out, act=(qv, sa.to(DEV)))
    torch.cuda.synchronize()
    _same(out, X.expected(X.acc64(x.double() * sa.double()[:, None], wd), b, r, "bias_resid"), "fp8 prefill strided")
    assert X.gaps_intact(buf, 8, N) and _guards_intact(flat) and X.gaps_intact(rbuf, 16, N)


@pytest.mark.parametrize("T,H", [(5, 384), (37, 4096)])
def test_rmsnorm_leading_dimensions(native, T, H):
    """x, resid and out strided, at the tolerance of test_kernels_gpu.test_rmsnorm; the in-place residual update
    is exact."""
    g = torch.Generator().manual_seed(T)
    x, r = torch.randn(T, H, generator=g).bfloat16(), torch.randn(T, H, generator=g).bfloat16()
    w = torch.randn(H, generator=g).bfloat16()
    _, xv = X.strided(x, 8, 16, BF16, DEV)
    rbuf, rv = X.strided(r, 16, 24, BF16, DEV)
    flat, buf, out = _out_view(T, H, BF16)
    native.rmsnorm(xv, w.to(DEV), 1e-5, out=out, resid=rv)
    torch.cuda.synchronize()
    r_ref = r.clone()
    ref = R.rmsnorm(x, w, 1e-5, resid=r_ref)
    _same(rv, r_ref, "residual stream")
    y = out.cpu().float()
    assert (y - ref.float()).abs().max().item() <= 0.0625
    assert ((y - ref.float()).norm() / ref.float().norm()).item() < 4e-3
    assert X.gaps_intact(buf, 8, H) and _guards_intact(flat) and X.gaps_intact(rbuf, 16, H)


def test_add_partials_rmsnorm_leading_dimensions(native):
    S, M, H = 7, 5, 1000
    P = X.slab_ints(S, M, H, seed=1)
    h = X.ints((M, H), -64, 64, 2).bfloat16()
    hbuf, hv = X.strided(h, 16, 24, BF16, DEV)
    flat, buf, out = _out_view(M, H, BF16)
    native.add_partials_rmsnorm(P.to(DEV), hv, torch.ones(H, device=DEV).bfloat16(), 1e-5, out=out)
    torch.cuda.synchronize()
    want = _h_expected(P, h)
    _same(hv, want, "h")
    ref = R.rmsnorm(want, torch.ones(H).bfloat16(), 1e-5)
    assert ((out.cpu().float() - ref.float()).norm() / ref.float().norm()).item() < 4e-3
    assert X.gaps_intact(hbuf, 16, H) and X.gaps_intact(buf, 8, H) and _guards_intact(flat)


# ----------------------------------------------------------------------------------------------- 3. alignment
class _NoLaunch:
    """Stands in for the kernel library while misaligned operands are offered: host-side queries pass through,
    anything that could launch fails the test instead of running."""
    HOST = {"ragk_gemm_part_ksteps", "ragk_gemm_stream_splits", "ragk_gemm_dec_splits"}

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name in self.HOST:
            return getattr(self._real, name)
        raise AssertionError("a misaligned operand got as far as %s" % name)


@pytest.fixture
def no_launch(native, monkeypatch):
    proxy = _NoLaunch(native._lib.lib())
    monkeypatch.setattr(native._lib, "lib", lambda: proxy)
    return native


def _refused(fn):
    with pytest.raises(ValueError, match="aligned|pitch"):
        fn()


def _odd(rows, cols, dtype=BF16):
    """A view whose base pointer is off by one element."""
    v = torch.zeros(rows, cols + 8, dtype=dtype, device=DEV)[:, 1:1 + cols]
    assert v.data_ptr() % 16 != 0
    return v


def _odd_pitch(rows, cols, dtype=BF16):
    """An aligned base with a row pitch that is 8 bytes past a multiple of 16 (cols * element size is one)."""
    extra = 8 // torch.empty(0, dtype=dtype).element_size()
    v = torch.zeros(rows, cols + extra, dtype=dtype, device=DEV)[:, :cols]
    assert (v.stride(0) * v.element_size()) % 16 == 8 and v.data_ptr() % 16 == 0
    return v


def _z(rows, cols, dtype=BF16):
    return torch.zeros(rows, cols, dtype=dtype, device=DEV)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_gemm_refuses_misaligned_operands(no_launch, route):
    n = no_launch
    M, N, K = X.STRIDED[route]
    kw = ROUTES[route]
    for bad in (_odd, _odd_pitch):
        _refused(lambda: n.gemm(bad(M, K), _z(N, K), **kw))
        _refused(lambda: n.gemm(_z(M, K), bad(N, K), **kw))
    if route in ("tile", "pp", "w4"):  # vector epilogues: out, bias and resid too
        bias = torch.zeros(N + 8, dtype=BF16, device=DEV)
        for bad in (_odd, _odd_pitch):
            _refused(lambda: n.gemm(_z(M, K), _z(N, K), out=bad(M, N), **kw))
            _refused(lambda: n.gemm(_z(M, K), _z(N, K), out=bad(M, N, F32), out_f32=True, **kw))
            _refused(lambda: n.gemm(_z(M, K), _z(N, K), resid=bad(M, N), epi="resid", **kw))
        _refused(lambda: n.gemm(_z(M, K), _z(N, K), bias=bias[1:1 + N], epi="bias", **kw))
    if route == "tile":  # the forced tile path stores vectors at any M; a path the library does not know is refused
        _refused(lambda: n.gemm(_z(17, K), _z(N, K), out=_odd(17, N), path=0))
        with pytest.raises(ValueError, match="unknown GEMM path"):
            n.gemm(_z(M, K), _z(N, K), out=_odd(M, N), path=7)


def test_slab_gemms_refuse_misaligned_operands(no_launch, monkeypatch):
    n = no_launch
    for stream_part in (False, True):
        monkeypatch.setattr(n, "STREAM_PART", stream_part)
        for bad in (_odd, _odd_pitch):
            _refused(lambda: n.gemm_part(bad(17, 1792), _z(1000, 1792)))
            _refused(lambda: n.gemm_part(_z(17, 1792), bad(1000, 1792)))
    for bad in (_odd, _odd_pitch):
        _refused(lambda: n.gemm_stream_part(bad(17, 1792), _z(1000, 1792), rows=64, S=2))
        _refused(lambda: n.gemm_stream_part(_z(17, 1792), bad(1000, 1792), rows=64, S=2))
        _refused(lambda: n.gemm_splitk(bad(300, 512), _z(264, 512), 2))
        _refused(lambda: n.gemm_splitk(_z(300, 512), bad(264, 512), 2))
        _refused(lambda: n.gemm_part(_z(17, 1792), Fp8Weight(bad(1000, 1792, FP8), torch.ones(1000, device=DEV))))
        _refused(lambda: n.gemm_part_norm(bad(2, 4096), torch.ones(4096, device=DEV).bfloat16(), 1e-5, _z(1280, 4096)))
    slab = torch.zeros(2 * 17 * 1000 + 4, device=DEV)[1:1 + 2 * 17 * 1000]
    _refused(lambda: n.gemm_stream_part(_z(17, 1792), _z(1000, 1792), out=slab, rows=64, S=2))


def test_fp8_gemm_refuses_misaligned_operands(no_launch):
    n = no_launch
    wq = Fp8Weight(_z(136, 384, FP8), torch.ones(136, device=DEV))
    sa = torch.ones(129, device=DEV)
    for bad in (_odd, _odd_pitch):
        _refused(lambda: n.gemm_fp8(bad(17, 384), wq))  # decode
        _refused(lambda: n.quant_fp8_rows(bad(129, 384)))  # called directly
        _refused(lambda: n.gemm_fp8(bad(129, 384), wq))  # prefill: quant_rows reads x
        _refused(lambda: n.gemm_fp8(None, wq, act=(bad(129, 384, FP8), sa)))
        _refused(lambda: n.gemm_fp8(_z(129, 384), wq, out=bad(129, 136)))
        _refused(lambda: n.gemm_fp8(_z(129, 384), wq, resid=bad(129, 136), epi="resid"))
    odd_w = torch.zeros(136 * 384 + 16, dtype=torch.uint8, device=DEV)[1:1 + 136 * 384].view(FP8).view(136, 384)
    _refused(lambda: n.gemm_fp8(_z(17, 384), Fp8Weight(odd_w, torch.ones(136, device=DEV))))


def test_norms_refuse_misaligned_operands(no_launch):
    n = no_launch
    T, H = 5, 384
    w = torch.ones(H + 8, device=DEV).bfloat16()
    for bad in (_odd, _odd_pitch):
        _refused(lambda: n.rmsnorm(bad(T, H), w[:H], 1e-5))
        _refused(lambda: n.rmsnorm(_z(T, H), w[:H], 1e-5, out=bad(T, H)))
        _refused(lambda: n.rmsnorm(_z(T, H), w[:H], 1e-5, resid=bad(T, H)))
        _refused(lambda: n.add_partials_rmsnorm(torch.zeros(2, T, H, device=DEV), bad(T, H), w[:H], 1e-5))
        _refused(lambda: n.add_partials_rmsnorm(torch.zeros(2, T, H, device=DEV), _z(T, H), w[:H], 1e-5, out=bad(T, H)))
    _refused(lambda: n.rmsnorm(_z(T, H), w[1:1 + H], 1e-5))
    _refused(lambda: n.add_partials_rmsnorm(torch.zeros(2, T, H, device=DEV), _z(T, H), w[1:1 + H], 1e-5))
    Hq, Hkv, D = 4, 2, 128
    P = torch.zeros(2, T, (Hq + 2 * Hkv) * D, device=DEV)
    kc = torch.zeros(2, Hkv, 64, D, device=DEV).bfloat16()
    i32 = torch.zeros(T, dtype=torch.int32, device=DEV)
    cs = torch.zeros(8, D // 2, device=DEV)
    for bad in (_odd, _odd_pitch):
        _refused(lambda: n.rope_kv_partials(P, bad(T, Hq * D), i32, cs, cs, i32, kc, kc.clone(), Hq, Hkv, D))
