"""gemm_w4 with an M-tile list (gemm(..., m_tiles=) / gemm_splitk(..., m_tiles=)): the rows of listed 256-row
tiles are bit-identical to the same call without a list, the rows of unlisted tiles keep what they held, for
every epilogue that takes a list (none, residual in place, SiLU*up, fp32 split-K slabs), rings of an even and
an odd number of K-tiles down to the minimum of three, a ragged last tile, and the scheduler's edges (one
item per block with idle CUs; several items per block in non-adjacent M-tiles)."""
import math

import pytest
import torch

import exact_cases as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32

M0 = 3 * 256 + 17  # four tiles, the last one ragged
LISTS = ([3], [0, 2], [0, 1, 2, 3], [1])
CANARY = -7.0
EPIS = ("none", "resid", "silu_mul", "splitk")
# per slab / per GEMM: 4 K-tiles, the minimum of 3 (K = 192) and 5 (K = 192 + 128): odd counts flip the ring slot
# parity from one tile to the next
KS = (256, 192, 320)


def _tiles(lst):
    return torch.tensor(lst, dtype=torch.int32, device=DEV)


def _row_mask(M, lst):
    m = torch.zeros(M, dtype=torch.bool)
    for t in lst:
        m[t * 256:min(M, (t + 1) * 256)] = True
    return m.to(DEV)


def _raw_gemm(native, x, w, out, resid, epi, mt):
    """The C entry point: the Python wrapper refuses K % 128 != 0, the kernel takes any K % 64 == 0 >= 192."""
    from rag_llm_k8s_amd.ops._lib import check, lib, ptr, stream_ptr
    from rag_llm_k8s_amd.ops.reference import EPI

    M, K = x.shape
    N = w.shape[0] // 2 if epi == "silu_mul" else w.shape[0]
    check(lib().ragk_gemm_w4(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), out.stride(0), None,
                             ptr(resid), resid.stride(0) if resid is not None else 0, M, N, K, EPI[epi], 0,
                             ptr(mt), mt.numel() if mt is not None else 0, stream_ptr()), "ragk_gemm_w4")


def _raw_splitk(native, x, w, out, ns, mt):
    from rag_llm_k8s_amd.ops._lib import check, lib, ptr, stream_ptr

    M, K = x.shape
    check(lib().ragk_gemm_w4_splitk(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), M, w.shape[0],
                                    K, ns, ptr(mt), mt.numel() if mt is not None else 0, stream_ptr()),
          "ragk_gemm_w4_splitk")


def _run(native, epi, x, w, r, mt):
    """One call of form `epi` into canary-filled outputs; returns the tensor the call writes (the residual form
    runs in place on a copy of r: there r itself is the pattern written beforehand)."""
    M, K = x.shape
    wrap = K % 128 == 0
    if epi == "splitk":
        out = torch.full((2, M, w.shape[0]), CANARY, dtype=F32, device=DEV)
        if wrap and K // 2 >= 256:
            native.gemm_splitk(x, w, 2, out=out, m_tiles=mt)
        else:
            _raw_splitk(native, x, w, out, 2, mt)
        return out
    if epi == "resid":
        h = r.clone()
        if wrap:
            native.gemm(x, w, resid=h, epi="resid", out=h, path=6, m_tiles=mt)
        else:
            _raw_gemm(native, x, w, h, h, epi, mt)
        return h
    N = w.shape[0] // 2 if epi == "silu_mul" else w.shape[0]
    out = torch.full((M, N), CANARY, dtype=BF16, device=DEV)
    if wrap:
        native.gemm(x, w, epi=epi, out=out, path=6, m_tiles=mt)
    else:
        _raw_gemm(native, x, w, out, None, epi, mt)
    return out


def _operands(epi, M, N, K, random=False):
    """Exact-integer operands (tests/exact_cases.py: any summation order gives the same fp32 accumulator) or
    random bf16 ones; N = weight rows (512: for SiLU*up 2 x 256 packed gate/up rows)."""
    Kt = 2 * K if epi == "splitk" else K
    if random:
        g = torch.Generator().manual_seed(M + N + Kt)
        x = torch.randn(M, Kt, generator=g)
        w = torch.randn(N, Kt, generator=g) / math.sqrt(Kt)
        r = torch.randn(M, N, generator=g)
    elif epi == "silu_mul":
        x, gate, up = X.silu_inputs(M, N // 2, Kt)
        w, r = X.pack_gate_up(gate, up), torch.zeros(M, N // 2)
    else:
        x, w, _, r = X.gemm_inputs(M, N, Kt)
    return x.to(BF16).to(DEV), w.to(BF16).to(DEV), r.to(BF16).to(DEV)


def _check(native, epi, x, w, r, lst, full=None):
    M = x.shape[0]
    full = _run(native, epi, x, w, r, None) if full is None else full
    got = _run(native, epi, x, w, r, _tiles(lst))
    rows = _row_mask(M, lst)
    assert torch.equal(got[..., rows, :], full[..., rows, :]), (epi, lst, "listed rows differ from the full call")
    before = r if epi == "resid" else torch.full_like(got, CANARY)
    assert torch.equal(got[..., ~rows, :], before[..., ~rows, :]), (epi, lst, "an unlisted row was written")
    return full


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("epi", EPIS)
def test_listed_rows_equal_full_call(native, epi, K):
    x, w, r = _operands(epi, M0, 512, K)
    full = None
    for lst in LISTS:
        full = _check(native, epi, x, w, r, lst, full)
    if epi in ("none", "resid") and K == 256:  # and the full call is the exact product (rounded once to bf16)
        ref = X.expected(X.acc64(x.cpu(), w.cpu()), None, r.cpu(), epi)
        assert torch.equal(full.cpu(), ref)


@pytest.mark.parametrize("epi", EPIS)
def test_listed_rows_equal_full_call_random(native, epi):
    x, w, r = _operands(epi, M0, 512, 256, random=True)
    _check(native, epi, x, w, r, [0, 2])


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M,N,lst,grid", [
    (40 * 256, 2048, [3, 37], 8),   # 16 items on 8 blocks: each block streams tile 3 then tile 37
    (40 * 256, 2048, [3, 37], -1),  # 16 items, one per block, the other CUs idle
    (M0, 4096, [1], -1),            # 16 items of one M-tile
    (M0, 4096, [3], 8),             # the ragged tile, two items per block
])
def test_scheduler_edges(native, epi, M, N, lst, grid):
    x, w, r = _operands(epi, M, N, 256)
    full = _run(native, epi, x, w, r, None)
    native.set_w4_grid(grid)
    try:
        _check(native, epi, x, w, r, lst, full)
    finally:
        native.set_w4_grid(-1)


def test_m_tiles_refused_elsewhere(native):
    """A list is taken by the gemm_w4 path only; any other path, an fp32 output or a bias epilogue raises."""
    x, w, r = _operands("none", M0, 512, 256)
    mt = _tiles([1])
    with pytest.raises(ValueError):
        native.gemm(x, w, path=2, m_tiles=mt)
    with pytest.raises(ValueError):
        native.gemm(x, w, out_f32=True, m_tiles=mt)
    with pytest.raises(ValueError):
        native.gemm(x, w, bias=torch.zeros(512, dtype=BF16, device=DEV), epi="bias", m_tiles=mt)
    with pytest.raises(ValueError):
        native.gemm(x, w, m_tiles=_tiles([0, 1, 2, 3, 3]))  # more entries than tiles
    out = torch.full((M0, 512), CANARY, dtype=BF16, device=DEV)
    native.gemm(x, w, out=out, m_tiles=_tiles([]))  # an empty list: nothing to do
    assert torch.equal(out, torch.full_like(out, CANARY))
