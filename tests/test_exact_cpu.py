"""The conditions tests/test_exact_gpu.py and tests/test_attn_probe_gpu.py rely on, checked on the oracles alone
(no GPU): integer GEMM operands keep every fp32 partial sum exact, every visible key of an attention probe holds
a share of its output column that the tolerance cannot hide, and the strided operand views stay 16-byte aligned."""
import pytest
import torch

import exact_cases as X


def _acc_bound(K, amp):
    """max |partial sum| over any summation order <= sum |x_k w_k| <= K amp^2."""
    return K * amp * amp


@pytest.mark.parametrize("M,N,K", sorted(set(X.ALL_GEMM_SHAPES)))
def test_every_partial_sum_is_exact(M, N, K):
    assert K <= 14336 and _acc_bound(K, 8) + 8 + 64 < X.ACC_LIMIT


@pytest.mark.parametrize("M,N,K", [(64, 1000, 4096), (17, 1000, 14336), (200, 264, 384)])
def test_float64_and_fp32_products_identical(M, N, K):
    """The fp32 product (any blocking the CPU BLAS picks) equals the float64 one bit for bit, and the sum of the
    absolute products -- a bound on every partial sum in any order -- stays below 2^24."""
    x, w, b, r = X.gemm_inputs(M, N, K)
    a64 = X.acc64(x, w)
    assert torch.equal((x.float() @ w.float().t()).double(), a64)
    assert float((x.abs() @ w.abs().t()).max()) < X.ACC_LIMIT
    assert float(a64.abs().max()) < 2 ** 15  # the observed sums are far smaller than the bound
    for epi in X.LINEAR_EPIS:
        e = X.expected(a64, b, r, epi)
        assert e.dtype == torch.bfloat16
    # the bf16 rounding point is really exercised: most sums are not bf16 numbers
    f = X.expected(a64, b, r, "bias_resid", out_f32=True)
    assert float((f.bfloat16().float() != f).float().mean()) > 0.5 or K < 1024


def test_part_shapes_cover_every_slice_width():
    """gemm_part is built for K-slices of 4, 8, 14, 16, 28 and 32 steps; the matrix reaches each of them."""
    assert {ks for M, N, K in X.PART for ks in X.part_legal_ks(M, K)} == X.PART_KS
    assert all(X.part_legal_ks(M, K) for M, N, K in X.PART)


def test_slab_sums_exact_and_rounded():
    for S in X.SLABS:
        P = X.slab_ints(S, 5, 256, seed=S)
        s64 = P.double().sum(0)
        assert float(P.abs().sum(0).max()) < X.ACC_LIMIT
        assert torch.equal(P.sum(0).double(), s64)
        assert float((s64.float().bfloat16().float() != s64.float()).float().mean()) > 0.5


def test_activation_inputs_small():
    for route, M, N, K in X.ACT + X.SILU:
        assert K <= 384
    x, g, u = X.silu_inputs(17, 128, 384)
    assert float(x.abs().max()) == 1 and bool((g[:64] == 0).all()) and bool((u[64:128] == 0).all())
    gate, up = X.acc64(x, g), X.acc64(x, u)
    ref = X.silu_expected(gate, up)
    assert bool((ref[:, :128] == 0).all())


def _share(q_lens, kv_lens, Hq, Hkv, D, causal=True, seed=0):
    q, Ks, Vs, ref, share = X.probe_case(q_lens, kv_lens, Hq, Hkv, D, causal, seed)
    assert all(bool((v.float().sum(-1) == 1).all()) for v in Vs)  # one-hot V rows
    return ref, share


@pytest.mark.parametrize("q_lens,kv_lens", X.PREFILL_LENS)
@pytest.mark.parametrize("Hq,Hkv,D", [(h, k, 128) for h, k in X.PREFILL_HEADS_V3 + X.PREFILL_HEADS_GENERIC]
                         + [(h, k, 64) for h, k in X.PREFILL_D64])
def test_prefill_probe_share(q_lens, kv_lens, Hq, Hkv, D):
    ref, share = _share(q_lens, kv_lens, Hq, Hkv, D)
    assert share >= X.MIN_SHARE, share
    assert torch.allclose(ref.sum(-1), torch.ones(ref.shape[:2], dtype=torch.float64))


@pytest.mark.parametrize("D,H", X.ENCODER)
def test_encoder_probe_share(D, H):
    ref, share = _share(X.ENCODER_LENS, X.ENCODER_LENS, H, H, D, causal=False)
    assert share >= X.MIN_SHARE, share


@pytest.mark.parametrize("Hq,Hkv,D", sorted(set(X.DECODE_SPLIT + [(h, k, 128) for h, k in X.DECODE_HEADS_SINGLE])))
def test_decode_probe_share(Hq, Hkv, D):
    L = X.DECODE_LENS
    ref, share = _share([1] * len(L), L, Hq, Hkv, D)
    assert share >= X.MIN_SHARE, share
    # causal prefill rows: the columns of keys not yet visible are exact zeros in the oracle
    ref2, _ = _share([37], [37], Hq, Hkv, D)
    assert bool((ref2[0, :, 1:] == 0).all()) and bool((ref2[0, :, 0] == 1).all())


def _as_kernel(ref):
    """The oracle after the roundings a correct kernel makes: P to bf16 (2^-9 relative per key) and the output
    to bf16; modelled as the two worst-case relative errors stacked."""
    return (ref * (1 + 2.0 ** -9)).float().bfloat16()


@pytest.mark.parametrize("q_lens,kv_lens,Hq,Hkv,D,causal", [([5, 70], [513, 70], 8, 2, 128, True),
                                                           ([1] * 6, X.DECODE_LENS, 4, 1, 128, True),
                                                           (X.ENCODER_LENS, X.ENCODER_LENS, 12, 12, 32, False)])
def test_probe_check_catches_one_wrong_key(q_lens, kv_lens, Hq, Hkv, D, causal):
    """The check passes a correctly rounded output and fails when ONE key per query is dropped, counted twice
    or (causal) visible one position early -- what a norm over the row cannot see."""
    q, Ks, _, ref, share = X.probe_case(q_lens, kv_lens, Hq, Hkv, D, causal)
    X.probe_check(_as_kernel(ref), ref)

    def one_key(value):
        def mult(vis):  # the last key of the first 64-key tile where visible, else the first key
            m = vis.float()
            j = 63 if vis.shape[1] > 63 else 0
            m[:, j] = torch.where(vis[:, j], torch.tensor(float(value)), m[:, j])
            if value == 0 and not bool((m.sum(1) > 0).all()):
                m[m.sum(1) == 0, 0] = 1.0  # a query whose only key it is keeps it
            return m
        return mult

    def early(vis):
        m = vis.clone()
        m[:, 1:] |= vis[:, :-1]  # key j + 1 visible wherever key j is
        return m.float()

    # a NaN the kernel produces, and a row of the NaN-prefilled output it never wrote
    for row in (0, ref.shape[0] - 1):
        for cols in (slice(None), slice(3, 4)):
            nan = _as_kernel(ref).float()
            nan[row, 0, cols] = float("nan")
            with pytest.raises(AssertionError, match="non-finite"):
                X.probe_check(nan.bfloat16(), ref)
    inf = _as_kernel(ref).float()
    inf[0, 0, 0] = float("inf")
    with pytest.raises(AssertionError, match="non-finite"):
        X.probe_check(inf.bfloat16(), ref)

    for mult in [one_key(0), one_key(2)] + ([early] if causal and max(q_lens) > 1 else []):
        wrong, _ = X.probe_oracle(q, Ks, q_lens, kv_lens, Hq, D, causal, mult=mult)
        assert float((wrong - ref).abs().max()) > 1e-3
        with pytest.raises(AssertionError):
            X.probe_check(_as_kernel(wrong), ref)


def test_paged_layout_hides_what_no_query_may_see():
    kv = [100, 300, 129]
    bt, hidden, total = X.paged_layout(kv)
    nb = [-(-L // 64) for L in kv]
    live = {int(b) for s, n in enumerate(nb) for b in bt[s, :n]}
    assert len(live) == sum(nb) and total == sum(nb) + 3
    decoy = int(bt[0, nb[0]])
    assert decoy not in live and 0 <= decoy < total and bool(hidden[decoy].all())
    assert all(bool((bt[s, n:] == decoy).all()) for s, n in enumerate(nb))
    assert int((~hidden).sum()) == sum(kv)
    rows = [torch.ones(L, 2, 128) for L in kv]
    a = X.paged_fill(rows, kv, bt, total, 2, 128, hidden, stale=False)
    b = X.paged_fill(rows, kv, bt, total, 2, 128, hidden, stale=True)
    h = hidden[:, None, :, None].expand_as(a)
    assert torch.equal(a[~h], b[~h]) and bool((a[h] == 0).all()) and bool((b[h].float().abs() == X.BIG).all())
    w = X.hidden_scale_bits((total, 2, 64))
    assert bool(torch.isnan(w).any()) and bool(torch.isinf(w).any())
    c = X.hidden_fp8_codes((total, 2, 64, 128)).view(torch.float8_e4m3fn).float()
    assert bool(torch.isfinite(c).all())


@pytest.mark.parametrize("dtype,off", [(torch.bfloat16, 8), (torch.float32, 8), (torch.float8_e4m3fn, 16),
                                        (torch.bfloat16, 16)])
def test_strided_views_are_16_byte_aligned(dtype, off):
    t = torch.zeros(5, 136)
    buf, v = X.strided(t, off, 24, dtype)  # pitches 168 / 176 elements: multiples of 16 bytes in every dtype
    assert X.aligned16(v) and not v.is_contiguous() and v.shape == t.shape
    assert X.gaps_intact(buf, off, 136)
    buf[2, 0] = 1
    assert not X.gaps_intact(buf, off, 136)
    assert not X.aligned16(buf[:, 1:137])  # the misaligned views of the validation tests really are misaligned
