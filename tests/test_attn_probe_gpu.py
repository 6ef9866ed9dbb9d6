"""Which keys does each query see? Column-coded probes and stale-cache invariance of the attention kernels.

Probe: V[j, h, :] is one-hot at column j % D, so out[i, h, c] is the softmax mass of the visible keys
j = c (mod D). Every element is checked against a float64 oracle within 2^-6 relative (twice the worst case of a
bf16-rounded P plus a bf16-rounded output), and must be exactly 0 where no visible key maps to the column. The
oracle itself shows that every visible key holds at least 4 * 2^-6 of its column (asserted here and, without a
GPU, in tests/test_exact_cpu.py): a key dropped at a tile or partition boundary, counted twice, or visible one
position early fails by a factor of four. A norm over 4k keys sees none of these.

Stale cache: every paged kernel runs twice on caches that differ only where no query may look -- rows past
kv_len in the last block, blocks in no block table, and the block that every table entry past ceil(kv_len / 64)
points at -- zeros in one run, +-2^60 in the other (fp8: arbitrary scale words, NaN and Inf included, and random
finite codes). The outputs must be bit-identical.

q is the [:, :Hq*D] view of a qkv-wide buffer, as the engine passes it, and out a strided view whose row gaps
hold a sentinel that must survive."""
import functools

import pytest
import torch

import exact_cases as X
from rag_llm_k8s_amd.ops import reference as R
from rag_llm_k8s_amd.ops.fp8 import FP8, Fp8KV, quantize_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
BS = X.BS


@functools.lru_cache(maxsize=None)
def _case(q_lens, kv_lens, Hq, Hkv, D, causal=True, fp8=False):
    """(q, K rows, V rows, oracle, layout) of one probe, computed once and shared by the tests that use it. fp8:
    K as quantize_rows stores it (the oracle sees the dequantized rows, as tests/test_kv_fp8_gpu.py builds it)."""
    q, Ks, Vs, ref, share = X.probe_case(list(q_lens), list(kv_lens), Hq, Hkv, D, causal)
    K8 = None
    if fp8:
        K8 = []
        for i, K in enumerate(Ks):
            c, s = quantize_rows(K.reshape(-1, D))
            K8.append((c.view(torch.uint8).view(K.shape), s.view(K.shape[:2])))
            Ks[i] = (c.float() * s[:, None]).view(K.shape)
        ref, share = X.probe_oracle(q, Ks, list(q_lens), list(kv_lens), Hq, D, causal)
    assert share >= X.MIN_SHARE, share
    return q, Ks, Vs, K8, ref, X.paged_layout(list(kv_lens))


def _place(cache, rows, kv_lens, bt):
    """rows[s] [L, Hkv, ...] -> cache [total, Hkv, BS, ...] through the block table."""
    for s, (L, r) in enumerate(zip(kv_lens, rows)):
        for b in range(-(-L // BS)):
            n = min(BS, L - b * BS)
            cache[int(bt[s, b]), :, :n] = r[b * BS:b * BS + n].transpose(0, 1)


def _caches(case, kv_lens, Hkv, D, stale, fp8):
    """(k cache, v cache, block tables) on the GPU; the hidden slots hold zeros or, with stale, garbage."""
    q, Ks, Vs, K8, ref, (bt, hidden, total) = case
    if not fp8:
        kc = X.paged_fill(Ks, kv_lens, bt, total, Hkv, D, hidden, stale, seed=1)
        vc = X.paged_fill(Vs, kv_lens, bt, total, Hkv, D, hidden, stale, seed=2)
        return kc.to(DEV), vc.to(DEV), bt.to(DEV)
    out = []
    one = torch.ones(1).to(FP8).view(torch.uint8)
    for side, seed in (("k", 1), ("v", 2)):
        if stale:
            data = X.hidden_fp8_codes((total, Hkv, BS, D), seed)
            scale = X.hidden_scale_bits((total, Hkv, BS), seed)
        else:
            data = torch.zeros(total, Hkv, BS, D, dtype=torch.uint8)
            scale = torch.zeros(total, Hkv, BS)
        if side == "k":
            _place(data, [c for c, _ in K8], kv_lens, bt)
            _place(scale, [s for _, s in K8], kv_lens, bt)
        else:  # one-hot rows, code of 1.0 with scale 1.0: dequantizes exactly
            _place(data, [(v.float() * float(one)).to(torch.uint8) for v in Vs], kv_lens, bt)
            _place(scale, [torch.ones(v.shape[:2]) for v in Vs], kv_lens, bt)
        out.append(Fp8KV(data.to(DEV).view(FP8), scale.to(DEV)))
    return out[0], out[1], bt.to(DEV)


def _q_view(q, Hq, Hkv, D):
    """q as the engine passes it: the first Hq*D columns of the qkv-wide projection buffer."""
    buf = torch.full((q.shape[0], (Hq + 2 * Hkv) * D), X.SENT, device=DEV).bfloat16()
    buf[:, :Hq * D] = q.to(DEV)
    return buf[:, :Hq * D]


def _out_view(T, W):
    buf = torch.full((T, W + 24), X.SENT, device=DEV).bfloat16()
    view = buf[:, 8:8 + W]
    view.fill_(float("nan"))
    return buf, view


def _prefill(native, q_lens, kv_lens, Hq, Hkv, D, stale, fp8=False):
    case = _case(tuple(q_lens), tuple(kv_lens), Hq, Hkv, D, True, fp8)
    kc, vc, bt = _caches(case, kv_lens, Hkv, D, stale, fp8)
    T = sum(q_lens)
    cu = torch.tensor([0] + list(torch.cumsum(torch.tensor(q_lens), 0)), dtype=torch.int32, device=DEV)
    kvl = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    tiles = native.build_prefill_tiles(q_lens, Hq, Hkv).to(DEV)
    buf, out = _out_view(T, Hq * D)
    native.attn_prefill(_q_view(case[0], Hq, Hkv, D), kc, vc, cu, kvl, tiles, out, Hq, Hkv, D, causal=True, paged=True,
                        block_tables=bt)
    torch.cuda.synchronize()
    assert X.gaps_intact(buf, 8, Hq * D), "row gaps of out"
    return out.cpu(), case[4]


def _both(run):
    """Run on the clean and on the stale cache: bit-identical outputs; returns the stale run's."""
    a, ref = run(False)
    b, _ = run(True)
    assert torch.equal(a, b), "%d elements depend on slots no query may see" % int((a.float() != b.float()).sum())
    return b, ref


# ----------------------------------------------------------------------------------------------- prefill
@pytest.mark.parametrize("q_lens,kv_lens", X.PREFILL_LENS)
@pytest.mark.parametrize("Hq,Hkv", X.PREFILL_HEADS_V3 + X.PREFILL_HEADS_GENERIC)
def test_prefill_probe(native, q_lens, kv_lens, Hq, Hkv):
    """D = 128, paged, causal: the pipelined 8-wave kernel (4 query heads per KV head) and the generic one."""
    out, ref = _prefill(native, q_lens, kv_lens, Hq, Hkv, 128, stale=True)
    X.probe_check(out, ref)


@pytest.mark.parametrize("q_lens,kv_lens", X.PREFILL_LENS)
@pytest.mark.parametrize("Hq,Hkv", X.PREFILL_D64)
def test_prefill_probe_d64(native, q_lens, kv_lens, Hq, Hkv):
    """D = 64: one query head per KV head (the GPT-2 route) and four (8-wave blocks)."""
    out, ref = _prefill(native, q_lens, kv_lens, Hq, Hkv, 64, stale=True)
    X.probe_check(out, ref)


@pytest.mark.parametrize("q_lens,kv_lens", X.PREFILL_LENS)
@pytest.mark.parametrize("Hq,Hkv", X.PREFILL_HEADS_V3 + X.PREFILL_HEADS_GENERIC)
def test_prefill_probe_fp8(native, q_lens, kv_lens, Hq, Hkv):
    """The same probes on the fp8 cache (4, 2 and 1 query heads per block)."""
    out, ref = _prefill(native, q_lens, kv_lens, Hq, Hkv, 128, stale=True, fp8=True)
    X.probe_check(out, ref)


@pytest.mark.parametrize("Hq,Hkv,D,fp8", [(h, k, 128, f) for f in (False, True)
                                           for h, k in X.PREFILL_HEADS_V3 + X.PREFILL_HEADS_GENERIC]
                         + [(h, k, 64, False) for h, k in X.PREFILL_D64])  # the fp8 cache: head_dim 128 only
def test_prefill_stale_cache_invariant(native, Hq, Hkv, D, fp8):
    for q_lens, kv_lens in X.PREFILL_LENS[2:]:
        _both(lambda stale: _prefill(native, q_lens, kv_lens, Hq, Hkv, D, stale, fp8))


@pytest.mark.parametrize("D,H", X.ENCODER)
def test_encoder_probe(native, D, H):
    """Contiguous, non-causal. The kernel clamps the rows of a K/V tile past kv_len onto row kv_len - 1: the
    value check catches that row being counted more than once."""
    lens = X.ENCODER_LENS
    q, Ks, Vs, _, ref, _ = _case(tuple(lens), tuple(lens), H, H, D, False)
    T = sum(lens)
    qkv = torch.cat([q, torch.cat(Ks).reshape(T, H * D), torch.cat(Vs).reshape(T, H * D)], 1).to(DEV)
    cu = torch.tensor([0] + list(torch.cumsum(torch.tensor(lens), 0)), dtype=torch.int32, device=DEV)
    kvl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    tiles = native.build_prefill_tiles(lens, H, H).to(DEV)
    buf, out = _out_view(T, H * D)
    native.attn_prefill(qkv, qkv[:, H * D:], qkv[:, 2 * H * D:], cu, kvl, tiles, out, H, H, D, causal=False,
                        paged=False, cu_kv=cu, kv_stride=3 * H * D)
    torch.cuda.synchronize()
    assert X.gaps_intact(buf, 8, H * D)
    X.probe_check(out.cpu(), ref)


# ----------------------------------------------------------------------------------------------- decode
def _decode(native, Hq, Hkv, stale, fp8, parts, D=128):
    kv_lens = X.DECODE_LENS
    B = len(kv_lens)
    case = _case((1,) * B, tuple(kv_lens), Hq, Hkv, D, True, fp8)
    kc, vc, bt = _caches(case, kv_lens, Hkv, D, stale, fp8)
    kvl = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    pt, mp = parts
    buf, out = _out_view(B, Hq * D)
    native.attn_decode(_q_view(case[0], Hq, Hkv, D), kc, vc, bt, kvl, out, Hq, Hkv, D, pt, mp)
    torch.cuda.synchronize()
    assert X.gaps_intact(buf, 8, Hq * D), "row gaps of out"
    return out.cpu(), case[4]


def _split_parts(native, Hkv):
    pt, mp = native.decode_partitions(max(X.DECODE_LENS), len(X.DECODE_LENS), Hkv, target_blocks=1024, min_tiles=1)
    assert mp > 1
    return pt, mp


def _single_parts(native, monkeypatch, Hkv, kl, nt):
    monkeypatch.setattr(native, "DECODE_NW8_MIN_PAIRS", 1)
    monkeypatch.setattr(native, "DECODE_KL", bool(kl))
    monkeypatch.setattr(native, "DECODE_NT_MIN_BH", 1 if nt else 1 << 30)
    pt, mp = native.decode_partitions(max(X.DECODE_LENS), len(X.DECODE_LENS), Hkv)
    assert mp == 1
    return pt, mp


DECODE_SPLIT = [(h, k, d, False) for h, k, d in X.DECODE_SPLIT] + [(h, k, d, True) for h, k, d in X.DECODE_SPLIT if d == 128]


@pytest.mark.parametrize("Hq,Hkv,D,fp8", DECODE_SPLIT)
def test_decode_split_k_probe_and_stale(native, Hq, Hkv, D, fp8):
    """One 64-key tile per partition, 9 partitions: every partition boundary of the 300- and 513-key contexts,
    and partitions past the short ones; every (D, heads per KV head) instantiation of the split-K kernel."""
    parts = _split_parts(native, Hkv)
    out, ref = _both(lambda stale: _decode(native, Hq, Hkv, stale, fp8, parts, D))
    X.probe_check(out, ref)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("kl", [0, 1])
@pytest.mark.parametrize("Hq,Hkv", X.DECODE_HEADS_SINGLE)
def test_decode_single_partition_probe_and_stale(native, Hq, Hkv, kl, nt, fp8, monkeypatch):
    """The batch-32 grid: 8-wave blocks with K in registers (kl = 0; fp8: 4-wave split-K blocks with one
    partition) and 4-wave blocks with K tiles by LDS-DMA (kl = 1), non-temporal loads off and on."""
    parts = _single_parts(native, monkeypatch, Hkv, kl, nt)
    out, ref = _both(lambda stale: _decode(native, Hq, Hkv, stale, fp8, parts))
    X.probe_check(out, ref)


def _decode_rope(native, Hq, Hkv, stale, fp8, parts, D=128):
    """attn_decode_rope: the new token's q / k / v come from qkv partial slabs, its k / v rows are appended at
    position kv_len - 1. Returns the output and both caches as float32 CPU tensors."""
    kv_lens, S = X.DECODE_LENS, 3
    B = len(kv_lens)
    case = _case((1,) * B, tuple(kv_lens), Hq, Hkv, D, True, fp8)
    bt0, hidden, total = case[5]
    kc, vc, bt = _caches(case, kv_lens, Hkv, D, stale, fp8)
    kvl = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    pos = kvl - 1
    slots = (bt[torch.arange(B, device=DEV), (pos // BS).long()] * BS + pos % BS).int()
    P = (0.3 * torch.randn(S, B, (Hq + 2 * Hkv) * D, generator=torch.Generator().manual_seed(5))).to(DEV)
    cos, sin = R.rope_tables(D, 1024, theta=500000.0)
    pt, mp = parts
    buf, out = _out_view(B, Hq * D)
    before = [(c.data.view(torch.uint8).clone(), c.scale.view(torch.int32).clone()) if fp8 else (c.clone(),)
              for c in (kc, vc)]
    native.attn_decode_rope(P, pos, cos.to(DEV), sin.to(DEV), slots, kc, vc, bt, kvl, out, Hq, Hkv, D, pt, mp)
    torch.cuda.synchronize()
    assert X.gaps_intact(buf, 8, Hq * D), "row gaps of out"
    after = [(c.data.view(torch.uint8), c.scale.view(torch.int32)) if fp8 else (c,) for c in (kc, vc)]
    live = []
    for bef, aft in zip(before, after):
        for b, a in zip(bef, aft):
            h = hidden.to(DEV)[:, None, :].expand(a.shape[:3])
            assert torch.equal(a[h], b[h]), "a hidden cache slot was written"  # bit patterns: NaN scales included
            live.append(a[~h].cpu())
    return (out.cpu(), live), None


@pytest.mark.parametrize("Hq,Hkv,D,fp8,route", [(h, k, d, f, "split") for h, k, d, f in DECODE_SPLIT]
                         + [(h, k, 128, f, r) for f in (False, True) for r in ("single_kl", "single_nw8")
                            for h, k in X.DECODE_HEADS_SINGLE])
def test_decode_rope_stale_cache_invariant(native, Hq, Hkv, D, fp8, route, monkeypatch):
    """Split-K (every instantiation), and the single-partition grid with K tiles by LDS-DMA (kl) and on the
    8-wave blocks (nw8)."""
    parts = (_split_parts(native, Hkv) if route == "split"
             else _single_parts(native, monkeypatch, Hkv, route == "single_kl", 1))
    (a, la), _ = _decode_rope(native, Hq, Hkv, False, fp8, parts, D)
    (b, lb), _ = _decode_rope(native, Hq, Hkv, True, fp8, parts, D)
    assert bool(torch.isfinite(a.float()).all())
    assert torch.equal(a, b), "%d output elements depend on slots no query may see" % int((a.float() != b.float()).sum())
    for x, y in zip(la, lb):
        assert torch.equal(x, y), "the live cache rows differ after the append"
