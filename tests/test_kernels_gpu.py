"""T1 kernel tier: every gfx950 HIP kernel vs a plain PyTorch fp32 reference of the same op."""
import math

import numpy as np
import pytest
import torch

from rag_llm_k8s_amd.ops import reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.parametrize("M,N,K", [(1, 256, 256), (7, 4096, 512), (64, 512, 1024), (100, 384, 384), (256, 512, 512),
                                   (300, 1024, 768), (1111, 6144, 4096)])
def test_gemm_plain(native, M, N, K):
    torch.manual_seed(0)
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    y = native.gemm(x, w)
    ref = x.float() @ w.float().t()
    assert rel_err(y, ref) < 1e-2


@pytest.mark.parametrize("M,N,K", [(1, 256, 128), (300, 1024, 768), (1111, 6144, 4096), (256, 256, 128),
                                   (2049, 512, 1024), (513, 4104, 256), (260, 768, 384), (700, 1024, 384)])
@pytest.mark.parametrize("kernel", ["pp", "w4"])
def test_gemm_pingpong(native, M, N, K, kernel):
    """The two 256x256 large-M kernels: gemm_w4 (4 waves, the prefill default, K >= 192) and gemm_pp (8-wave
    ping-pong, 64-bit addressing: the fallback for operands past 2 GiB)."""
    if kernel == "w4":
        if K < 192:
            pytest.skip("gemm_w4 needs three K-tiles per tile")
        _check_pingpong(native, M, N, K, path=6)
        return
    _check_pingpong(native, M, N, K, path=2)


@pytest.mark.parametrize("grid", [8, 16])
@pytest.mark.parametrize("M,N,K", [(1111, 1024, 256), (513, 4104, 256), (2048, 512, 256), (777, 1280, 384),
                                   (1030, 768, 1024)])
def test_gemm_w4_persistent(native, M, N, K, grid):
    """Persistent gemm_w4: a few blocks loop over every tile (full and edge tiles, rings of 4-16 K-tiles), so the next-tile staging inside the K-stream, the register epilogue and the counted
    waits around it run many times per block."""
    native.set_w4_grid(grid)
    try:
        _check_pingpong(native, M, N, K, path=6)
    finally:
        native.set_w4_grid(-1)


def test_gemm_w4_grid_independent(native):
    """A tile's K-loop and epilogue do not depend on which block computes it or how many tiles the block
    streams before it: every grid (one block per tile, 8 / 24 blocks, one per CU) gives bit-identical
    outputs, for the plain, residual (in place), SiLU*up, bias+GELU and fp32 split-K forms."""
    torch.manual_seed(23)
    M, N, K = 1300, 1536, 640
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    r = torch.randn(M, N, device=DEV).bfloat16()
    b = torch.randn(N, device=DEV).bfloat16()
    outs = []
    for grid in (-1, 0, 8, 24):
        native.set_w4_grid(grid)
        try:
            h = r.clone()
            native.gemm(x, w, resid=h, epi="resid", out=h, path=6)
            outs.append((native.gemm(x, w, path=6), h, native.gemm(x, w, epi="silu_mul", path=6),
                         native.gemm(x, w, bias=b, epi="bias_gelu", path=6), native.gemm_splitk(x, w, 2)))
        finally:
            native.set_w4_grid(-1)
    for o in outs[1:]:
        for a, c in zip(outs[0], o):
            assert torch.equal(a, c)


def test_gemm_large_m_routing(native, monkeypatch):
    """Large-M prefill GEMMs: every epilogue runs on the hand-written gemm_w4 by default (PREFILL_BLAS =
    "none": the default route equals an explicit path-6 call bit for bit, residual add in place included);
    the A/B route PREFILL_BLAS = "resid" (in-place hipBLASLt addmm) agrees within bf16 rounding of gemm_w4
    and of fp32."""
    torch.manual_seed(21)
    M, N, K = 8192 + 17, 1024, 512
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    r = torch.randn(M, N, device=DEV).bfloat16()
    assert native.PREFILL_BLAS == "none"
    assert torch.equal(native.gemm(x, w), native.gemm(x, w, path=6))
    w4 = native.gemm(x, w, resid=r, epi="resid", path=6)
    h2 = r.clone()
    native.gemm(x, w, resid=h2, epi="resid", out=h2)  # default route, in place
    assert torch.equal(h2, w4)
    ref = x.float() @ w.float().t() + r.float()
    assert rel_err(w4, ref) < 1e-2
    monkeypatch.setattr(native, "PREFILL_BLAS", "resid")
    h = r.clone()
    native.gemm(x, w, resid=h, epi="resid", out=h)
    assert rel_err(h, ref) < 1e-2
    assert (h.float() - w4.float()).abs().max().item() <= 2 * (ref.abs().max().item() * 2 ** -8)
    y = torch.empty_like(r)
    native.gemm(x, w, resid=r, epi="resid", out=y)  # out-of-place form
    assert torch.equal(y, h)


def _check_pingpong(native, M, N, K, path=2):
    torch.manual_seed(20)
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    b = torch.randn(N, device=DEV).bfloat16()
    r = torch.randn(M, N, device=DEV).bfloat16()
    y = native.gemm(x, w, path=path)
    assert rel_err(y, x.float() @ w.float().t()) < 1e-2
    for epi in ["bias", "resid", "bias_resid", "bias_gelu", "gelu", "bias_gelu_tanh"]:
        y = native.gemm(x, w, bias=b, resid=r, epi=epi, path=path)
        assert rel_err(y.cpu(), R.linear(x.cpu(), w.cpu(), b.cpu(), r.cpu(), epi=epi)) < 1e-2, epi
    yf = native.gemm(x, w, out_f32=True, path=path)
    assert rel_err(yf, x.float() @ w.float().t()) < 1e-3
    if N % 256 == 0:
        g, u = w[: N // 2], w[N // 2:]
        y = native.gemm(x, R.pack_gate_up(g, u), epi="silu_mul", path=path)
        ref = torch.nn.functional.silu(x.float() @ g.float().t()) * (x.float() @ u.float().t())
        assert rel_err(y, ref) < 1e-2


@pytest.mark.parametrize("M", [1, 7, 16, 32, 33, 64])
@pytest.mark.parametrize("N,K", [(4096, 4096), (6144, 4096), (4096, 14336), (384, 512), (1000, 768)])
def test_gemm_decode_v3(native, M, N, K):
    torch.manual_seed(21)
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    r = torch.randn(M, N, device=DEV).bfloat16()
    ref = x.float() @ w.float().t()
    for _ in range(2):  # second call checks the split-K counters were reset
        y = native.gemm(x, w, path=4)
        assert rel_err(y, ref) < 1e-2
    y = native.gemm(x, w, resid=r, epi="resid", path=4)
    assert rel_err(y, ref + r.float()) < 1e-2
    yf = native.gemm(x, w, out_f32=True, path=4)
    assert rel_err(yf, ref) < 1e-3
    if N % 128 == 0:
        g, u = w[: N // 2], w[N // 2:]
        y = native.gemm(x, R.pack_gate_up(g, u), epi="silu_mul", path=4)
        ref2 = torch.nn.functional.silu(x.float() @ g.float().t()) * (x.float() @ u.float().t())
        assert rel_err(y, ref2) < 1e-2


@pytest.mark.parametrize("M", [1, 4, 13])
def test_gemm_skinny_long_k(native, M):
    """Skinny decode GEMM (ragk_gemm routing at M <= 16) on the long-K down projection shape with the
    residual epilogue (K-blocks strided over the block's 8 waves)."""
    torch.manual_seed(22)
    N, K = 4096, 14336
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    r = torch.randn(M, N, device=DEV).bfloat16()
    ref = x.float() @ w.float().t() + r.float()
    assert rel_err(native.gemm(x, w, resid=r, epi="resid"), ref) < 1e-2


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("M", [1, 16, 33, 64])
def test_gemm_paths_agree(native, path, M):
    torch.manual_seed(1)
    K, N = 1024, 768
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / 32).bfloat16()
    y = native.gemm(x, w, path=path)
    assert rel_err(y, x.float() @ w.float().t()) < 1e-2


@pytest.mark.parametrize("M", [1, 5, 64, 200])
def test_gemm_epilogues(native, M):
    torch.manual_seed(2)
    K, N = 512, 640
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / 16).bfloat16()
    b = torch.randn(N, device=DEV).bfloat16()
    r = torch.randn(M, N, device=DEV).bfloat16()
    for epi in ["bias", "resid", "bias_resid", "bias_gelu", "gelu", "bias_gelu_tanh"]:
        y = native.gemm(x, w, bias=b, resid=r, epi=epi)
        ref = R.linear(x.cpu(), w.cpu(), b.cpu(), r.cpu(), epi=epi)
        assert rel_err(y.cpu(), ref) < 1e-2, epi
    yf = native.gemm(x, w, out_f32=True)
    assert yf.dtype == torch.float32 and rel_err(yf, x.float() @ w.float().t()) < 1e-3


@pytest.mark.parametrize("M", [1, 3, 64, 129])
def test_gemm_silu_mul(native, M):
    torch.manual_seed(3)
    K, I = 512, 384
    x = torch.randn(M, K, device=DEV).bfloat16()
    g = (torch.randn(I, K, device=DEV) / 16).bfloat16()
    u = (torch.randn(I, K, device=DEV) / 16).bfloat16()
    wp = R.pack_gate_up(g, u)
    y = native.gemm(x, wp, epi="silu_mul")
    ref = torch.nn.functional.silu(x.float() @ g.float().t()) * (x.float() @ u.float().t())
    assert y.shape == (M, I)
    assert rel_err(y, ref) < 1e-2


def test_gemm_inplace_residual(native):
    torch.manual_seed(4)
    M, K, N = 80, 256, 256
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / 16).bfloat16()
    h = torch.randn(M, N, device=DEV).bfloat16()
    ref = h.float() + x.float() @ w.float().t()
    native.gemm(x, w, resid=h, epi="resid", out=h)
    assert rel_err(h, ref) < 1e-2


@pytest.mark.parametrize("T,H", [(1, 4096), (37, 4096), (5, 384), (8, 1024)])
def test_rmsnorm(native, T, H):
    torch.manual_seed(5)
    x = torch.randn(T, H, device=DEV).bfloat16()
    w = torch.randn(H, device=DEV).bfloat16()
    y = native.rmsnorm(x, w, 1e-5)
    ref = R.rmsnorm(x.cpu(), w.cpu(), 1e-5)
    assert (y.cpu().float() - ref.float()).abs().max().item() <= 0.0625
    assert rel_err(y.cpu(), ref) < 4e-3
    # fused residual
    r = torch.randn(T, H, device=DEV).bfloat16()
    r_ref = r.cpu().clone()
    y2 = native.rmsnorm(x, w, 1e-5, resid=r)
    ref2 = R.rmsnorm(x.cpu(), w.cpu(), 1e-5, resid=r_ref)
    assert torch.equal(r.cpu(), r_ref)
    assert rel_err(y2.cpu(), ref2) < 4e-3


@pytest.mark.parametrize("T,H", [(3, 384), (17, 1024)])
def test_layernorm(native, T, H):
    torch.manual_seed(6)
    x = torch.randn(T, H, device=DEV).bfloat16()
    r = torch.randn(T, H, device=DEV).bfloat16()
    g = torch.randn(H, device=DEV).bfloat16()
    b = torch.randn(H, device=DEV).bfloat16()
    y = native.layernorm(x, g, b, 1e-12, resid=r)
    assert rel_err(y.cpu(), R.layernorm(x.cpu(), g.cpu(), b.cpu(), 1e-12, resid=r.cpu())) < 1e-2


def test_embed_and_gather(native):
    V, H = 1000, 256
    table = torch.randn(V, H, device=DEV).bfloat16()
    ids = torch.randint(0, V, (33,), device=DEV, dtype=torch.int32)
    assert torch.equal(native.embed(ids, table), table[ids.long()])
    idx = torch.tensor([3, 0, 32], dtype=torch.int32, device=DEV)
    e = native.embed(ids, table)
    assert torch.equal(native.gather_rows(e, idx), e[idx.long()])


def test_embed_ln(native):
    torch.manual_seed(7)
    V, P, H = 500, 64, 384
    word = torch.randn(V, H, device=DEV).bfloat16()
    pos = torch.randn(P, H, device=DEV).bfloat16()
    typ = torch.randn(1, H, device=DEV).bfloat16()
    g = torch.randn(H, device=DEV).bfloat16()
    b = torch.randn(H, device=DEV).bfloat16()
    ids = torch.randint(0, V, (20,), device=DEV, dtype=torch.int32)
    pids = torch.randint(0, P, (20,), device=DEV, dtype=torch.int32)
    y = native.embed_ln(ids, pids, word, pos, typ, g, b, 1e-12)
    h = word[ids.long()].float() + pos[pids.long()].float() + typ.float()
    ref = torch.nn.functional.layer_norm(h, (H,), g.float(), b.float(), 1e-12)
    assert rel_err(y, ref) < 1e-2


def test_rope_kv_write(native):
    torch.manual_seed(8)
    T, Hq, Hkv, D, BS = 70, 8, 2, 128, 64
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device=DEV).bfloat16()
    pos = torch.arange(T, dtype=torch.int32, device=DEV) + 5
    cos, sin = R.rope_tables(D, 1024, theta=500000.0,
                             scaling={"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                      "high_freq_factor": 4.0, "original_max_position_embeddings": 8192})
    kc = torch.zeros(4, Hkv, BS, D, device=DEV).bfloat16()
    vc = torch.zeros_like(kc)
    slots = torch.arange(T, dtype=torch.int32, device=DEV) + 64  # blocks 1..2
    orig = qkv.clone()
    native.rope_kv(qkv, pos, cos.to(DEV), sin.to(DEV), slots, kc, vc, Hq, Hkv, D)
    q = orig[:, :Hq * D].reshape(T, Hq, D).cpu()
    k = orig[:, Hq * D:(Hq + Hkv) * D].reshape(T, Hkv, D).cpu()
    v = orig[:, (Hq + Hkv) * D:].reshape(T, Hkv, D).cpu()
    q_ref = R.apply_rope(q, pos.long().cpu(), cos, sin)
    k_ref = R.apply_rope(k, pos.long().cpu(), cos, sin)
    assert torch.equal(qkv[:, :Hq * D].reshape(T, Hq, D).cpu(), q_ref)
    kc_c = kc.cpu()
    vc_c = vc.cpu()
    for t in range(T):
        s = t + 64
        assert torch.equal(kc_c[s // BS, :, s % BS], k_ref[t])
        assert torch.equal(vc_c[s // BS, :, s % BS], v[t])


@pytest.mark.parametrize("M,Hq,Hkv", [(2300, 32, 8), (4096, 32, 8), (1111, 4, 1)])
def test_gemm_rope_kv_bit_identical_to_gemm_then_rope_kv(native, M, Hq, Hkv):
    """The qkv projection with rope_kv's work in the gemm_w4 epilogue (EPI_ROPE_KV) vs gemm_w4 followed by
    rope_kv: the qkv rows (rotated q / k, plain v) and both paged caches bit-identical, ragged M tails
    (guarded edge tiles), rows without a cache slot (slot -1), llama3-scaled RoPE tables, positions out of
    order; TP=8-shard widths (4 q heads, 1 KV head)."""
    D, BS, K = 128, 64, 4096
    N = (Hq + 2 * Hkv) * D
    g = torch.Generator(device=DEV).manual_seed(M + Hq)
    x = (torch.randn(M, K, device=DEV, generator=g) * 0.5).bfloat16()
    w = (torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)).bfloat16()
    cos, sin = R.rope_tables(D, 16384, theta=500000.0,
                             scaling={"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                      "high_freq_factor": 4.0, "original_max_position_embeddings": 8192})
    cos, sin = cos.to(DEV), sin.to(DEV)
    pos = torch.randint(0, 16384, (M,), device=DEV, generator=g).int()
    nb = M // BS + 4
    slots = torch.randperm(nb * BS, device=DEV, generator=g)[:M].int()
    slots[::7] = -1
    kc = torch.zeros(nb, Hkv, BS, D, device=DEV).bfloat16()
    vc = torch.zeros_like(kc)
    assert native.gemm_rope_kv_ok(x, w, pos, cos, sin, slots, kc, vc, Hq, Hkv, D)
    got = native.gemm_rope_kv(x, w, pos, cos, sin, slots, kc, vc, Hq, Hkv, D)
    kc2, vc2 = torch.zeros_like(kc), torch.zeros_like(vc)
    ref = native.gemm(x, w)
    native.rope_kv(ref, pos, cos, sin, slots, kc2, vc2, Hq, Hkv, D)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
    assert int((kc != 0).sum().item()) > 0


def _paged_setup(lens, Hkv, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    nb_per = [(L + 63) // 64 for L in lens]
    total = sum(nb_per) + 3
    kc = torch.zeros(total, Hkv, 64, D).bfloat16()
    vc = torch.zeros_like(kc)
    perm = torch.randperm(total, generator=g)
    bts, i = [], 0
    maxb = max(nb_per)
    for L, nb in zip(lens, nb_per):
        blocks = perm[i:i + nb]
        i += nb
        bt = torch.zeros(maxb, dtype=torch.int32)
        bt[:nb] = blocks.int()
        bts.append(bt)
        kk = torch.randn(nb * 64, Hkv, D, generator=g)
        vv = torch.randn(nb * 64, Hkv, D, generator=g)
        kc[blocks] = kk.reshape(nb, 64, Hkv, D).permute(0, 2, 1, 3).bfloat16()
        vc[blocks] = vv.reshape(nb, 64, Hkv, D).permute(0, 2, 1, 3).bfloat16()
    return kc, vc, torch.stack(bts)


@pytest.mark.parametrize("q_lens,kv_lens,Hq,Hkv", [([37], [37], 8, 2), ([100, 64, 1], [100, 300, 129], 32, 8),
                                                   ([5, 70], [513, 70], 8, 1), ([1], [1], 4, 1),
                                                   ([64, 65], [64, 200], 4, 1),
                                                   ([2048, 1104], [4096, 5200], 32, 8)])
@pytest.mark.parametrize("big_cache", [False, True])
def test_attn_prefill_llama_kernels(native, q_lens, kv_lens, Hq, Hkv, big_cache):
    """The Llama prefill kernels vs the fp32 oracle on ragged query tails, chunked prefill (q_len <
    kv_len), single-tile sequences and 4 / 8 query heads per KV head: the software-pipelined 8-wave
    kernel (attn_prefill_v3_kernel, per-layer cache < 4 GiB: buffer-descriptor K/V staging) and, with a
    cache of >= 4 GiB per layer (big_cache: the same blocks placed at the top of an 8 GiB pair), the
    8-wave attn_prefill_kernel. 64-query tiles for 4 heads per block."""
    D = 128
    torch.manual_seed(19)
    kc, vc, bt = _paged_setup(kv_lens, Hkv, D)
    T = sum(q_lens)
    q = torch.randn(T, Hq * D).bfloat16()
    cu = torch.tensor([0] + list(torch.cumsum(torch.tensor(q_lens), 0)), dtype=torch.int32)
    kvl = torch.tensor(kv_lens, dtype=torch.int32)
    if big_cache:  # >= 4 GiB of blocks per cache: the kernel cannot address it with 32-bit buffer offsets
        nblk = -(-(4 << 30) // (Hkv * 64 * D * 2)) + kc.shape[0]
        off = nblk - kc.shape[0]
        kd = torch.empty((nblk, Hkv, 64, D), dtype=torch.bfloat16, device=DEV)
        vd = torch.empty_like(kd)
        kd[off:] = kc.to(DEV)
        vd[off:] = vc.to(DEV)
        btd = (bt + off).to(DEV)
    else:
        kd, vd, btd = kc.to(DEV), vc.to(DEV), bt.to(DEV)
    tiles = native.build_prefill_tiles(q_lens, Hq, Hkv)
    if (Hq // Hkv) % 4 == 0:
        assert (tiles[:, 1] % 64 == 0).all()
    out = torch.full((T, Hq * D), float("nan"), device=DEV).bfloat16()
    native.attn_prefill(q.to(DEV), kd, vd, cu.to(DEV), kvl.to(DEV), tiles.to(DEV), out, Hq, Hkv, D, causal=True,
                        paged=True, block_tables=btd)
    ref = R.attention_varlen(q.reshape(T, Hq, D), None, None, cu, kvl, True, 1 / math.sqrt(D),
                             k_full=lambda s: R.paged_kv_view(kc, bt[s], kv_lens[s], 64),
                             v_full=lambda s: R.paged_kv_view(vc, bt[s], kv_lens[s], 64))
    assert rel_err(out.cpu().reshape(T, Hq, D), ref) < 2e-2
    del kd, vd


@pytest.mark.parametrize("D,H", [(32, 12), (64, 16)])
def test_attn_encoder_contig(native, D, H):
    torch.manual_seed(10)
    lens = [7, 130, 64]
    T = sum(lens)
    qkv = torch.randn(T, 3 * H * D).bfloat16()
    cu = torch.tensor([0, 7, 137, 201], dtype=torch.int32)
    kvl = torch.tensor(lens, dtype=torch.int32)
    tiles = native.build_prefill_tiles(lens, H, H)
    out = torch.empty(T, H * D, device=DEV).bfloat16()
    g = qkv.to(DEV)
    native.attn_prefill(g, g[:, H * D:], g[:, 2 * H * D:], cu.to(DEV), kvl.to(DEV), tiles.to(DEV), out, H, H, D,
                        causal=False, paged=False, cu_kv=cu.to(DEV), kv_stride=3 * H * D)
    q = qkv[:, :H * D].reshape(T, H, D)
    k = qkv[:, H * D:2 * H * D].reshape(T, H, D)
    v = qkv[:, 2 * H * D:].reshape(T, H, D)
    ref = R.attention_varlen(q, k, v, cu, kvl, False, 1 / math.sqrt(D), cu_kv=cu)
    assert rel_err(out.cpu().reshape(T, H, D), ref) < 2e-2


@pytest.mark.parametrize("kv_lens,Hq,Hkv,target", [([1], 32, 8, 1024), ([65, 300, 4100], 32, 8, 1024),
                                                   ([777, 5], 32, 8, 8), ([200], 8, 8, 64),
                                                   # per-rank head layouts at TP=8: 8B (4, 1), 70B (8, 1); TP=4: (8, 2)
                                                   ([5200, 1, 64], 4, 1, 1024), ([65, 3000], 8, 1, 1024),
                                                   ([4100, 700], 8, 2, 256), ([1], 4, 1, 8)])
def test_attn_decode(native, kv_lens, Hq, Hkv, target):
    D = 128
    torch.manual_seed(11)
    kc, vc, bt = _paged_setup(kv_lens, Hkv, D, seed=3)
    B = len(kv_lens)
    q = torch.randn(B, Hq * D).bfloat16()
    kvl = torch.tensor(kv_lens, dtype=torch.int32)
    pt, mp = native.decode_partitions(max(kv_lens), B, Hkv, target_blocks=target)
    out = torch.empty(B, Hq * D, device=DEV).bfloat16()
    native.attn_decode(q.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV), kvl.to(DEV), out, Hq, Hkv, D, pt, mp)
    cu = torch.arange(B + 1, dtype=torch.int32)
    ref = R.attention_varlen(q.reshape(B, Hq, D), None, None, cu, kvl, True, 1 / math.sqrt(D),
                             k_full=lambda s: R.paged_kv_view(kc, bt[s], kv_lens[s], 64),
                             v_full=lambda s: R.paged_kv_view(vc, bt[s], kv_lens[s], 64))
    assert rel_err(out.cpu().reshape(B, Hq, D), ref) < 2e-2


@pytest.mark.parametrize("kv_lens,Hq,Hkv", [([5200, 1, 64, 4100], 32, 8), ([65, 3000, 700], 4, 1), ([1], 32, 8),
                                             ([8100] * 3 + [5], 32, 8)])
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("kl", [0, 1])
def test_attn_decode_nw8_single_partition(native, kv_lens, Hq, Hkv, nt, kl, monkeypatch):
    """Single-partition decode attention (the batch-32 grid: one block per sequence and KV head, no merge
    launch), as 8-wave blocks with K in registers (kl = 0) and as 4-wave blocks with K tiles by LDS-DMA (kl = 1,
    attention.hip KL, the default): vs the fp32 oracle and within rounding of the split-K kernel, nt loads or not."""
    monkeypatch.setattr(native, "DECODE_KL", bool(kl))
    D = 128
    torch.manual_seed(17)
    kc, vc, bt = _paged_setup(kv_lens, Hkv, D, seed=5)
    B = len(kv_lens)
    q = torch.randn(B, Hq * D).bfloat16()
    kvl = torch.tensor(kv_lens, dtype=torch.int32)
    args = (q.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV), kvl.to(DEV))
    pt4, mp4 = native.decode_partitions(max(kv_lens), B, Hkv, target_blocks=512)
    ref4 = torch.empty(B, Hq * D, device=DEV).bfloat16()
    native.attn_decode(*args, ref4, Hq, Hkv, D, pt4, mp4)
    monkeypatch.setattr(native, "DECODE_NW8_MIN_PAIRS", 1)
    monkeypatch.setattr(native, "DECODE_NT_MIN_BH", 1 if nt else 1 << 30)
    pt, mp = native.decode_partitions(max(kv_lens), B, Hkv)
    assert mp == 1
    out = torch.full((B, Hq * D), float("nan"), device=DEV).bfloat16()
    native.attn_decode(*args, out, Hq, Hkv, D, pt, mp)
    torch.cuda.synchronize()
    cu = torch.arange(B + 1, dtype=torch.int32)
    ref = R.attention_varlen(q.reshape(B, Hq, D), None, None, cu, kvl, True, 1 / math.sqrt(D),
                             k_full=lambda s: R.paged_kv_view(kc, bt[s], kv_lens[s], 64),
                             v_full=lambda s: R.paged_kv_view(vc, bt[s], kv_lens[s], 64))
    assert rel_err(out.cpu().reshape(B, Hq, D), ref) < 2e-2
    assert rel_err(out.cpu(), ref4.cpu()) < 1e-2


@pytest.mark.parametrize("kl", [0, 1])
def test_attn_decode_rope_single_partition_kl(native, kl, monkeypatch):
    """The engine's batch-32 decode attention (fused RoPE + KV append from the qkv slabs, single partition,
    nt): same cache contents as rope_kv_partials (bit for bit) and the same attention output within rounding
    for the 8-wave and the K-by-LDS-DMA 4-wave kernels; new tokens at a block end, a block start, alone."""
    monkeypatch.setattr(native, "DECODE_NW8_MIN_PAIRS", 1)
    monkeypatch.setattr(native, "DECODE_NT_MIN_BH", 1)
    D, S, Hq, Hkv = 128, 4, 32, 8
    kv_lens = [5200, 64, 65, 1, 3001, 4160]
    torch.manual_seed(15)
    kc, vc, bt = _paged_setup(kv_lens, Hkv, D, seed=6)
    B = len(kv_lens)
    kc, vc, bt = kc.to(DEV), vc.to(DEV), bt.to(DEV)
    kvl = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    pos = kvl - 1
    slots = (bt[torch.arange(B, device=DEV), (pos // 64).long()] * 64 + pos % 64).int()
    P = torch.randn(S, B, (Hq + 2 * Hkv) * D, device=DEV)
    cos, sin = R.rope_tables(D, 8192, theta=500000.0, scaling=None)
    cos, sin = cos.to(DEV), sin.to(DEV)
    pt, mp = native.decode_partitions(max(kv_lens), B, Hkv)
    assert mp == 1
    kc2, vc2 = kc.clone(), vc.clone()
    q = torch.empty(B, Hq * D, device=DEV).bfloat16()
    native.rope_kv_partials(P, q, pos, cos, sin, slots, kc2, vc2, Hq, Hkv, D)
    monkeypatch.setattr(native, "DECODE_KL", False)
    ref = torch.empty(B, Hq * D, device=DEV).bfloat16()
    native.attn_decode(q, kc2, vc2, bt, kvl, ref, Hq, Hkv, D, pt, mp)
    monkeypatch.setattr(native, "DECODE_KL", bool(kl))
    out = torch.full((B, Hq * D), float("nan"), device=DEV).bfloat16()
    native.attn_decode_rope(P, pos, cos, sin, slots, kc, vc, bt, kvl, out, Hq, Hkv, D, pt, mp)
    torch.cuda.synchronize()
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
    if kl:
        assert rel_err(out, ref) < 1e-2
    else:
        assert torch.equal(out, ref)
    cu = torch.arange(B + 1, dtype=torch.int32)
    qh = q.cpu().reshape(B, Hq, D)
    oracle = R.attention_varlen(qh, None, None, cu, kvl.cpu(), True, 1 / math.sqrt(D),
                                k_full=lambda s: R.paged_kv_view(kc.cpu(), bt.cpu()[s], kv_lens[s], 64),
                                v_full=lambda s: R.paged_kv_view(vc.cpu(), bt.cpu()[s], kv_lens[s], 64))
    assert rel_err(out.cpu().reshape(B, Hq, D), oracle) < 2e-2


@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (4, 1), (8, 1)])
@pytest.mark.parametrize("kv_lens,target", [([1], 1024), ([5200, 1, 64, 65, 3000, 700], 1024), ([777, 129], 8)])
def test_attn_decode_rope_matches_unfused(native, kv_lens, target, Hq, Hkv):
    """attn_decode_rope (q/k RoPE + KV append from the qkv partial slabs inside the attention kernel)
    == rope_kv_partials + attn_decode: same attention output and same cache contents, bit for bit
    (new token at the end of a block, at a block start, and as the only token), at the TP=1 heads and
    the per-rank heads of TP=8 (8B: 4 q / 1 kv, 70B: 8 / 1)."""
    D, S = 128, 8
    torch.manual_seed(14)
    kc, vc, bt = _paged_setup(kv_lens, Hkv, D, seed=5)
    B = len(kv_lens)
    kc, vc, bt = kc.to(DEV), vc.to(DEV), bt.to(DEV)
    kvl = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    pos = kvl - 1
    slots = (bt[torch.arange(B, device=DEV), (pos // 64).long()] * 64 + pos % 64).int()
    P = torch.randn(S, B, (Hq + 2 * Hkv) * D, device=DEV)
    cos, sin = R.rope_tables(D, 8192, theta=500000.0,
                             scaling={"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                      "high_freq_factor": 4.0, "original_max_position_embeddings": 8192})
    cos, sin = cos.to(DEV), sin.to(DEV)
    pt, mp = native.decode_partitions(max(kv_lens), B, Hkv, target_blocks=target)
    kc2, vc2 = kc.clone(), vc.clone()
    q = torch.empty(B, Hq * D, device=DEV).bfloat16()
    ref = torch.empty(B, Hq * D, device=DEV).bfloat16()
    native.rope_kv_partials(P, q, pos, cos, sin, slots, kc2, vc2, Hq, Hkv, D)
    native.attn_decode(q, kc2, vc2, bt, kvl, ref, Hq, Hkv, D, pt, mp)
    out = torch.empty(B, Hq * D, device=DEV).bfloat16()
    native.attn_decode_rope(P, pos, cos, sin, slots, kc, vc, bt, kvl, out, Hq, Hkv, D, pt, mp)
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
    assert torch.equal(out, ref)


def test_attn_decode_policy_does_not_outlive_its_call(native):
    """The launch policy of a decode-attention call is an argument of that call: a deferred-merge launch leaves
    nothing behind for the next one. 3 and 9 KV tiles over max_parts = 3 (sequence 0 takes one partition and is
    written by the partition kernel, sequence 1 takes three), plain / deferred / plain on identical inputs: the
    plain outputs and all three partition workspaces are equal bit for bit (the flag only drops the reduce
    launch); then attn_decode (no rope) after a deferred launch == the same call made before it."""
    D, S, Hq, Hkv = 128, 4, 8, 2
    kv_lens = [130, 517]
    torch.manual_seed(23)
    kc0, vc0, bt = _paged_setup(kv_lens, Hkv, D, seed=9)
    B = len(kv_lens)
    kc0, vc0, bt = kc0.to(DEV), vc0.to(DEV), bt.to(DEV)
    kvl = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    pos = kvl - 1
    slots = (bt[torch.arange(B, device=DEV), (pos // 64).long()] * 64 + pos % 64).int()
    P = torch.randn(S, B, (Hq + 2 * Hkv) * D, device=DEV)
    cos, sin = R.rope_tables(D, 8192, theta=500000.0, scaling=None)
    cos, sin = cos.to(DEV), sin.to(DEV)
    pt, mp = native.decode_partitions(640, B, Hkv)
    assert (pt, mp) == (4, 3)  # min(ceil(512 / 4), ceil(10 / 4)) partitions of at least 4 tiles

    def fresh():  # output and zeroed partition workspaces (single-partition rows leave theirs untouched)
        return (torch.zeros(B, Hq * D, device=DEV).bfloat16(),
                torch.zeros((B, Hq, mp, D), dtype=torch.float32, device=DEV),
                torch.zeros((B, Hq, mp, 2), dtype=torch.float32, device=DEV))

    # q rows and a cache that already holds the new token, for the no-rope calls
    kcq, vcq = kc0.clone(), vc0.clone()
    q = torch.empty(B, Hq * D, device=DEV).bfloat16()
    native.rope_kv_partials(P, q, pos, cos, sin, slots, kcq, vcq, Hq, Hkv, D)
    first = fresh()
    native.attn_decode(q, kcq, vcq, bt, kvl, first[0], Hq, Hkv, D, pt, mp, ws_o=first[1], ws_ml=first[2])

    runs = []
    for defer in (False, True, False):
        out, ws_o, ws_ml = fresh()
        native.attn_decode_rope(P, pos, cos, sin, slots, kc0.clone(), vc0.clone(), bt, kvl, out, Hq, Hkv, D, pt, mp,
                                ws_o=ws_o, ws_ml=ws_ml, defer_merge=defer)
        runs.append((out, ws_o, ws_ml))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[2][0])
    assert bool((runs[0][1][1] != 0).any())  # sequence 1's partition records were written
    for r in runs[1:]:
        assert torch.equal(r[1], runs[0][1]) and torch.equal(r[2], runs[0][2])
    # the deferred launch wrote sequence 0 (one partition) itself and left sequence 1's output row to the consumer
    assert torch.equal(runs[1][0][0], runs[0][0][0]) and not bool(runs[1][0][1].any())

    out, ws_o, ws_ml = fresh()
    native.attn_decode_rope(P, pos, cos, sin, slots, kc0.clone(), vc0.clone(), bt, kvl, out, Hq, Hkv, D, pt, mp,
                            ws_o=ws_o, ws_ml=ws_ml, defer_merge=True)
    after = fresh()
    native.attn_decode(q, kcq, vcq, bt, kvl, after[0], Hq, Hkv, D, pt, mp, ws_o=after[1], ws_ml=after[2])
    torch.cuda.synchronize()
    for x, y in zip(after, first):
        assert torch.equal(x, y)
    assert torch.equal(first[0], runs[0][0])  # and the fused launch == rope_kv_partials + attn_decode


def _part_ksteps_rule(M, N, K, min_blocks, legal=(32, 28, 16, 14, 8, 4)):
    """The slice rule of gemm_part.hip (ragk_gemm_part_ksteps), written out: the widest K-slice (64 * ks) that
    divides K, fits LDS in whole 8-wave DMA pieces and still gives min_blocks blocks, else the narrowest legal."""
    mt, nb = (M + 15) // 16, (N + 63) // 64
    ok = [ks for ks in legal if K % (64 * ks) == 0 and 16 * mt * 64 * ks * 2 <= 128 * 1024
          and (16 * mt * 64 * ks * 2) % 8192 == 0]
    for ks in ok:
        if nb * (K // (64 * ks)) >= min_blocks:
            return ks
    return ok[-1] if ok else 0


def test_gemm_part_slabs_follows_min_blocks_at_call_time(native, monkeypatch):
    """PART_MIN_BLOCKS is read on every gemm_part_slabs call (no launch here; the kernel library answers the
    host-side query): at (1, 4096, 4096) the legal slices are 32 / 16 / 8 / 4 steps, so a threshold of 1 picks
    the widest and one nothing reaches picks the narrowest, within one process. _silu_ks applies the same rule
    to its own legal set (16 / 8 / 4 steps) with the same constant."""
    M, N, K = 1, 4096, 4096
    assert (_part_ksteps_rule(M, N, K, 1), _part_ksteps_rule(M, N, K, 1 << 30)) == (32, 4)
    for mb in (1, 1 << 30, 512):
        monkeypatch.setattr(native, "PART_MIN_BLOCKS", mb)
        want = _part_ksteps_rule(M, N, K, mb)
        assert native.gemm_part_slabs(M, N, K) == (want, K // (64 * want)), mb
        silu = native._silu_ks(M, N, K)
        assert silu == _part_ksteps_rule(M, N, K, mb, legal=(16, 8, 4)), mb
        if want <= 16:  # a slice both may take: the two agree
            assert silu == want, mb


@pytest.mark.parametrize("M,N,K,ns", [(5207, 4096, 4096, 2), (5207, 4096, 14336, 2), (300, 4096, 4096, 4),
                                       (1000, 1024, 2048, 2), (256, 520, 1024, 4)])
def test_gemm_splitk_slabs(native, M, N, K, ns):
    """gemm_w4c KSPLIT (one persistent launch over ns K-slabs x tiles): slab z == x[:, z-th K range]
    @ w[:, z-th K range]^T in fp32, and the slab sum vs the fp32 oracle of the whole product."""
    torch.manual_seed(23)
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    P = native.gemm_splitk(x, w, ns)
    Ks = K // ns
    for z in (0, ns - 1):
        ref = x[:, z * Ks:(z + 1) * Ks].float() @ w[:, z * Ks:(z + 1) * Ks].float().t()
        assert rel_err(P[z].cpu(), ref.cpu()) < 1e-5, z
    assert rel_err(P.sum(0).cpu(), (x.float() @ w.float().t()).cpu()) < 1e-5


def _run_prefill_logits(m, T):
    from rag_llm_k8s_amd.models.llama import StepInput
    from rag_llm_k8s_amd.ops.backend import AttnMeta
    from rag_llm_k8s_amd.ops.native import build_prefill_tiles

    nb = (T + 63) // 64
    m.allocate_kv_cache(nb + 1)
    bt = torch.arange(1, nb + 1, dtype=torch.int32).view(1, nb)
    slots = torch.arange(64, 64 + T, dtype=torch.int32)
    meta = AttnMeta("prefill", torch.tensor([T], dtype=torch.int32).to(DEV), bt.to(DEV),
                    cu_q=torch.tensor([0, T], dtype=torch.int32).to(DEV),
                    tiles=build_prefill_tiles([T], 4, 1).to(DEV), host_kv_lens=[T])
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, m.cfg.vocab_size, (T,), generator=g, dtype=torch.int32)
    inp = StepInput(ids.to(DEV), torch.arange(T, dtype=torch.int32).to(DEV), slots.to(DEV), meta, None)
    return m.forward(inp).float().cpu()


def test_prefill_splitk_model_matches_resid_path(native):
    """Llama prefill with the split-K o_proj / down (fp32 slabs -> add_partials_rmsnorm) == the
    residual-epilogue path within bf16 rounding (one ~5k-token prompt at 8B widths, 2 layers)."""
    from rag_llm_k8s_amd.models import llama as L
    from rag_llm_k8s_amd.ops.backend import AttnMeta, NativeBackend  # noqa: F401

    cfg = L.llama31_8b()
    cfg.num_hidden_layers = 2
    cfg.vocab_size = 1024
    w = L.LlamaWeights.random(cfg, DEV, seed=3)
    m = L.LlamaModel(cfg, w, DEV, max_positions=8192)
    T = 5207
    assert native.prefill_nsplit(T, 4096, 4096) == 2 and native.prefill_nsplit(32768, 4096, 14336) == 1
    outs = []
    for split in (False, True):
        native.PREFILL_SPLITK = split
        try:
            outs.append(_run_prefill_logits(m, T))
        finally:
            native.PREFILL_SPLITK = True
    assert rel_err(outs[1], outs[0]) < 2e-2, rel_err(outs[1], outs[0])


@pytest.mark.parametrize("kv_lens,target,fp8,Hq,Hkv", [([5200], 512, False, 32, 8), ([70, 3000], 256, False, 32, 8),
                                                        ([5200, 64], 256, False, 32, 8),
                                                        ([777, 5300, 65, 2000], 512, False, 32, 8),
                                                        ([4100], 1024, True, 32, 8), ([8100], 512, False, 32, 8),
                                                        ([5200], 1024, False, 4, 1), ([5200, 70], 1024, False, 8, 1),
                                                        ([3000], 512, True, 4, 1)])
def test_gemm_part_merge_matches_reduce_then_part(native, kv_lens, target, fp8, Hq, Hkv):
    """o_proj fed by the UNMERGED split-K decode attention (attn_decode_rope with defer_merge, the
    partitions merged per K-slice inside gemm_part_merge) == attn_decode_rope (reduce launch) followed
    by gemm_part: same slabs up to fp32 summation order (bf16 activation may differ by 1 ulp), and vs an
    fp32 oracle of the attention output. Covers single-partition rows, mixed lengths, M = 1..4, fp8."""
    from rag_llm_k8s_amd.ops.fp8 import quantize_weight

    D, S = 128, 8
    torch.manual_seed(21)
    kc, vc, bt = _paged_setup(kv_lens, Hkv, D, seed=7)
    B = len(kv_lens)
    kc, vc, bt = kc.to(DEV), vc.to(DEV), bt.to(DEV)
    kvl = torch.tensor(kv_lens, dtype=torch.int32, device=DEV)
    pos = kvl - 1
    slots = (bt[torch.arange(B, device=DEV), (pos // 64).long()] * 64 + pos % 64).int()
    P = torch.randn(S, B, (Hq + 2 * Hkv) * D, device=DEV)
    cos, sin = R.rope_tables(D, 131072, theta=500000.0)
    cos, sin = cos.to(DEV), sin.to(DEV)
    pt, mp = native.decode_partitions(max(kv_lens), B, Hkv, target_blocks=target)
    assert mp > 1
    w = (torch.randn(4096, Hq * D, device=DEV) / math.sqrt(Hq * D)).bfloat16()
    wq = quantize_weight(w) if fp8 else w
    assert native.gemm_part_merge_ok(B, wq, Hq, mp, torch.empty(1))
    ws_o = torch.empty((B, Hq, mp, D), dtype=torch.float32, device=DEV)
    ws_ml = torch.empty((B, Hq, mp, 2), dtype=torch.float32, device=DEV)
    kc2, vc2 = kc.clone(), vc.clone()
    ref_attn = torch.empty(B, Hq * D, device=DEV).bfloat16()
    native.attn_decode_rope(P, pos, cos, sin, slots, kc2, vc2, bt, kvl, ref_attn, Hq, Hkv, D, pt, mp)
    ref = native.gemm_part(ref_attn, wq).sum(0)
    attn = torch.zeros(B, Hq * D, device=DEV).bfloat16()
    native.attn_decode_rope(P, pos, cos, sin, slots, kc, vc, bt, kvl, attn, Hq, Hkv, D, pt, mp, ws_o=ws_o,
                            ws_ml=ws_ml, defer_merge=True)
    out = native.gemm_part_merge(attn, kvl, pt, mp, ws_o, ws_ml, Hq, wq).sum(0)
    torch.cuda.synchronize()
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
    # the deferred launch leaves multi-partition rows of attn unwritten (zeros here)
    wd = wq.dequant() if fp8 else w.float()
    oracle = ref_attn.float() @ wd.t()
    assert rel_err(ref.cpu(), oracle.cpu()) < 1e-4
    assert rel_err(out.cpu(), oracle.cpu()) < 2e-3, rel_err(out.cpu(), oracle.cpu())


@pytest.mark.parametrize("M,N,K", [(1, 6144, 4096), (3, 6144, 4096), (4, 1280, 8192), (2, 10240, 8192)])
def test_gemm_part_norm_matches_rmsnorm_then_part(native, M, N, K):
    """gemm_part_norm (RMSNorm applied while staging the activation slice) == rmsnorm_kernel followed
    by gemm_part, bit for bit (same reduction order and rounding points)."""
    torch.manual_seed(15)
    h = (torch.randn(M, K, device=DEV) * 3).bfloat16()
    g = (1 + 0.1 * torch.randn(K, device=DEV)).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    out = native.gemm_part_norm(h, g, 1e-5, w)
    ref = native.gemm_part(native.rmsnorm(h, g, 1e-5), w, ks=K // (64 * out.shape[0]))  # same K-slices
    assert out.shape == ref.shape
    assert torch.equal(out, ref)


def test_pool_l2norm(native):
    torch.manual_seed(12)
    h = torch.randn(50, 384, device=DEV).bfloat16()
    cu = torch.tensor([0, 10, 11, 50], dtype=torch.int32, device=DEV)
    for mode in ["cls", "mean", "last"]:
        y = native.pool_l2norm(h, cu, mode=mode)
        ref = R.pool_l2norm(h.cpu(), cu.cpu(), mode=mode)
        assert rel_err(y.cpu(), ref) < 1e-3, mode
        assert torch.allclose(y.norm(dim=-1).cpu(), torch.ones(3), atol=1e-4)


def test_silu_mul(native):
    x = torch.randn(9, 2 * 512, device=DEV).bfloat16()
    y = native.silu_mul(x)
    ref = torch.nn.functional.silu(x[:, :512].float()) * x[:, 512:].float()
    assert rel_err(y, ref) < 1e-2


def test_topk_and_greedy(native):
    torch.manual_seed(13)
    B, V = 4, 128256
    logits = torch.randn(B, V, device=DEV) * 3
    cv, ci = native.topk_candidates(logits, 50)
    chunks = native.topk_chunks(V, 50)
    assert chunks > 1 and cv.shape == (B, chunks * 50)
    # each chunk's list is the exact sorted top-50 of its vocab slice
    Vc = ((V + chunks - 1) // chunks + 7) & ~7
    for c in range(chunks):
        sl = logits[:, c * Vc: min((c + 1) * Vc, V)]
        rv, ri = torch.topk(sl, 50, dim=-1)
        assert torch.allclose(cv[:, c * 50:(c + 1) * 50], rv)
        assert torch.equal(ci[:, c * 50:(c + 1) * 50].long(), ri + c * Vc)
    # merged, they contain the global top-50
    ref_v, ref_i = torch.topk(logits, 50, dim=-1)
    mv, order = torch.sort(cv, dim=-1, descending=True)
    assert torch.allclose(mv[:, :50], ref_v)
    assert torch.equal(torch.gather(ci, 1, order)[:, :50].long(), ref_i)
    # single-chunk path, vocab offset (TP shard) and short rows
    cv1, ci1 = native.topk_candidates(logits, 50, vocab_offset=1000, chunks=1)
    assert torch.allclose(cv1, ref_v) and torch.equal(ci1.long(), ref_i + 1000)
    short = logits[:, :37].contiguous()
    cvs, cis = native.topk_candidates(short, 50, chunks=3)
    assert cvs.shape == (B, 150)
    valid = cis >= 0
    assert int(valid.sum()) == B * 37
    assert torch.isinf(cvs[~valid]).all()
    temps = torch.zeros(B, device=DEV)
    ks = torch.full((B,), 50, dtype=torch.int32, device=DEV)
    ps = torch.full((B,), 0.9, device=DEV)
    seeds = torch.arange(B, dtype=torch.int64, device=DEV)
    steps = torch.zeros(B, dtype=torch.int32, device=DEV)
    tok = native.sample_candidates(cv, ci, temps, ks, ps, seeds, steps)
    assert torch.equal(tok.long(), logits.argmax(-1))


@pytest.mark.parametrize("V,K,chunks,topk", [(128256, 64, 7, 50), (4000, 50, 3, 50), (30000, 64, 16, 64),
                                              (37, 50, 3, 40), (128256, 64, 31, 50), (16032, 64, 4, 50),
                                              (20000, 50, 12, 50)])
def test_sample_list_merge_matches_sort(native, V, K, chunks, topk):
    """Rank-merging the sorted per-chunk candidate lists (top_k <= 64) samples exactly the same tokens
    as the full bitonic sort of all candidates: sampled (many seeds), greedy, and with -inf padding
    (a 37-entry row spread over 3 chunks of 50)."""
    torch.manual_seed(16)
    B = 64
    logits = (torch.randn(B, V, device=DEV) * 3).contiguous()
    logits[:, 5] = logits[:, 9]  # an exact tie across ids
    cv, ci = native.topk_candidates(logits, K, chunks=chunks)
    for temp in (0.7, 0.0):
        args = (torch.full((B,), temp, device=DEV), torch.full((B,), topk, dtype=torch.int32, device=DEV),
                torch.full((B,), 0.9, device=DEV), torch.arange(B, dtype=torch.int64, device=DEV) * 31 + 7,
                torch.arange(B, dtype=torch.int32, device=DEV))
        a = native.sample_candidates(cv, ci, *args)
        b = native.sample_candidates(cv, ci, *args, list_len=K)
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,V,chunks", [(1, 128256, 31), (4, 128256, 31), (3, 16032, 9), (2, 5000, 8), (2, 200, 9)])
def test_small_batch_topk_chunks_exact(native, B, V, chunks):
    """Small decode batches: many short chunks selected by the wave-network kernel -- each chunk's list is
    the exact sorted top-K of its slice (ties: lower id first), and the sampler's network merge of the
    lists equals the full sort."""
    torch.manual_seed(B * V)
    K = 64
    logits = (torch.randn(B, V, device=DEV) * 3).contiguous()
    logits[:, 7] = logits[:, 3]  # exact ties
    logits[:, 100:164] = logits[:, 100:101]  # a run of 64 equal values
    cv, ci = native.topk_candidates(logits, K, chunks=chunks)
    Vc = ((V + chunks - 1) // chunks + 7) & ~7
    n_valid = 0
    for c in range(chunks):
        sl = logits[:, c * Vc: min((c + 1) * Vc, V)].cpu()
        kk = min(K, sl.shape[1])
        if kk <= 0:
            continue
        n_valid += kk
        for b in range(B):  # reference order: value descending, index ascending
            idx = torch.from_numpy(np.lexsort((np.arange(sl.shape[1]), -sl[b].numpy())))
            assert torch.equal(ci[b, c * K:c * K + kk].cpu().long(), idx[:kk] + c * Vc), (b, c)
            assert torch.equal(cv[b, c * K:c * K + kk].cpu(), sl[b, idx[:kk]])
    valid = ci >= 0
    assert int(valid.sum()) == B * n_valid and bool(torch.isinf(cv[~valid]).all())
    for temp in (0.7, 0.0):
        args = (torch.full((B,), temp, device=DEV), torch.full((B,), 50, dtype=torch.int32, device=DEV),
                torch.full((B,), 0.9, device=DEV), torch.arange(B, dtype=torch.int64, device=DEV) * 3 + 1,
                torch.arange(B, dtype=torch.int32, device=DEV))
        a = native.sample_candidates(cv, ci, *args)
        b = native.sample_candidates(cv, ci, *args, list_len=K)
        assert torch.equal(a, b)


def test_sampling_support_matches_hf_rules(native):
    """Sampled tokens always lie in the HF temperature->top-k->top-p kept set, and the
    empirical distribution matches the renormalised kept probabilities."""
    torch.manual_seed(14)
    V = 1000
    logits = torch.randn(1, V) * 4
    kept, probs, _ = R.sample_from_logits(logits[0], 0.7, 50, 0.9)
    n = 4000
    L = logits.to(DEV).expand(n, V).contiguous()
    cv, ci = native.topk_candidates(L, 50)
    tok = native.sample_candidates(cv, ci, torch.full((n,), 0.7, device=DEV),
                                   torch.full((n,), 50, dtype=torch.int32, device=DEV),
                                   torch.full((n,), 0.9, device=DEV),
                                   torch.arange(n, dtype=torch.int64, device=DEV) * 7919 + 1,
                                   torch.zeros(n, dtype=torch.int32, device=DEV)).cpu().long()
    kept_set = set(kept.tolist())
    assert set(tok.tolist()) <= kept_set
    counts = torch.zeros(V)
    counts.index_add_(0, tok, torch.ones(n))
    emp = counts[kept] / n
    assert (emp - probs).abs().max().item() < 0.05


@pytest.mark.parametrize("N,d,nq,k", [(0, 64, 2, 5), (3, 64, 1, 5), (10000, 384, 32, 4), (5000, 1024, 3, 10),
                                      (70000, 128, 9, 8), (300000, 32, 3, 64), (1000, 100, 40, 1),
                                      (129, 384, 16, 64), (20000, 1024, 1, 5),
                                      # MFMA path (nq >= 16, k <= 8): 16 and 64 rows per wave, 1 / 2 query tiles
                                      (300000, 64, 33, 5), (5000, 1024, 16, 8), (777, 96, 70, 3)])
def test_l2_search(native, N, d, nq, k):
    torch.manual_seed(15)
    xb = torch.randn(N, d)
    q = torch.randn(nq, d)
    cap = max(N, 1) + 17
    xt = torch.zeros(d, cap, device=DEV)
    if N:
        native.l2_append(xt, cap, 0, xb.to(DEV))
    D, I = native.l2_search(xt, cap, N, q.to(DEV), k)
    Dr, Ir = R.l2_knn(xb, q, k)
    bad = I.cpu() != Ir
    # any order difference vs the fp64 reference must be a swap of (near-)equal distances
    assert bad.sum() <= 2 and (Dr[bad] - D.cpu()[bad]).abs().max().item() < 1e-3 if bad.any() else True
    assert torch.allclose(D.cpu(), Dr, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("N", [500, 100000])
def test_l2_search_ties_ids_map_and_row_range(native, N):
    """Exact ties (duplicated rows) come out in ascending id order, a row sub-range [row_begin, n)
    is honoured, ids are remapped through ids_map, and (-1, FLT_MAX) pads k > rows."""
    torch.manual_seed(3)
    d = 64
    base = torch.randn(N // 4, d)
    xb = base.repeat(4, 1)  # every vector 4 times: rows i, i + N/4, i + N/2, i + 3N/4
    cap = N + 5
    xt = torch.zeros(d, cap, device=DEV)
    native.l2_append(xt, cap, 0, xb.to(DEV))
    q = base[:7].clone()
    D, I = native.l2_search(xt, cap, N, q.to(DEV), 8)
    n4 = N // 4
    for j in range(7):
        assert I[j, :4].cpu().tolist() == [j, j + n4, j + 2 * n4, j + 3 * n4]
        assert float(D[j, :4].abs().max()) == 0.0
    ids = (torch.arange(cap, dtype=torch.int32) * 3 + 11).to(DEV)
    D2, I2 = native.l2_search(xt, cap, N, q.to(DEV), 8, row_begin=n4 + 1, ids_map=ids)
    assert I2[0, :3].cpu().tolist() == [(n4 * 2) * 3 + 11, (n4 * 3) * 3 + 11, I2[0, 2].item()]
    assert int(I2[1, 0]) == (n4 + 1) * 3 + 11
    D3, I3 = native.l2_search(xt, cap, 3, q[:2].to(DEV), 6)
    assert I3[:, 3:].eq(-1).all() and torch.all(D3[:, 3:] == torch.finfo(torch.float32).max)


def test_l2_search_mfma_path_matches_scan_path(native):
    """The batched-query MFMA path (||x||^2 + ||q||^2 - 2 x.q) and the direct-form scan agree: same ids
    up to swaps of near-equal distances, distances within fp32 rounding; exact duplicates come out in
    ascending id order on both."""
    torch.manual_seed(7)
    N, d, nq, k = 40000, 384, 32, 5
    base = torch.randn(N // 2, d)
    xb = torch.cat([base, base])  # row i and i + N/2 identical
    cap = N + 1
    xt = torch.zeros(d, cap, device=DEV)
    native.l2_append(xt, cap, 0, xb.to(DEV))
    q = (base[:nq] + 0.05 * torch.randn(nq, d)).to(DEV)
    Dm, Im = native.l2_search(xt, cap, N, q, k)
    native.l2_search_set_mfma_min_nq(10 ** 6)
    try:
        Ds, Is = native.l2_search(xt, cap, N, q, k)
    finally:
        native.l2_search_set_mfma_min_nq(16)
    assert torch.allclose(Dm.cpu(), Ds.cpu(), rtol=1e-4, atol=1e-2)
    for j in range(nq):  # nearest: the perturbed source row and its duplicate, lower id first
        assert Im[j, :2].tolist() == [j, j + N // 2] and Is[j, :2].tolist() == [j, j + N // 2]
    assert (Im == Is).float().mean() > 0.95


def test_l2_search_guard_canaries(native):
    """Outputs and partial-list buffers of the search are sized exactly: kernels write nothing past
    them (sentinel-padded allocations; SURVEY §5 OOB checks)."""
    torch.manual_seed(4)
    N, d, nq, k = 7777, 384, 5, 4
    cap = N + 3
    xt = torch.zeros(d, cap, device=DEV)
    native.l2_append(xt, cap, 0, torch.randn(N, d, device=DEV))
    L = native._lib.lib()
    G = L.ragk_l2_search_groups(0, N, nq, k, d)
    pad = 4096
    q = torch.randn(nq, d, device=DEV)
    bufs = [torch.full((2 * pad + n,), -7.0, device=DEV) for n in (nq * G * k, nq * k)]
    ibufs = [torch.full((2 * pad + n,), -7, dtype=dt, device=DEV)
             for n, dt in zip((nq * G * k, nq * k), (torch.int32, torch.int64))]
    views = [b[pad:pad + n] for b, n in zip(bufs, (nq * G * k, nq * k))]
    iviews = [b[pad:pad + n] for b, n in zip(ibufs, (nq * G * k, nq * k))]
    native.check(L.ragk_l2_search(xt.data_ptr(), cap, d, 0, N, q.data_ptr(), nq, k, None, views[0].data_ptr(),
                                  iviews[0].data_ptr(), views[1].data_ptr(), iviews[1].data_ptr(),
                                  native.stream_ptr()), "ragk_l2_search")
    torch.cuda.synchronize()
    for b, ib in zip(bufs, ibufs):
        assert b[:pad].eq(-7.0).all() and b[-pad:].eq(-7.0).all()
        assert ib[:pad].eq(-7).all() and ib[-pad:].eq(-7).all()
    Dr, Ir = R.l2_knn(xt[:, :N].t().cpu(), q.cpu(), k)
    assert torch.equal(iviews[1].view(nq, k).cpu(), Ir)  # int64 ids straight from the merge kernel


@pytest.mark.parametrize("M", [1, 7, 16, 33, 64])
@pytest.mark.parametrize("N,K", [(768, 1024), (4096, 4096), (6144, 4096), (1024, 14336)])
def test_gemm_stream_bf16(native, M, N, K):
    torch.manual_seed(M * 7 + N)
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    r = torch.randn(M, N, device=DEV).bfloat16()
    b = torch.randn(N, device=DEV).bfloat16()
    ref = x.float() @ w.float().t()
    for _ in range(2):  # second call: split-K counters were reset
        assert rel_err(native.gemm(x, w, path=5), ref) < 1e-2
    assert rel_err(native.gemm(x, w, resid=r, epi="resid", path=5), ref + r.float()) < 1e-2
    assert rel_err(native.gemm(x, w, bias=b, epi="bias_gelu", path=5),
                   torch.nn.functional.gelu(ref + b.float())) < 1e-2
    assert rel_err(native.gemm(x, w, out_f32=True, path=5), ref) < 1e-3
    if N % 128 == 0:
        g, u = w[: N // 2], w[N // 2:]
        y = native.gemm(x, R.pack_gate_up(g, u), epi="silu_mul", path=5)
        ref2 = torch.nn.functional.silu(x.float() @ g.float().t()) * (x.float() @ u.float().t())
        assert rel_err(y, ref2) < 1e-2
        # 128-row tiles (one block per CU) == 64-row pair tiles (two per CU): same k order per output
        L = native._lib.lib()
        try:
            L.ragk_gemm_stream_set_pair_rows(128)
            y128 = native.gemm(x, R.pack_gate_up(g, u), epi="silu_mul", path=5)
        finally:
            L.ragk_gemm_stream_set_pair_rows(64)
        assert torch.equal(y, y128)


@pytest.mark.parametrize("M", [1, 7, 16, 32, 33, 64])
@pytest.mark.parametrize("N,K", [(4096, 4096), (6144, 4096), (4096, 14336), (384, 512), (1000, 1024),
                                 (4096, 1792), (768, 4096), (4096, 512)])  # TP=8 shard down / qkv / o_proj
def test_gemm_part(native, M, N, K, monkeypatch):
    """Decode GEMM v5: fp32 split-K partial slabs sum to x @ w^T (the register-streaming kernel itself;
    the stream GEMM's slab mode, which gemm_part dispatches to from batch 5, has its own test)."""
    monkeypatch.setattr(native, "STREAM_PART", False)
    torch.manual_seed(3)
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    ks, S = native.gemm_part_slabs(M, N, K)
    if S == 0:
        pytest.skip("shape not supported by gemm_part")
    P = native.gemm_part(x, w)
    assert P.shape == (S, M, N)
    assert rel_err(P.sum(0), x.float() @ w.float().t()) < 2e-3


@pytest.mark.parametrize("M", [17, 32])
def test_gemm_vocab_stream_route(native, M):
    """Vocab-sized projections above batch 16 run on the stream GEMM (non-temporal weights, fp32 logits):
    same values as the gemm_dec path within fp32 summation order, and vs an fp32 oracle."""
    torch.manual_seed(M)
    N, K = 65536 + 64, 1024
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    assert native.use_stream(M, N, K, "none")
    y = native.gemm(x, w, out_f32=True)
    ref = x.float() @ w.float().t()
    assert rel_err(y, ref) < 1e-3
    assert rel_err(y, native.gemm(x, w, out_f32=True, path=4)) < 1e-4
    assert not native.use_stream(16, N, K, "none")


@pytest.mark.parametrize("M", [5, 8, 16, 17, 32, 64])
@pytest.mark.parametrize("N,K", [(4096, 4096), (6144, 4096), (4096, 14336), (1000, 1024), (4096, 1792)])
@pytest.mark.parametrize("rows", [None, 64])
def test_gemm_stream_part(native, M, N, K, rows):
    """Split-K slabs from the LDS-DMA stream GEMM (gemm_stream.hip SLAB): P.sum(0) = x @ w^T, [S, M, N].
    M = 5..16 is the one-row-tile instantiation (activation rows padded below 16) that decode batches
    from STREAM_PART_MIN_M up take by default."""
    torch.manual_seed(M + N)
    x = torch.randn(M, K, device=DEV).bfloat16()
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16()
    r, S = native.stream_part_cfg(M, N, K)
    # shapes the policy leaves on gemm_part (grid under half the CUs) still run correctly with an explicit split
    P = native.gemm_stream_part(x, w, rows=rows or r or 128, S=S or 2)
    assert P.shape[1:] == (M, N) and (K // 64) % P.shape[0] == 0
    assert rel_err(P.sum(0), x.float() @ w.float().t()) < 2e-3
    if rows is None:  # the register-streaming gemm_part that the slabs replace agrees
        old = native.STREAM_PART
        native.STREAM_PART = False
        try:
            Q = native.gemm_part(x, w)
        finally:
            native.STREAM_PART = old
        assert rel_err(P.sum(0), Q.sum(0)) < 1e-4


@pytest.mark.parametrize("M", [1, 2, 4])
@pytest.mark.parametrize("I,H", [(1792, 4096), (3584, 4096), (7168, 4096), (3584, 8192), (14336, 4096)])
def test_gemm_part_silu(native, M, I, H):
    """Down partials fed by the packed gate/up partial slabs: P.sum(0) = bf16(silu(g) * u) @ w_down^T,
    g / u = the slab sums (TP shard shapes: I = 14336 / TP, 70B H = 8192)."""
    torch.manual_seed(M + I)
    x = torch.randn(M, H, device=DEV).bfloat16()
    wgu = (torch.randn(2 * I, H, device=DEV) / math.sqrt(H)).bfloat16()
    wd = (torch.randn(H, I, device=DEV) / math.sqrt(I)).bfloat16()
    assert native.gemm_part_silu_ok(M, wgu, wd)
    pgu = native.gemm_part_gu(x, wgu)
    assert pgu.shape[0] <= native.SILU_MAX_SLABS and pgu.shape[1:] == (M, 2 * I)
    assert rel_err(pgu.sum(0), x.float() @ wgu.float().t()) < 2e-3
    P = native.gemm_part_silu(pgu, wd)
    gu = pgu.sum(0).view(M, I // 64, 2, 64)
    a = (torch.nn.functional.silu(gu[:, :, 0]) * gu[:, :, 1]).reshape(M, I).bfloat16()
    assert rel_err(P.sum(0), a.float() @ wd.float().t()) < 2e-3
    ref = R.linear(x.float().cpu(), wgu.float().cpu(), None, None, epi="silu_mul").bfloat16().float() @ wd.float().cpu().t()
    assert rel_err(P.sum(0).cpu(), ref) < 1e-2


@pytest.mark.parametrize("S,M,H", [(1, 3, 384), (4, 32, 4096), (7, 17, 4096), (9, 32, 4096), (16, 5, 4096)])
def test_add_partials_rmsnorm(native, S, M, H):
    """Split-K consumer: h <- bf16(h + bf16(sum P)), out = rmsnorm(h) (bit-exact with the torch oracle
    for h; the norm within bf16 rounding)."""
    torch.manual_seed(11)
    P = torch.randn(S, M, H, device=DEV)
    h = torch.randn(M, H, device=DEV).bfloat16()
    w = torch.randn(H, device=DEV).bfloat16()
    h_ref = (h.cpu().float() + P.cpu().sum(0).bfloat16().float()).bfloat16()
    ref = R.rmsnorm(h_ref, w.cpu(), 1e-5)
    y = native.add_partials_rmsnorm(P, h, w, 1e-5)
    # fp32 slab sums may differ in the last ulp from torch's order -> rare 1-ulp bf16 flips
    assert (h.cpu().float() - h_ref.float()).abs().max().item() <= 0.0625
    assert rel_err(h.cpu(), h_ref) < 1e-3
    assert rel_err(y.cpu(), ref) < 4e-3


@pytest.mark.parametrize("S,T", [(4, 33), (9, 32), (16, 1)])  # S > 8: more than one unrolled slab group
def test_rope_kv_partials(native, S, T):
    torch.manual_seed(12)
    Hq, Hkv, D, BS = 8, 2, 128, 64
    W = (Hq + 2 * Hkv) * D
    P = torch.randn(S, T, W, device=DEV)
    pos = torch.arange(T, dtype=torch.int32, device=DEV) + 7
    cos, sin = R.rope_tables(D, 1024, theta=500000.0,
                             scaling={"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                      "high_freq_factor": 4.0, "original_max_position_embeddings": 8192})
    cos, sin = cos.to(DEV), sin.to(DEV)
    slots = torch.arange(T, dtype=torch.int32, device=DEV) + 64
    kc = torch.zeros(4, Hkv, BS, D, device=DEV).bfloat16()
    vc = torch.zeros_like(kc)
    q = torch.zeros(T, Hq * D, device=DEV).bfloat16()
    native.rope_kv_partials(P, q, pos, cos, sin, slots, kc, vc, Hq, Hkv, D)
    # oracle: plain rope_kv on the bf16-rounded sum
    qkv = P.sum(0).bfloat16()
    kc2, vc2 = torch.zeros_like(kc), torch.zeros_like(vc)
    native.rope_kv(qkv, pos, cos, sin, slots, kc2, vc2, Hq, Hkv, D)
    assert rel_err(q, qkv[:, :Hq * D]) < 1e-3
    assert rel_err(kc, kc2) < 1e-3 and rel_err(vc, vc2) < 1e-3
