"""OCP MXFP4 weights on the CPU: the format (ops/mxfp4.py), its quantizer, the fp32 oracle of the GPU kernels
and the model / config plumbing of DTYPE=mxfp4."""
import math

import pytest
import torch

from rag_llm_k8s_amd.ops import mxfp4 as F4


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _weight(codes, scales):
    """codes [rows, K] nibble codes in k order, scales [rows, K/32] bytes -> Mxfp4Weight."""
    c = torch.tensor(codes, dtype=torch.uint8)
    c = c.reshape(c.shape[0], -1, 2)
    return F4.Mxfp4Weight(c[:, :, 0] | (c[:, :, 1] << 4), torch.tensor(scales, dtype=torch.uint8))


def test_dequant_fixed_codes():
    # block 0 (byte 127 = 2^0): every code once, low / high nibbles alternating; block 1: byte 129 = 4x;
    # block 2: byte 1 = 2^-126 (smallest); block 3: byte 254 = 2^127 (largest)
    codes = [list(range(16)) * 2 + [1, 9, 7, 15] + [0] * 28 + [1, 2, 10] + [0] * 29 + [1, 2, 10] + [0] * 29]
    w = _weight(codes, [[127, 129, 1, 254]])
    assert w.shape == (1, 128) and w.nbytes() == 64 + 4
    assert w.packed[0, 0].item() == 0x10 and w.packed[0, 7].item() == 0xFE  # k even -> low nibble
    d = w.dequant()[0]
    lut = [0, 0.5, 1, 1.5, 2, 3, 4, 6]
    assert d[:16].tolist() == lut + [-v for v in lut]
    assert d[16:32].tolist() == d[:16].tolist()
    assert d[32:36].tolist() == [2.0, -2.0, 24.0, -24.0]
    assert d[64:67].tolist() == [2.0 ** -127, 2.0 ** -126, -(2.0 ** -126)]
    assert d[96].item() == 2.0 ** 126 and d[97].item() == 2.0 ** 127 and d[98].item() == -(2.0 ** 127)
    # exact in bf16 (where bf16 has the range: everything but the 2^-127 subnormal scale product is normal)
    assert torch.equal(w.dequant(torch.bfloat16)[0, :64].float(), d[:64])


def test_quantize_zero_block_saturation_and_rounding():
    w = torch.zeros(2, 128)
    w[0, 32] = 7.5  # amax 7.5: e = floor(log2 7.5) - 2 = 0, 7.5 / 1 in (6, 8) saturates at 6
    w[0, 33:40] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])  # ties -> even code
    w[0, 40:44] = torch.tensor([-0.26, -2.6, 5.1, -7.0])
    w[1, 64] = -3.0 * 2.0 ** -20  # e = -19 - 2
    q = F4.quantize_weight(w)
    assert q.scale[0].tolist() == [127, 127, 127, 127]  # all-zero blocks: e = 0
    assert q.scale[1].tolist() == [127, 127, 127 - 21, 127]
    d = q.dequant()
    assert d[0, :32].abs().max().item() == 0 and q.packed[0, :16].eq(0).all()
    assert d[0, 32:44].tolist() == [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, -0.5, -3.0, 6.0, -6.0]
    assert d[1, 64].item() == -3.0 * 2.0 ** -20  # 6 * 2^-21
    assert int(q.scale.min()) >= 1 and int(q.scale.max()) <= 254


@pytest.mark.parametrize("N,K", [(768, 1024), (4096, 4096)])
def test_quantize_error_and_idempotence(N, K):
    torch.manual_seed(N)
    w = (torch.randn(N, K) / math.sqrt(K)).bfloat16()
    q = F4.quantize_weight(w)
    assert q.packed.shape == (N, K // 2) and q.scale.shape == (N, K // 32) and q.shape == (N, K)
    assert q.nbytes() * 8 == N * K * 4.25
    e = rel_err(q.dequant(), w)
    print("mxfp4 weight error (%d,%d): %.4f" % (N, K, e))
    assert e < 0.13  # e2m1 with a power-of-two block scale on Gaussian data: 0.115
    q2 = F4.quantize_weight(q.dequant(torch.bfloat16))
    assert torch.equal(q2.packed, q.packed) and torch.equal(q2.scale, q.scale)


@pytest.mark.parametrize("N,K", [(768, 1024), (4096, 4096)])
def test_reference_linear_close_to_bf16(N, K):
    """W4A16 (M = 10) and W4A8 (M = 100) against the bf16 product: measured 0.114-0.118 with these seeds; the
    weight error (0.115) dominates, the e4m3 activations add ~0.025 in quadrature. Bound: 15 % margin."""
    torch.manual_seed(N + 1)
    w = (torch.randn(N, K) / math.sqrt(K)).bfloat16()
    q = F4.quantize_weight(w)
    x = torch.randn(100, K).bfloat16()
    for M in (10, 100):
        e = rel_err(F4.reference_linear(x[:M], q, out_f32=True), x[:M].float() @ w.float().t())
        print("mxfp4 linear error (%d,%d) M=%d: %.4f" % (N, K, M, e))
        assert e < 0.135
    b = torch.randn(N).bfloat16()
    y = F4.reference_linear(x[:3], q, bias=b, epi="bias")
    assert y.dtype == torch.bfloat16 and rel_err(y, x[:3].float() @ q.dequant().t() + b.float()) < 1e-2


def test_row_parallel_k_slice_commutes():
    torch.manual_seed(2)
    w = (torch.randn(64, 1024) * 0.05).bfloat16()
    full = F4.quantize_weight(w)
    for lo, hi in ((0, 384), (384, 1024)):  # multiples of 128: MX blocks never straddle a shard
        part = F4.quantize_weight(w[:, lo:hi].contiguous())
        assert torch.equal(part.packed, full.packed[:, lo // 2:hi // 2])
        assert torch.equal(part.scale, full.scale[:, lo // 32:hi // 32])


def test_k_not_multiple_of_128_raises():
    with pytest.raises(ValueError, match="128"):
        F4.quantize_weight(torch.randn(8, 192))
    with pytest.raises(ValueError, match="128"):
        F4.quantize_weight(torch.randn(8, 32))


def _prefill_logits(model, ids):
    from rag_llm_k8s_amd.models.llama import StepInput
    from rag_llm_k8s_amd.ops.backend import AttnMeta

    n = len(ids)
    model.allocate_kv_cache(4)
    bt = torch.tensor([[1, 2, 0, 0]], dtype=torch.int32)
    meta = AttnMeta("prefill", torch.tensor([n], dtype=torch.int32), bt, cu_q=torch.tensor([0, n], dtype=torch.int32),
                    host_kv_lens=[n], host_q_lens=[n])
    return model.forward(StepInput(torch.tensor(ids, dtype=torch.int32), torch.arange(n, dtype=torch.int32),
                                   torch.arange(64, 64 + n, dtype=torch.int32), meta, None))


def test_quantize_mxfp4_model_close_to_bf16():
    """The tiny random model of test_fp8_weights_cpu_reference_close_to_bf16: a random-init model is the worst
    case for a 4-bit format (no outlier structure to exploit); measured 0.37-0.38 here, fp8 gives 0.09-0.12."""
    from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights, llama_tiny
    from rag_llm_k8s_amd.utils.synthetic import llama_state_dict

    cfg = llama_tiny(vocab=512, layers=2, hidden=256, heads=4, kv_heads=2, inter=512)
    sd = llama_state_dict(cfg, seed=1, std=0.05)
    w16 = LlamaWeights.from_state_dict(cfg, sd, "cpu")
    w8 = LlamaWeights.from_state_dict(cfg, sd, "cpu").quantize_fp8()
    w4 = LlamaWeights.from_state_dict(cfg, sd, "cpu").quantize_mxfp4()
    assert w4.dtype == "mxfp4"
    for L in w4.layers:
        assert all(isinstance(L[k], F4.Mxfp4Weight) for k in ("wqkv", "wo", "wgu", "wdown"))
        assert L["ln_in"].dtype == torch.bfloat16
    assert w4.lm_head.dtype == torch.bfloat16 and w4.embed.dtype == torch.bfloat16
    assert w4.nbytes() < w8.nbytes() < w16.nbytes()
    lin = sum(v.numel() * 2 for L in w16.layers for k, v in L.items() if k.startswith("w"))
    assert w16.nbytes() - w4.nbytes() == lin - lin * 4.25 / 16
    l16 = _prefill_logits(LlamaModel(cfg, w16, "cpu", max_positions=512), list(range(1, 90)))
    l4 = _prefill_logits(LlamaModel(cfg, w4, "cpu", max_positions=512), list(range(1, 90)))
    e = rel_err(l4, l16)
    print("mxfp4 tiny-model prefill logits vs bf16: %.4f" % e)
    assert e < 0.45
    # TP shards: quantized after slicing, row-parallel K shards are multiples of 128
    s0 = LlamaWeights.from_state_dict(cfg, sd, "cpu", tp_rank=1, tp_size=2).quantize_mxfp4()
    assert s0.layers[0]["wo"].shape == (256, 128) and s0.layers[0]["wdown"].shape == (256, 256)
    assert torch.equal(s0.layers[0]["wdown"].packed, w4.layers[0]["wdown"].packed[:, 128:])


def test_backend_gates_refuse_mxfp4():
    from rag_llm_k8s_amd.ops.backend import AttnMeta, TorchBackend

    be = TorchBackend()
    be.enable_part = True
    w = F4.quantize_weight(torch.randn(256, 256).bfloat16())
    bf = torch.randn(256, 256).bfloat16()
    assert be.part_ok(1, bf) and not be.part_ok(1, w)
    assert not be.part_norm_ok(1, w) and not be.part_silu_ok(1, w, w) and not be.mlp_engine_ok(1, w, w)
    assert not be.part_merge_ok(1, AttnMeta("decode", None, None), w, 2, 128) and be.prefill_nsplit(5000, w) == 1
    x = torch.randn(3, 256).bfloat16()
    assert torch.equal(be.gemm_part(x, w)[0], x.float() @ w.dequant().t())
    assert torch.equal(be.gemm(x, w), F4.reference_linear(x, w))


def test_config_and_builder_accept_mxfp4(tmp_path, monkeypatch):
    import json

    from rag_llm_k8s_amd.config import RagConfig
    from rag_llm_k8s_amd.server import builder

    monkeypatch.setenv("DTYPE", "mxfp4")
    cfg = RagConfig.from_env()
    assert cfg.dtype == "mxfp4"
    # a GPT-2 checkpoint has no MXFP4 path: refuse instead of silently serving bf16
    (tmp_path / "config.json").write_text(json.dumps({"model_type": "gpt2"}))
    cfg.model_path = str(tmp_path)
    with pytest.raises(ValueError, match="mxfp4"):
        builder.build_generator(cfg, "cpu")
