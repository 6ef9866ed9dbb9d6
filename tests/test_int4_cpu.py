"""4-bit integer weights on the CPU: the container and its AWQ / GPTQ unpackers (ops/int4.py), the quantizer, the
fp32 oracle of the GPU routes and the model / config / builder plumbing of DTYPE=int4."""
import json

import pytest
import torch

from int4_cases import pack_awq, pack_gptq, random_params
from rag_llm_k8s_amd.ops import int4 as I4

PACK = {"awq": (pack_awq, I4.unpack_awq, (0, 15)), "gptq": (pack_gptq, I4.unpack_gptq, (1, 16))}  # zero range


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _formula(codes, zeros, scales, G=128):
    return scales.double().repeat_interleave(G, 1) * (codes.double() - zeros.double().repeat_interleave(G, 1))


@pytest.mark.parametrize("N,K", [(16, 128), (24, 384)])
@pytest.mark.parametrize("fmt", ["awq", "gptq"])
def test_unpack_matches_formula_and_k_shard(fmt, N, K):
    pack, unpack, (zlo, zhi) = PACK[fmt]
    codes, zeros, scales = random_params(N, K, seed=N + K, zlo=zlo, zhi=zhi)
    t = pack(codes, zeros, scales)
    w = unpack(**t)
    assert w.shape == (N, K) and w.packed.dtype == torch.uint8 and w.meta.dtype == torch.int32
    assert w.nbytes() * 8 == N * K * 4.25
    assert torch.equal(w.codes(), codes) and torch.equal(w.zeros(), zeros.int()) and torch.equal(w.scales(), scales)
    assert torch.equal(w.dequant(torch.float64), _formula(codes, zeros, scales))
    if K > 128:
        part = unpack(**t, k_range=(128, K))
        assert torch.equal(part.packed, w.packed[:, 64:]) and torch.equal(part.meta, w.meta[:, 1:])
        assert torch.equal(part.packed, w.slice(cols=(128, K)).packed)
    # per-channel scales: one group of K, the meta word repeated per 128
    c1, z1, s1 = random_params(N, K, seed=7, G=K, zlo=1, zhi=15)
    w1 = unpack(**pack(c1, z1, s1))
    assert w1.meta.shape == (N, K // 128) and torch.equal(w1.dequant(torch.float64), _formula(c1, z1, s1, G=K))


def test_unsupported_checkpoints_are_refused():
    codes, zeros, scales = random_params(16, 128, seed=1, G=64, zlo=1, zhi=15)
    for pack, unpack, _ in PACK.values():
        with pytest.raises(ValueError, match="group_size"):
            unpack(**pack(codes, zeros, scales))
    c, z, s = random_params(16, 256, seed=2, zlo=1, zhi=15)
    t = pack_gptq(c, z, s)
    t["g_idx"] = t["g_idx"].flip(0)
    with pytest.raises(ValueError, match="g_idx"):
        I4.unpack_gptq(**t)
    ok = {"quant_method": "gptq", "bits": 4, "group_size": 128, "desc_act": False}
    assert I4.check_quant_config(ok) == "gptq"
    assert I4.check_quant_config({"quant_method": "awq", "bits": 4, "group_size": -1, "version": "gemm",
                                  "zero_point": True}) == "awq"
    for bad, why in [({"group_size": 64}, "group_size"), ({"desc_act": True}, "desc_act"), ({"bits": 8}, "bits"),
                     ({"quant_method": "awq", "version": "gemv"}, "gemm"), ({"quant_method": "bnb"}, "awq or gptq")]:
        with pytest.raises(ValueError, match=why):
            I4.check_quant_config(dict(ok, **bad))


def test_quantize_hand_computed_and_constant_groups():
    w = torch.zeros(3, 128)
    w[0, :16] = torch.arange(16) * 0.5 - 2.0  # min -2, max 5.5: scale 0.5, zero 4, codes 0..15
    w[0, 16:] = 1.3  # 1.3 / 0.5 = 2.6 -> 3, + 4
    w[1] = 3.7  # all equal: scale 1, zero 0 (round(-3.7) clamps), code 4
    q = I4.quantize_weight(w)
    assert q.scales()[:, 0].tolist() == [0.5, 1.0, 1.0] and q.zeros()[:, 0].tolist() == [4, 0, 0]
    assert q.codes()[0, :17].tolist() == list(range(16)) + [7]
    assert q.codes()[1].eq(4).all() and q.codes()[2].eq(0).all() and q.dequant()[2].eq(0).all()
    assert q.packed[0, :4].tolist() == [0x40, 0x51, 0x62, 0x73]  # byte j: code k0 + j | code k0 + 4 + j << 4
    assert q.meta[0, 0].item() == 0x3800 | (4 << 16)
    with pytest.raises(ValueError, match="128"):
        I4.quantize_weight(torch.randn(8, 192))


def test_quantize_error_bound_and_idempotence():
    torch.manual_seed(0)
    w = (torch.randn(48, 384) * 0.05).bfloat16()
    q = I4.quantize_weight(w)
    s = q.scales().double().repeat_interleave(128, 1)
    # half a step, plus the fp16 rounding of the scale (relative 2^-11) over the 15 steps of the range
    assert bool(((w.double() - q.dequant(torch.float64)).abs() <= s / 2 + 15 * s * 2.0 ** -11).all())
    # A container whose groups all hold a code 0 and a code 15 quantizes to itself: max - min = 15 s and -min = z s
    # are exact in fp32, so the scale, the zero and every code come back. (A group of rounded weights whose codes
    # stop at 14 -- about one in 150 here -- gets the scale 14/15 s the second time: the formulas' doing.)
    codes, zeros, scales = random_params(48, 384, seed=5, zlo=0, zhi=15)
    codes[:, 0::128], codes[:, 1::128] = 0, 15
    q = I4.Int4Weight.from_codes(codes, scales, zeros)
    q2 = I4.quantize_weight(q.dequant())
    assert torch.equal(q2.packed, q.packed) and torch.equal(q2.meta, q.meta)


@pytest.mark.parametrize("M", [10, 100])
def test_reference_linear_exact_on_integers(M):
    """Integer activations, power-of-two scales: every product and sum is exact in fp32 (and the dequantized
    weights exact in bf16), so both M regimes equal the float64 product bit for bit."""
    codes, zeros, scales = random_params(24, 384, seed=M, pow2=True)
    w = I4.Int4Weight.from_codes(codes, scales, zeros)
    x = torch.randint(-4, 5, (M, 384), generator=torch.Generator().manual_seed(M)).bfloat16()
    ref = x.double() @ _formula(codes, zeros, scales).t()
    assert torch.equal(I4.reference_linear(x, w, out_f32=True), ref.float())
    r = torch.randint(-8, 9, (M, 24)).bfloat16()
    assert torch.equal(I4.reference_linear(x, w, resid=r, epi="resid"), (ref + r.double()).bfloat16())


LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj",
           "mlp.up_proj", "mlp.down_proj")


def _quantized_state_dicts(cfg, seed=3):
    """One set of random codes / zeros (1..15: both formats can store them) / scales per projection, packed
    as AWQ and as GPTQ, plus the state dict of the dequantized fp32 weights."""
    from rag_llm_k8s_amd.utils.synthetic import llama_state_dict

    base = llama_state_dict(cfg, seed=seed, std=0.05)
    sds = {"awq": {}, "gptq": {}, "f32": {}}
    for name, t in base.items():
        if not any(name.endswith(p + ".weight") for p in LINEARS):
            for sd in sds.values():
                sd[name] = t
            continue
        c, z, s = random_params(t.shape[0], t.shape[1], seed=len(sds["f32"]), zlo=1, zhi=15)
        sds["f32"][name] = _formula(c, z, s).float()
        for fmt, pack in (("awq", pack_awq), ("gptq", pack_gptq)):
            sds[fmt].update({name[:-6] + k: v for k, v in pack(c, z, s).items()})
    return sds


def _prefill_logits(model, n):
    from rag_llm_k8s_amd.models.llama import StepInput
    from rag_llm_k8s_amd.ops.backend import AttnMeta

    model.allocate_kv_cache(4, dtype=model.w.embed.dtype)
    bt = torch.tensor([[1, 2, 0, 0]], dtype=torch.int32)
    meta = AttnMeta("prefill", torch.tensor([n], dtype=torch.int32), bt, cu_q=torch.tensor([0, n], dtype=torch.int32),
                    host_kv_lens=[n], host_q_lens=[n])
    return model.forward(StepInput(torch.arange(1, n + 1, dtype=torch.int32), torch.arange(n, dtype=torch.int32),
                                   torch.arange(64, 64 + n, dtype=torch.int32), meta, None))


def test_llama_from_awq_and_gptq_state_dicts():
    from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights, llama_tiny

    cfg = llama_tiny(vocab=512, layers=2, hidden=256, heads=4, kv_heads=2, inter=512)
    sds = _quantized_state_dicts(cfg)
    w4 = {fmt: LlamaWeights.from_state_dict(cfg, sds[fmt], "cpu", quant=fmt) for fmt in ("awq", "gptq")}
    for La, Lg in zip(w4["awq"].layers, w4["gptq"].layers):
        for k in ("wqkv", "wo", "wgu", "wdown"):
            assert isinstance(La[k], I4.Int4Weight) and isinstance(Lg[k], I4.Int4Weight)
            assert torch.equal(La[k].packed, Lg[k].packed) and torch.equal(La[k].meta, Lg[k].meta)
        assert La["ln_in"].dtype == torch.bfloat16
    w = w4["gptq"]
    assert w.dtype == "int4" and w.lm_head.dtype == torch.bfloat16 and w.embed.dtype == torch.bfloat16

    def get(name, rows=None, cols=None):
        t = sds["f32"][name]
        t = t if rows is None else t[rows[0]:rows[1]]
        return t if cols is None else t[:, cols[0]:cols[1]]

    w32 = LlamaWeights.from_hf(cfg, get, "cpu", dtype=torch.float32)
    w16 = LlamaWeights.from_hf(cfg, get, "cpu")
    assert torch.equal(w.layers[1]["wgu"].dequant(), w32.layers[1]["wgu"])
    for n in (40, 89):  # the W4A16 regime and the dequantize-to-bf16 one
        l32, l16, l4 = (_prefill_logits(LlamaModel(cfg, x, "cpu", max_positions=512), n) for x in (w32, w16, w))
        e4, e16 = rel_err(l4, l32), rel_err(l16, l32)
        print("int4 tiny-model prefill logits vs fp32, n=%d: int4 %.5f, bf16 weights %.5f" % (n, e4, e16))
        assert e4 <= 2 * e16
    # TP shards are slices of the whole: rows for qkv / gate-up, a K range for o / down
    s1 = LlamaWeights.from_state_dict(cfg, sds["awq"], "cpu", tp_rank=1, tp_size=2, quant="awq")
    full, part = w.layers[0], s1.layers[0]
    assert part["wo"].shape == (256, 128) and part["wdown"].shape == (256, 256)
    assert torch.equal(part["wdown"].packed, full["wdown"].packed[:, 128:])
    assert torch.equal(part["wdown"].meta, full["wdown"].meta[:, 2:])
    assert torch.equal(part["wo"].dequant(), full["wo"].dequant()[:, 128:])
    assert torch.equal(part["wqkv"].packed[:128], full["wqkv"].packed[128:256])  # q heads 2, 3
    assert torch.equal(part["wgu"].meta, full["wgu"].meta[512:])


def test_backend_gates_refuse_int4():
    from rag_llm_k8s_amd.ops.backend import AttnMeta, TorchBackend

    be = TorchBackend()
    be.enable_part = True
    w = I4.quantize_weight(torch.randn(256, 256).bfloat16())
    bf = torch.randn(256, 256).bfloat16()
    assert be.part_ok(1, bf) and not be.part_ok(1, w)
    assert not be.part_norm_ok(1, w) and not be.part_silu_ok(1, w, w) and not be.mlp_engine_ok(1, w, w)
    assert not be.part_merge_ok(1, AttnMeta("decode", None, None), w, 2, 128) and be.prefill_nsplit(5000, w) == 1
    x = torch.randn(3, 256).bfloat16()
    assert torch.equal(be.gemm_part(x, w)[0], x.float() @ w.dequant().t())
    assert torch.equal(be.gemm(x, w), I4.reference_linear(x, w))


def test_config_and_builder(tmp_path, monkeypatch):
    from rag_llm_k8s_amd.config import RagConfig
    from rag_llm_k8s_amd.engine.llm_engine import SamplingParams
    from rag_llm_k8s_amd.models.llama import llama_tiny
    from rag_llm_k8s_amd.runtime.safetensors_io import save_sharded
    from rag_llm_k8s_amd.server import builder
    from rag_llm_k8s_amd.utils import synthetic as S

    monkeypatch.setenv("DTYPE", "int4")
    cfg = RagConfig.from_env()
    assert cfg.dtype == "int4"
    (tmp_path / "config.json").write_text(json.dumps({"model_type": "gpt2"}))
    cfg.model_path, cfg.kv_cache_blocks, cfg.use_cuda_graphs = str(tmp_path), 32, False
    with pytest.raises(ValueError, match="int4"):
        builder.build_generator(cfg, "cpu")
    # a GPTQ checkpoint directory: quantization_config in config.json, qweight / qzeros / scales / g_idx tensors
    lc = llama_tiny(vocab=512, layers=2, hidden=256, heads=4, kv_heads=2, inter=512)
    qc = {"quant_method": "gptq", "bits": 4, "group_size": 128, "desc_act": False}
    (tmp_path / "config.json").write_text(json.dumps(dict(lc.to_hf_dict(), quantization_config=qc)))
    save_sharded(_quantized_state_dicts(lc)["gptq"], str(tmp_path), 2)
    S.train_small_bpe(str(tmp_path), lc.vocab_size, S.WordModel(n_words=2000, seed=11))
    cfg.dtype = "bf16"
    with pytest.raises(ValueError, match="DTYPE=int4"):
        builder.build_generator(cfg, "cpu")
    cfg.dtype = "int4"
    engine, tok, _ = builder.build_generator(cfg, "cpu")
    assert isinstance(engine.model.w.layers[0]["wqkv"], I4.Int4Weight) and engine.model.w.dtype == "int4"
    out = engine.generate([tok.encode("the quick brown fox")], SamplingParams(max_new_tokens=4, do_sample=False,
                                                                             ignore_eos=True))
    assert len(out[0]) == 4
