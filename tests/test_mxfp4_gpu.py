"""MXFP4 weight GEMMs (csrc/kernels/gemm_mxfp4.hip) vs their fp32 oracle (ops/mxfp4.reference_linear):
W4A16 decode (M <= 64, v_cvt_scalef32_pk_bf16_fp4 + bf16 MFMA) and W4A8 prefill (block-scaled e4m3 x e2m1 MFMA).
The exact-integer tests pin the operand layout of both instructions bit for bit."""
import functools
import math

import pytest
import torch

from rag_llm_k8s_amd.ops import mxfp4 as F4
from rag_llm_k8s_amd.ops import reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


# ----------------------------------------------------------------------------- operand layout, bit for bit
def _int_weight(N, K, seed):
    """Every one of the 16 codes, scale bytes 125..129: values k / 8 with |k| <= 192."""
    g = torch.Generator().manual_seed(seed)
    packed = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    scale = torch.randint(125, 130, (N, K // 32), generator=g, dtype=torch.uint8)
    return F4.Mxfp4Weight(packed.to(DEV), scale.to(DEV)), F4.Mxfp4Weight(packed, scale).dequant().double()


def _int_acts(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (M, K), generator=g).float()


@pytest.mark.parametrize("K", [128, 384, 512])
@pytest.mark.parametrize("N", [16, 40])
@pytest.mark.parametrize("M", [1, 16, 17, 64])
def test_decode_layout_exact(native, M, N, K):
    """Integer activations in [-8, 8] against weights that are multiples of 1/8 up to 24: every product and every
    partial sum (at most 512 * 8 * 192 < 2^20 eighths) is exact in fp32, so any summation order gives the same
    bits -- and a swapped nibble, a transposed tile or a scale from the wrong lane or block cannot."""
    w, wd = _int_weight(N, K, 1000 * M + N + K)
    x = _int_acts(M, K, M + K)
    y = native.gemm_mxfp4(x.to(DEV).bfloat16(), w, out_f32=True)
    ref = (x.double() @ wd.t()).float()
    assert torch.equal(y.cpu(), ref), (y.cpu() - ref).abs().max().item()


@pytest.mark.parametrize("K", [128, 384, 512, 640, 1152])  # 1, 3, 4, 5, 9 K steps: the scale groups and their tails
@pytest.mark.parametrize("N", [128, 136])
@pytest.mark.parametrize("M", [65, 129])
def test_prefill_layout_exact(native, M, N, K):
    """The scaled MFMA with e4m3 activations (integers, exact) and power-of-two row scales handed in through act=:
    same exactness argument as the decode test, on the fp4 operand and scale-operand lane maps."""
    w, wd = _int_weight(N, K, 2000 * M + N + K)
    x = _int_acts(M, K, M + K + 1)
    g = torch.Generator().manual_seed(M)
    sa = torch.ldexp(torch.ones(M), torch.randint(-2, 3, (M,), generator=g))
    y = native.gemm_mxfp4(None, w, out_f32=True, act=(x.to(torch.float8_e4m3fn).to(DEV), sa.to(DEV)))
    ref = ((x.double() * sa.double()[:, None]) @ wd.t()).float()
    assert torch.equal(y.cpu(), ref), (y.cpu() - ref).abs().max().item()


# ----------------------------------------------------------------------------- random data, every epilogue
@functools.lru_cache(maxsize=None)
def _weights(N, K):
    g = torch.Generator(device=DEV).manual_seed(N + K)
    w = (torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)).bfloat16()
    return w, F4.quantize_weight(w)


@pytest.fixture(scope="module", autouse=True)
def _release_shared_weights():
    """The weights shared by the epilogue cases live for this module only: hand their HBM back afterwards."""
    yield
    _weights.cache_clear()
    torch.cuda.empty_cache()


SHAPES = [(M, N, K) for N, K in [(768, 1024), (4096, 4096)] for M in (1, 7, 16, 33, 64, 65, 200)]
SHAPES += [(1, 1024, 14336), (200, 1024, 14336)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_mxfp4_epilogues(native, M, N, K):
    torch.manual_seed(M + N)
    w, wq = _weights(N, K)
    x = torch.randn(M, K, device=DEV).bfloat16()
    bias = torch.randn(N, device=DEV).bfloat16()
    r = torch.randn(M, N, device=DEV).bfloat16()
    for epi, kw in [("none", {}), ("resid", dict(resid=r)), ("bias", dict(bias=bias)),
                    ("bias_gelu", dict(bias=bias))]:
        y = native.gemm_mxfp4(x, wq, epi=epi, **kw)
        ref = F4.reference_linear(x, wq, epi=epi, **kw)
        assert rel_err(y, ref) < 1e-2, (epi, rel_err(y, ref))
    yf = native.gemm_mxfp4(x, wq, out_f32=True)
    assert rel_err(yf, F4.reference_linear(x, wq, out_f32=True)) < 2e-3
    # vs the bf16 product: the MXFP4 error budget of tests/test_mxfp4_cpu.py
    assert rel_err(native.gemm_mxfp4(x, wq), x.float() @ w.float().t()) < 0.135


@pytest.mark.parametrize("M", [1, 64, 300])
def test_gemm_mxfp4_silu_mul(native, M):
    torch.manual_seed(5)
    K, N = 1024, 192  # three packed [64 gate | 64 up] tiles
    x = torch.randn(M, K, device=DEV).bfloat16()
    g = (torch.randn(N, K, device=DEV) / 32).bfloat16()
    u = (torch.randn(N, K, device=DEV) / 32).bfloat16()
    wq = F4.quantize_weight(R.pack_gate_up(g, u))
    y = native.gemm_mxfp4(x, wq, epi="silu_mul")
    ref = F4.reference_linear(x, wq, epi="silu_mul")
    assert y.shape == (M, N) and rel_err(y, ref) < 1e-2


def test_gemm_mxfp4_shape_checks(native):
    _, wq = _weights(768, 1024)
    with pytest.raises(Exception):
        native.gemm_mxfp4(torch.zeros(4, 512, device=DEV).bfloat16(), wq)  # K mismatch
    with pytest.raises(Exception):
        native.gemm_mxfp4(torch.zeros(4, 1024, device=DEV).bfloat16(), wq, epi="bias")  # bias missing


# ----------------------------------------------------------------------------- out-of-bounds canary
PAD = 4096


@pytest.mark.parametrize("M,N,epi", [(7, 40, "none"), (7, 40, "resid"), (65, 136, "none"), (65, 136, "resid")])
def test_outputs_stay_in_bounds(native, M, N, epi):
    """Ragged M and N tails of the decode (N = 40: 2.5 column tiles) and prefill (N = 136: one tile + 8 columns)
    kernels: the output is a view inside a sentinel-filled buffer and the sentinels stay untouched."""
    torch.manual_seed(M)
    K = 384
    x = torch.randn(M, K, device=DEV).bfloat16()
    wq = F4.quantize_weight((torch.randn(N, K, device=DEV) / math.sqrt(K)).bfloat16())
    r = torch.randn(M, N, device=DEV).bfloat16() if epi == "resid" else None
    for dt in (torch.bfloat16, torch.float32):
        buf = torch.full((2 * PAD + M * N,), -7.0, dtype=dt, device=DEV)
        out = buf[PAD:PAD + M * N].view(M, N)
        native.gemm_mxfp4(x, wq, resid=r, epi=epi, out=out, out_f32=dt == torch.float32)
        torch.cuda.synchronize()
        assert bool(buf[:PAD].eq(-7.0).all()) and bool(buf[-PAD:].eq(-7.0).all())
        assert rel_err(out, F4.reference_linear(x, wq, resid=r, epi=epi, out_f32=True)) < 1e-2


# ----------------------------------------------------------------------------- engine
def test_mxfp4_engine_gpu_matches_cpu_reference(native):
    """MXFP4-weight Llama: GPU engine (fp4 kernels, generic decode path under hipGraph) vs the CPU engine running
    the fp32 oracle of the same quantized arithmetic; prefill logits (W4A8) and greedy tokens (W4A16)."""
    from rag_llm_k8s_amd.engine.llm_engine import LLMEngine, SamplingParams
    from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights, StepInput, llama_tiny
    from rag_llm_k8s_amd.ops.backend import AttnMeta
    from rag_llm_k8s_amd.ops.native import build_prefill_tiles
    from rag_llm_k8s_amd.utils.synthetic import llama_state_dict

    cfg = llama_tiny(vocab=1024, layers=2, hidden=512, heads=4, kv_heads=1, inter=512)
    sd = llama_state_dict(cfg, seed=3, std=0.05)

    def engine(dev, graphs):
        w = LlamaWeights.from_state_dict(cfg, sd, dev).quantize_mxfp4()
        assert isinstance(w.layers[0]["wqkv"], F4.Mxfp4Weight) and w.dtype == "mxfp4"
        m = LlamaModel(cfg, w, dev, max_positions=2048)
        return LLMEngine(m, num_blocks=64, max_batch=8, max_prefill_tokens=300, max_model_len=2048, use_graphs=graphs)

    outs = {}
    for dev in ("cuda", "cpu"):
        eng = engine(dev, False)
        eng.bm.ensure(7, 150)
        tbl = eng.bm.table(7)
        slots = torch.tensor([tbl[p // 64] * 64 + p % 64 for p in range(150)], dtype=torch.int32)
        bt = torch.tensor([tbl + [0] * (eng.max_blocks - len(tbl))], dtype=torch.int32)
        meta = AttnMeta("prefill", torch.tensor([150], dtype=torch.int32).to(dev), bt.to(dev),
                        cu_q=torch.tensor([0, 150], dtype=torch.int32).to(dev),
                        tiles=build_prefill_tiles([150], 4, 1).to(dev), host_kv_lens=[150])
        ids = torch.arange(150, dtype=torch.int32) * 7 % 1000
        inp = StepInput(ids.to(dev), torch.arange(150, dtype=torch.int32).to(dev), slots.to(dev), meta, None)
        outs[dev] = eng.model.forward(inp).float().cpu()
    # the weights dequantize exactly on both sides; W4A8 re-quantizes every layer input, so bf16-level GPU/CPU
    # differences flip e4m3 roundings exactly as in the fp8 engine test
    e = rel_err(outs["cuda"], outs["cpu"])
    print("mxfp4 engine prefill logits GPU vs CPU: %.4f" % e)
    assert e < 0.15
    torch.manual_seed(0)
    prompts = [torch.randint(3, 1000, (n,)).tolist() for n in (5, 77, 130, 300)]
    p = SamplingParams(max_new_tokens=6, do_sample=False, ignore_eos=True)
    gpu = engine("cuda", True).generate(prompts, p)
    cpu = engine("cpu", False).generate(prompts, p)
    first = sum(int(g[0] == c[0]) for g, c in zip(gpu, cpu))
    assert first >= 3, (gpu, cpu)
