"""4-bit integer weight kernels (csrc/kernels/gemm_int4.hip) against float64: the fused W4A16 decode GEMM bit for
bit on exact-integer data and within the fp32 product's own error on random data, dequant_int4, the M > 64
route through the bf16 GEMM, the launcher's refusals and the tiny int4 engine."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from int4_cases import random_params
from rag_llm_k8s_amd.ops import int4 as I4
from rag_llm_k8s_amd.ops import reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 1024


def _weight(N, K, seed, pow2):
    codes, zeros, scales = random_params(N, K, seed=seed, pow2=pow2)
    w = I4.Int4Weight.from_codes(codes, scales, zeros)
    return w.to(DEV), w.dequant(torch.float64)


@functools.lru_cache(maxsize=None)
def _exact_case(N, K):
    """Shared by the M cases: the weight, 64 rows of integer activations, bias, residual, the float64 product."""
    w, wd = _weight(N, K, seed=N + K, pow2=True)
    g = torch.Generator().manual_seed(K + N)
    x = torch.randint(-4, 5, (64, K), generator=g).double()
    bias, resid = torch.randint(-8, 9, (N,), generator=g).double(), torch.randint(-8, 9, (64, N), generator=g).double()
    # every partial sum, in any order, is a multiple of 2^-3 below 2^24 of them: exact in fp32
    assert float((x.abs() @ wd.abs().t()).max()) * 8 < 2 ** 24
    return w, x, bias, resid, x @ wd.t()


def _framed(M, N, dt):
    """An [M, N] output inside a sentinel frame, rows pitched N + 8 apart (the gaps are sentinels too)."""
    buf = torch.full((2 * PAD + M * (N + 8),), -7.0, dtype=dt, device=DEV)
    return buf, buf[PAD:PAD + M * (N + 8)].view(M, N + 8)[:, :N]


def _frame_intact(buf, out):
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[PAD:PAD + out.shape[0] * out.stride(0)].view(out.shape[0], -1)[:, :out.shape[1]] = False
    return bool(buf[keep].eq(-7.0).all())


@pytest.mark.parametrize("K", [128, 256, 1152])  # 1152: 9 K blocks over 8 waves
@pytest.mark.parametrize("N", [16, 24, 136])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 64])
def test_decode_exact(native, M, N, K):
    """code - zero is an exact bf16 integer and the scales are powers of two, so the kernel's sums are exact in
    any order: a misplaced nibble, zero point, scale or tile cannot give the float64 product's bits."""
    w, x, bias, resid, ref = _exact_case(N, K)
    xg, bg, rg = x[:M].to(DEV).bfloat16(), bias.to(DEV).bfloat16(), resid[:M].to(DEV).bfloat16()
    cases = [("none", {}, ref[:M], False), ("resid", dict(resid=rg), ref[:M] + resid[:M], False),
             ("bias", dict(bias=bg), ref[:M] + bias, False), ("none", {}, ref[:M], True)]
    for epi, kw, want, f32 in cases:
        dt = torch.float32 if f32 else torch.bfloat16
        buf, out = _framed(M, N, dt)
        native.gemm_int4(xg, w, epi=epi, out=out, out_f32=f32, **kw)
        first = out.clone()
        assert torch.equal(first.cpu(), want.to(dt)), (epi, f32, (first.cpu().double() - want).abs().max().item())
        assert _frame_intact(buf, out)
        native.gemm_int4(xg, w, epi=epi, out=out, out_f32=f32, **kw)
        assert torch.equal(out, first)


def _bound(got, x, wd_parts, fn, out_dt):
    """|got - float64| <= max(8 x the fp32 torch result's error against float64, one ulp of the output)."""
    ref = fn(*(x.double() @ p.t() for p in wd_parts))
    e32 = (fn(*(x.float() @ p.float().t() for p in wd_parts)).double() - ref).abs().max().item()
    ulp = 2.0 ** (math.floor(math.log2(float(ref.abs().max()))) - (7 if out_dt == torch.bfloat16 else 23))
    err = (got.double().cpu() - ref).abs().max().item()
    print("err %.3e, fp32 product err %.3e, ulp %.3e" % (err, e32, ulp))
    assert err <= max(8 * e32, ulp)


@pytest.mark.parametrize("M", [1, 33, 64])
def test_decode_random_f32_out(native, M):
    w, wd = _weight(136, 1152, seed=M, pow2=False)
    x = torch.randn(M, 1152, generator=torch.Generator().manual_seed(M)).bfloat16()
    _bound(native.gemm_int4(x.to(DEV), w, out_f32=True), x, [wd], lambda y: y, torch.float32)


@pytest.mark.parametrize("N", [64, 192])
@pytest.mark.parametrize("M", [1, 17, 64])
def test_decode_silu_mul(native, M, N):
    w, wd = _weight(2 * N, 384, seed=N + M, pow2=False)
    x = torch.randn(M, 384, generator=torch.Generator().manual_seed(N)).bfloat16()
    y = native.gemm_int4(x.to(DEV), w, epi="silu_mul")
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    _bound(y, x, R.unpack_gate_up(wd), lambda g, u: F.silu(g) * u, torch.bfloat16)


@pytest.mark.parametrize("K", [128, 1152])
@pytest.mark.parametrize("rows", [1, 17, 136])
def test_dequant_int4(native, rows, K):
    w, _ = _weight(rows, K, seed=rows + K, pow2=False)
    buf, out = _framed(rows, K, torch.bfloat16)
    native.dequant_int4(w, out)
    assert torch.equal(out.cpu(), w.to("cpu").dequant(torch.bfloat16)) and _frame_intact(buf, out)


@pytest.mark.parametrize("M", [64, 65, 200])
def test_backend_routes(native, M):
    """Up to 64 rows the fused kernel (the fp32 oracle's bits on exact data), above that dequant_int4 into the
    scratch and the bf16 GEMM: the same kernel on the same operands as native.gemm on dequant(bf16)."""
    from rag_llm_k8s_amd.ops.backend import NativeBackend

    be = NativeBackend()
    w, wd = _weight(136, 384, seed=M, pow2=True)
    g = torch.Generator().manual_seed(M)
    x = torch.randint(-4, 5, (M, 384), generator=g).bfloat16().to(DEV)
    r = torch.randint(-8, 9, (M, 136), generator=g).bfloat16().to(DEV)
    y = be.gemm(x, w, resid=r, epi="resid")
    if M <= 64:
        assert torch.equal(y.cpu(), (x.cpu().double() @ wd.t() + r.cpu().double()).bfloat16())
    else:
        wb = torch.empty(136, 384, dtype=torch.bfloat16, device=DEV)
        native.dequant_int4(w, wb)
        assert torch.equal(wb.cpu(), w.to("cpu").dequant(torch.bfloat16))
        assert torch.equal(y, native.gemm(x, wb, resid=r, epi="resid"))
        w2, _ = _weight(128, 384, seed=M + 1, pow2=False)  # packed gate/up rows through the same route
        assert torch.equal(be.gemm(x, w2, epi="silu_mul"), native.gemm(x, native.dequant_int4(w2), epi="silu_mul"))


def test_launcher_refusals(native):
    """K % 128, a pitch that is not a multiple of 16 bytes and M > 64 come back as hipErrorInvalidValue from the
    entry points themselves, with nothing launched: the output keeps its sentinels."""
    L = native._lib.lib()
    w, _ = _weight(16, 256, seed=0, pow2=True)
    x = torch.ones(80, 264, dtype=torch.bfloat16, device=DEV)
    out = torch.full((80, 256), -7.0, dtype=torch.bfloat16, device=DEV)

    def call(M=4, K=256, ldw=128, ldx=264):
        return L.ragk_gemm_int4(x.data_ptr(), ldx, w.packed.data_ptr(), ldw, w.meta.data_ptr(), 2, out.data_ptr(), 256,
                                None, None, 0, M, 16, K, 0, 0, native.stream_ptr())

    assert call(K=192) == 1 and call(ldw=136) == 1 and call(ldx=260) == 1 and call(M=65) == 1
    assert L.ragk_dequant_int4(w.packed.data_ptr(), 128, w.meta.data_ptr(), 2, out.data_ptr(), 260, 16, 256,
                               native.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool(out.eq(-7.0).all())
    assert call() == 0
    with pytest.raises(ValueError):
        native.gemm_int4(x[:65, :256], w)  # the host-side check of the same limit
    with pytest.raises(ValueError):
        native.gemm_int4(x[:4, 4:260], w)  # rows not 16-byte aligned


def test_int4_engine_gpu_matches_cpu_reference(native):
    """Int4-weight Llama: the GPU engine (fused decode kernel under hipGraph, dequant + bf16 GEMM prefill)
    against the CPU engine running the fp32 oracle of the same arithmetic."""
    from rag_llm_k8s_amd.engine.llm_engine import LLMEngine, SamplingParams
    from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights, StepInput, llama_tiny
    from rag_llm_k8s_amd.ops.backend import AttnMeta
    from rag_llm_k8s_amd.ops.native import build_prefill_tiles
    from rag_llm_k8s_amd.utils.synthetic import llama_state_dict

    cfg = llama_tiny(vocab=1024, layers=2, hidden=512, heads=4, kv_heads=1, inter=512)
    sd = llama_state_dict(cfg, seed=3, std=0.05)

    def engine(dev, graphs):
        w = LlamaWeights.from_state_dict(cfg, sd, dev).quantize_int4()
        assert isinstance(w.layers[0]["wqkv"], I4.Int4Weight) and w.dtype == "int4"
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
    e = ((outs["cuda"] - outs["cpu"]).norm() / outs["cpu"].norm()).item()
    print("int4 engine prefill logits GPU vs CPU: %.4f" % e)
    assert e < 0.15
    torch.manual_seed(0)
    prompts = [torch.randint(3, 1000, (n,)).tolist() for n in (5, 77, 130, 300)]
    p = SamplingParams(max_new_tokens=6, do_sample=False, ignore_eos=True)
    cpu = engine("cpu", False).generate(prompts, p)
    for graphs in (False, True):  # eager and hipGraph decode
        gpu = engine("cuda", graphs).generate(prompts, p)
        assert sum(int(g[0] == c[0]) for g, c in zip(gpu, cpu)) >= 3, (graphs, gpu, cpu)
