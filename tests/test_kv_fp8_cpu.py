"""fp8 KV cache (KV_CACHE_DTYPE=fp8), CPU side: the oracle backend's cache format, sizing, configuration and
the format's drift against the bf16 cache (ops/fp8.Fp8KV: e4m3 data + one fp32 scale per cached row)."""
import types

import pytest
import torch

from rag_llm_k8s_amd.config import RagConfig
from rag_llm_k8s_amd.engine.llm_engine import LLMEngine, SamplingParams
from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights, StepInput, llama_tiny
from rag_llm_k8s_amd.ops.backend import AttnMeta
from rag_llm_k8s_amd.ops.fp8 import FP8, Fp8KV, quantize_rows
from rag_llm_k8s_amd.utils.synthetic import llama_state_dict


@pytest.fixture(scope="module")
def tiny_llama():
    cfg = llama_tiny(vocab=1024, layers=2, hidden=512, heads=4, kv_heads=1, inter=512)
    return cfg, llama_state_dict(cfg, seed=3, std=0.05)


def _engine(cfg, sd, kv_dtype, **kw):
    w = LlamaWeights.from_state_dict(cfg, sd, "cpu")
    m = LlamaModel(cfg, w, "cpu", max_positions=2048)
    return LLMEngine(m, num_blocks=64, max_batch=8, max_prefill_tokens=300, max_model_len=2048, use_graphs=False,
                     kv_dtype=kv_dtype, **kw)


def _prefill_logits(eng, ids):
    """Logits [T, V] of every position of `ids` (one prefill through the engine's model and cache)."""
    n = len(ids)
    eng.bm.ensure(99, n + 1)
    tbl = eng.bm.table(99)
    slots = torch.tensor([tbl[q // 64] * 64 + q % 64 for q in range(n)], dtype=torch.int32)
    bt = torch.tensor([tbl + [0] * (eng.max_blocks - len(tbl))], dtype=torch.int32)
    meta = AttnMeta("prefill", torch.tensor([n], dtype=torch.int32), bt, cu_q=torch.tensor([0, n], dtype=torch.int32),
                    host_kv_lens=[n])
    inp = StepInput(torch.tensor(ids, dtype=torch.int32), torch.arange(n, dtype=torch.int32), slots, meta, None)
    return eng.model.forward(inp).float()


def _assert_fp8_is_quantized_bf16(c8, c16):
    for li, ((k8, v8), (k16, v16)) in enumerate(zip(c8, c16)):
        for side, a, b in (("k", k8, k16), ("v", v8, v16)):
            assert isinstance(a, Fp8KV) and a.data.dtype == FP8 and a.scale.dtype == torch.float32
            q, s = quantize_rows(b.reshape(-1, b.shape[-1]))
            assert torch.equal(a.data.view(torch.uint8).reshape(-1, b.shape[-1]), q.view(torch.uint8)), (li, side)
            assert torch.equal(a.scale.reshape(-1), s), (li, side)


def test_oracle_fp8_cache_is_quantize_rows_of_bf16_cache():
    """The same prefill + 3 decode steps through a bf16-cache and an fp8-cache CPU model: after every step the
    fp8 cache equals quantize_rows of the bf16 cache, bit for bit, data and scales. The invariant is about
    identical inputs to the cache write, so the model has one layer (a deeper layer's input already carries the
    fp8 drift of the attention below it)."""
    cfg1 = llama_tiny(vocab=1024, layers=1, hidden=512, heads=4, kv_heads=1, inter=512)
    sd1 = llama_state_dict(cfg1, seed=3, std=0.05)
    torch.manual_seed(0)
    e16, e8 = _engine(cfg1, sd1, "bf16"), _engine(cfg1, sd1, "fp8")
    assert e8.stats["kv_dtype"] == "fp8" and e16.stats["kv_dtype"] == "bf16"
    n0 = 130
    ids = torch.randint(3, 1000, (n0 + 3,)).tolist()
    for eng in (e16, e8):
        eng.bm.ensure(7, len(ids) + 1)
    tbl = e16.bm.table(7)
    assert tbl == e8.bm.table(7)
    bt = torch.tensor([tbl + [0] * (e16.max_blocks - len(tbl))], dtype=torch.int32)

    def step(eng, lo, hi, kind):
        n = hi - lo
        slots = torch.tensor([tbl[q // 64] * 64 + q % 64 for q in range(lo, hi)], dtype=torch.int32)
        meta = AttnMeta(kind, torch.tensor([hi], dtype=torch.int32), bt, cu_q=torch.tensor([0, n], dtype=torch.int32),
                        host_kv_lens=[hi])
        inp = StepInput(torch.tensor(ids[lo:hi], dtype=torch.int32), torch.arange(lo, hi, dtype=torch.int32), slots,
                        meta, None)
        return eng.model.forward(inp)

    for eng in (e16, e8):
        step(eng, 0, n0, "prefill")
    _assert_fp8_is_quantized_bf16(e8.model.kv_cache, e16.model.kv_cache)
    for t in range(3):
        for eng in (e16, e8):
            step(eng, n0 + t, n0 + t + 1, "decode")
        _assert_fp8_is_quantized_bf16(e8.model.kv_cache, e16.model.kv_cache)
    k8 = e8.model.kv_cache[0][0]
    assert int((k8.data.view(torch.uint8) != 0).sum()) > 0 and bool((k8.scale != 1).any())


def test_kv_bytes_per_block_counts_scales(tiny_llama):
    cfg, sd = tiny_llama
    m = _engine(cfg, sd, "bf16").model
    layers, Hkv, D = cfg.num_hidden_layers, m.Hkv, m.D
    assert m.kv_bytes_per_block(torch.float8_e4m3fn) == 2 * layers * Hkv * 64 * (D + 4)
    assert m.kv_bytes_per_block(torch.bfloat16) == 2 * layers * Hkv * 64 * D * 2
    assert m.kv_bytes_per_block() == m.kv_bytes_per_block(torch.bfloat16)
    c = m.allocate_kv_cache(3, torch.float8_e4m3fn)
    assert sum(k.nbytes() + v.nbytes() for k, v in c) == 3 * m.kv_bytes_per_block(torch.float8_e4m3fn)


def test_kv_blocks_for_sizes_by_dtype(tiny_llama, monkeypatch):
    from rag_llm_k8s_amd.server import builder

    cfg, sd = tiny_llama
    m = _engine(cfg, sd, "bf16").model
    per16 = m.kv_bytes_per_block(torch.bfloat16)
    # a CPU budget of 2 GiB is far above `need` for the tiny model: shrink the model's blocks into range instead
    big = types.SimpleNamespace(kv_bytes_per_block=lambda dt=torch.bfloat16: m.kv_bytes_per_block(dt) * 512)
    rc = RagConfig(device="cpu", max_batch=64, max_model_len=16384)
    n16 = builder.kv_blocks_for(big, rc.replace(kv_cache_dtype="bf16"), "cpu")
    n8 = builder.kv_blocks_for(big, rc.replace(kv_cache_dtype="fp8"), "cpu")
    need = 64 * (16384 // 64) + 8
    assert n16 == (2 << 30) // (per16 * 512) and 16 < n16 < n8 <= need
    assert n8 == min(need, (2 << 30) // (m.kv_bytes_per_block(torch.float8_e4m3fn) * 512))
    small = RagConfig(device="cpu", max_batch=2, max_model_len=256)  # need = 2 * 4 + 8: both capped by need
    assert builder.kv_blocks_for(m, small.replace(kv_cache_dtype="fp8"), "cpu") == 16
    assert builder.kv_blocks_for(m, small.replace(kv_cache_dtype="bf16"), "cpu") == 16


def test_config_env_kv_cache_dtype(monkeypatch):
    monkeypatch.delenv("KV_CACHE_DTYPE", raising=False)
    assert RagConfig.from_env().kv_cache_dtype == "bf16"
    for v in ("bf16", "fp8"):
        monkeypatch.setenv("KV_CACHE_DTYPE", v)
        assert RagConfig.from_env().kv_cache_dtype == v
    monkeypatch.setenv("KV_CACHE_DTYPE", "int8")
    with pytest.raises(ValueError, match="KV_CACHE_DTYPE"):
        RagConfig.from_env()


def test_fp8_cache_refused_for_gpt2_and_head_dim_64():
    from rag_llm_k8s_amd.models.gpt2 import GPT2Model, GPT2Weights, gpt2_state_dict, gpt2_tiny

    cfg64 = llama_tiny(vocab=256, layers=1, hidden=256, heads=4, kv_heads=2, inter=256)  # head_dim 64
    assert cfg64.head_dim == 64
    m = LlamaModel(cfg64, LlamaWeights.random(cfg64, "cpu", 0, 1, seed=0), "cpu", max_positions=256)
    with pytest.raises(ValueError, match="head_dim 128"):
        LLMEngine(m, num_blocks=8, max_batch=2, max_model_len=256, use_graphs=False, kv_dtype="fp8")
    assert m.kv_cache is None or not isinstance(m.kv_cache[0][0], Fp8KV)  # never a silent bf16 fallback either
    LLMEngine(m, num_blocks=8, max_batch=2, max_model_len=256, use_graphs=False, kv_dtype="bf16")
    gc = gpt2_tiny(256)
    g = GPT2Model(gc, GPT2Weights.from_state_dict(gc, gpt2_state_dict(gc, seed=0), "cpu"), "cpu")
    with pytest.raises(ValueError, match="GPT-2"):
        LLMEngine(g, num_blocks=8, max_batch=2, max_model_len=128, use_graphs=False, kv_dtype="fp8")
    with pytest.raises(ValueError, match="bf16"):
        LLMEngine(m, num_blocks=8, max_batch=2, max_model_len=256, use_graphs=False, kv_dtype="int8")


def test_workload_answers_a_query_with_fp8_cache(monkeypatch):
    from rag_llm_k8s_amd.utils.workload import build_workload

    from rag_llm_k8s_amd.utils.workload import make_queries

    wl = build_workload(model="tiny", embedder="tiny", device="cpu", kv_dtype="fp8", n_chunks=40, chunk_words=30,
                        max_new_tokens=4, max_batch=2, max_model_len=1024, word_vocab=2000)
    svc = wl.svc
    assert svc.engine.stats["kv_dtype"] == "fp8" and svc.cfg.kv_cache_dtype == "fp8"
    assert isinstance(svc.engine.model.kv_cache[0][0], Fp8KV)
    out = svc.generate_batch(make_queries(wl.wm, 1, seed=1),
                             params=SamplingParams(max_new_tokens=4, do_sample=False, ignore_eos=True))[0]
    assert isinstance(out["generated_text"], str) and out["_gen_tokens"] == 4
    assert out["context"].startswith("Document 'synthetic_")
    # the env var is the default when the argument is not given
    monkeypatch.setenv("KV_CACHE_DTYPE", "fp8")
    wl2 = build_workload(model="tiny", embedder="tiny", device="cpu", n_chunks=8, chunk_words=30, max_new_tokens=2,
                         max_batch=2, max_model_len=1024, word_vocab=2000)
    assert wl2.svc.engine.stats["kv_dtype"] == "fp8"


# Worst per-step gap of the fp8-cache engine's greedy tokens below the bf16-cache oracle's top logit, as a
# fraction of the row's logit spread, measured on the tiny model (513-token prompt + 8 greedy tokens): 2.5191e-02
# (one near-tie flip at step 5, every other step the oracle's argmax; prefill-logit rel_err 6.3814e-02).
# The margin rule below runs at twice that.
FP8_KV_MEASURED_WORST_GAP = 2.5191e-2
FP8_KV_GREEDY_REL_TOL = 2 * FP8_KV_MEASURED_WORST_GAP


def test_format_drift_report(tiny_llama):
    """Report-only: how far the e4m3 cache moves the tiny model's prefill logits from the bf16-cache path (the
    parent's path is the reference). Asserts only that the drift is real and finite, and that the fp8 engine's
    greedy tokens stay within the measured margin of the bf16-cache oracle."""
    cfg, sd = tiny_llama
    torch.manual_seed(0)
    ids = torch.randint(3, 1000, (513,)).tolist()
    l16 = _prefill_logits(_engine(cfg, sd, "bf16"), ids)
    l8 = _prefill_logits(_engine(cfg, sd, "fp8"), ids)
    drift = ((l8 - l16).norm() / l16.norm()).item()
    print("fp8 KV cache: prefill-logit rel_err vs the bf16 cache at 513 tokens = %.4e" % drift)
    assert 0.0 < drift < float("inf")
    p = SamplingParams(max_new_tokens=8, do_sample=False, ignore_eos=True)
    out = _engine(cfg, sd, "fp8").generate([ids], p)[0]
    lg = _prefill_logits(_engine(cfg, sd, "bf16"), ids + out[:-1])
    worst = 0.0
    for k, tok in enumerate(out):
        row = lg[len(ids) - 1 + k]
        top = float(row.max())
        gap, spread = top - float(row[tok]), top - float(row.min())
        worst = max(worst, gap / spread)
        print("step %d: gap / spread = %.4e" % (k, gap / spread))
        assert gap <= FP8_KV_GREEDY_REL_TOL * spread, (k, tok, int(row.argmax()), gap, spread)
    print("worst gap / spread = %.4e" % worst)
