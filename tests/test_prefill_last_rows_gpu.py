"""The last decoder layer of a prefill step computed only where a row of logits_idx lies
(models/llama.py:_last_rows, RAGK_PREFILL_LAST_ROWS): with the knob on and off, hidden_states returns
bit-identical rows and every layer's K/V cache holds identical bits, for steps below the large-M route (the
layer runs in full either way), packed steps on the tile-list route, a chunk without a finishing row, a chunk
holding a prompt's tail, decode riders, and the split-K route (M >= 4096); and the engine samples the same
tokens."""
import numpy as np
import pytest
import torch

from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights, StepInput, llama_tiny
from rag_llm_k8s_amd.ops.backend import AttnMeta
from rag_llm_k8s_amd.utils.synthetic import llama_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
BLOCK = 64
SEQ_BLOCKS = 40  # cache blocks per sequence: 2560 tokens
MAX_SEQS = 6

CFGS = {
    "2x512": dict(vocab=1024, layers=2, hidden=512, heads=4, kv_heads=1, inter=512),
    "3x256": dict(vocab=1024, layers=3, hidden=256, heads=2, kv_heads=1, inter=512),
}


@pytest.fixture(scope="module", params=sorted(CFGS))
def models(request, native):
    """Two models on the same weights, each with its own KV cache: [knob on, knob off]."""
    cfg = llama_tiny(**CFGS[request.param])
    w = LlamaWeights.from_state_dict(cfg, llama_state_dict(cfg, seed=11, std=0.05), DEV)
    ms = [LlamaModel(cfg, w, DEV, max_positions=4096) for _ in range(2)]
    for m in ms:
        m.allocate_kv_cache(1 + MAX_SEQS * SEQ_BLOCKS)
    return ms


def _step_input(native, model, chunks, out_rows, cut):
    """Packed prefill step of chunks [(seq, start, n)]; sequence s owns cache blocks 1 + s * SEQ_BLOCKS ...
    cut: also hand the model the last-layer lists (as the engine does)."""
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
    ids, pos, slots, cu, kvl, qlens = [], [], [], [0], [], []
    bts = np.zeros((len(chunks), SEQ_BLOCKS), dtype=np.int32)
    for ci, (s, start, n) in enumerate(chunks):
        assert s < MAX_SEQS and start + n <= SEQ_BLOCKS * BLOCK
        table = 1 + s * SEQ_BLOCKS + np.arange(SEQ_BLOCKS)
        p = np.arange(start, start + n)
        ids.append((p * 7 + s * 131 + 3) % 1000)
        pos.append(p)
        slots.append(table[p // BLOCK] * BLOCK + p % BLOCK)
        cu.append(cu[-1] + n)
        kvl.append(start + n)
        qlens.append(n)
        bts[ci] = table
    tiles = native.build_prefill_tiles(qlens, model.Hq, model.Hkv)
    meta = AttnMeta("prefill", i32(kvl), i32(bts), cu_q=i32(cu), tiles=tiles.to(DEV), host_kv_lens=kvl,
                    host_q_lens=qlens)
    m_tiles = None
    if cut and out_rows:
        tl, mt = native.build_last_rows_lists(qlens, out_rows, model.Hq, model.Hkv, tiles=tiles)
        meta.tiles_last, m_tiles = tl.to(DEV), mt.to(DEV)
    return StepInput(i32(np.concatenate(ids)), i32(np.concatenate(pos)), i32(np.concatenate(slots)), meta,
                     i32(np.asarray(out_rows, dtype=np.int32)), m_tiles=m_tiles)


def _run_steps(native, models, monkeypatch, steps, expect):
    """Every step on both models; returns nothing, asserts equality after every step. expect[i]: the mode
    _last_rows must pick for step i with the knob on (None / "skip" / "tiles")."""
    on, off = models
    for m in models:
        for k, v in m.kv_cache:
            k.zero_()
            v.zero_()
    for (chunks, out_rows), mode in zip(steps, expect):
        M = sum(n for _, _, n in chunks)
        monkeypatch.setenv("RAGK_PREFILL_LAST_ROWS", "1")
        inp = _step_input(native, on, chunks, out_rows, cut=True)
        assert on._last_rows(inp, M) == mode
        a = on.hidden_states(inp)
        monkeypatch.setenv("RAGK_PREFILL_LAST_ROWS", "0")
        inp0 = _step_input(native, off, chunks, out_rows, cut=False)
        assert off._last_rows(inp0, M) is None
        b = off.hidden_states(inp0)
        assert a.shape == b.shape == (len(out_rows), on.cfg.hidden_size)
        assert torch.equal(a, b)
        assert not torch.isnan(a.float()).any()
        for li, ((k1, v1), (k0, v0)) in enumerate(zip(on.kv_cache, off.kv_cache)):
            assert torch.equal(k1, k0) and torch.equal(v1, v0), "layer %d K/V cache" % li
    assert any(float(k.float().abs().max()) > 0 for k, _ in on.kv_cache)


def _ends(lens):
    return (np.cumsum(lens) - 1).tolist()


def test_short_prompt(native, models, monkeypatch):
    _run_steps(native, models, monkeypatch, [([(0, 0, 100)], [99])], [None])  # below the large-M GEMM route


def test_four_packed_prompts(native, models, monkeypatch):
    lens = [300, 257, 411, 255]
    _run_steps(native, models, monkeypatch, [([(s, 0, n) for s, n in enumerate(lens)], _ends(lens))], ["tiles"])


def test_chunk_without_finishing_row_then_tail(native, models, monkeypatch):
    steps = [
        ([(0, 0, 1100)], []),                                            # seq 0 is 1500 tokens: no row needed
        ([(0, 1100, 400), (1, 0, 700), (2, 0, 130)], _ends([400, 700, 130])),  # its tail + whole prompts
    ]
    _run_steps(native, models, monkeypatch, steps, ["skip", "tiles"])


def test_mixed_step_with_decode_riders(native, models, monkeypatch):
    lens = [40, 70, 100]
    steps = [
        ([(s, 0, n) for s, n in enumerate(lens)], _ends(lens)),
        # the three sequences decode one token each inside the prefill step of a new 1100-token prompt
        ([(s, n, 1) for s, n in enumerate(lens)] + [(3, 0, 1100)], [0, 1, 2, 1102]),
    ]
    _run_steps(native, models, monkeypatch, steps, [None, "tiles"])


def test_split_k_route(native, models, monkeypatch):
    lens = [2100, 1500, 600]
    on = models[0]
    L0 = on.w.layers[0]
    assert max(on.be.prefill_nsplit(sum(lens), L0["wo"]), on.be.prefill_nsplit(sum(lens), L0["wdown"])) > 1
    _run_steps(native, models, monkeypatch, [([(s, 0, n) for s, n in enumerate(lens)], _ends(lens))], ["tiles"])


def test_engine_tokens_equal(native, monkeypatch):
    """Engine end to end (chunked prefill on the tile-list route, hipGraph decode): 3 prompts, 8 sampled tokens
    each with fixed seeds, identical with the knob on and off."""
    from rag_llm_k8s_amd.engine.llm_engine import LLMEngine, SamplingParams

    cfg = llama_tiny(**CFGS["2x512"])
    sd = llama_state_dict(cfg, seed=3, std=0.05)
    torch.manual_seed(5)
    prompts = [torch.randint(3, 1000, (n,)).tolist() for n in (1100, 300, 50)]
    p = SamplingParams(max_new_tokens=8, temperature=0.8, top_p=0.9, top_k=40, ignore_eos=True)
    outs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("RAGK_PREFILL_LAST_ROWS", knob)
        m = LlamaModel(cfg, LlamaWeights.from_state_dict(cfg, sd, DEV), DEV, max_positions=2048)
        eng = LLMEngine(m, num_blocks=64, max_batch=8, max_prefill_tokens=1200, max_model_len=2048, use_graphs=True)
        outs[knob] = eng.generate(prompts, p, seeds=[1, 2, 3])
    assert outs["1"] == outs["0"] and all(len(o) == 8 for o in outs["1"])
