"""The host lists of the cut-down last prefill layer (ops/native.py:build_last_rows_lists): the filtered
attention work list and the GEMM M-tile list cover every row of logits_idx, keep nothing else, and keep the
full list's order; the CPU engine (which only ever skips the last layer of a chunk without a finishing row)
samples the same tokens with RAGK_PREFILL_LAST_ROWS on and off."""
import numpy as np
import pytest
import torch

from rag_llm_k8s_amd.ops.native import build_last_rows_lists, build_prefill_tiles, prefill_qtile


def _covered(tiles, q_lens, qt):
    cu = np.concatenate([[0], np.cumsum(q_lens)])
    rows = set()
    for s, q0 in tiles.tolist():
        rows.update(range(cu[s] + q0, min(cu[s] + q0 + qt, cu[s + 1])))
    return rows


@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (4, 2), (4, 1)])
@pytest.mark.parametrize("q_lens", [
    [255, 1, 1, 300],        # prompt ends at packed rows 254 / 255 / 256 / 556
    [256, 1, 257],           # ... 255 / 256 / 513
    [257, 255, 1, 1, 1],     # ... 256 / 511 / 512 / 513 / 514
    [5210, 1, 1, 1, 700],
    [100],
])
def test_lists_cover_logits_rows(Hq, Hkv, q_lens):
    qt = prefill_qtile(Hq, Hkv)
    rows = (np.cumsum(q_lens) - 1).tolist()  # the last row of every sequence, riders included
    full = build_prefill_tiles(q_lens, Hq, Hkv)
    tl, mt = build_last_rows_lists(q_lens, rows, Hq, Hkv)
    assert tl.dtype == torch.int32 and mt.dtype == torch.int32 and tl.shape[1] == 2
    # every needed row lies in a kept query block and in a listed 256-row tile
    cov = _covered(tl, q_lens, qt)
    assert set(rows) <= cov
    assert set(r // 256 for r in rows) == set(mt.tolist())
    assert mt.tolist() == sorted(set(mt.tolist()))  # strictly increasing
    # nothing else is kept: every kept block holds a needed row, exactly one block per needed row here
    assert len(tl) == len(rows)
    for s, q0 in tl.tolist():
        assert q0 <= q_lens[s] - 1 < q0 + qt
    # a sub-list of the full work list, in its order
    fl = [tuple(t) for t in full.tolist()]
    pos = [fl.index(tuple(t)) for t in tl.tolist()]
    assert pos == sorted(pos)


def test_lists_inner_rows_and_errors():
    q_lens = [600, 40]
    tl, mt = build_last_rows_lists(q_lens, [0, 63, 64, 255, 256, 257, 639], 4, 1)  # 64-query blocks
    assert sorted(map(tuple, tl.tolist())) == [(0, 0), (0, 64), (0, 192), (0, 256), (1, 0)]
    assert mt.tolist() == [0, 1, 2]
    tl, mt = build_last_rows_lists(q_lens, [], 4, 1)
    assert tl.shape == (0, 2) and mt.numel() == 0
    with pytest.raises(ValueError):
        build_last_rows_lists(q_lens, [640], 4, 1)


def test_cpu_engine_tokens_equal_with_and_without(monkeypatch):
    """Chunked prefill on the CPU backend: chunks without a finishing row skip the last layer after its KV
    write, all other steps run it in full -- the sampled tokens do not change."""
    from rag_llm_k8s_amd.engine.llm_engine import LLMEngine, SamplingParams
    from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights, llama_tiny
    from rag_llm_k8s_amd.utils.synthetic import llama_state_dict

    cfg = llama_tiny(vocab=384, layers=2, hidden=256, heads=4, kv_heads=2, inter=512)
    sd = llama_state_dict(cfg, seed=5, std=0.05)
    torch.manual_seed(2)
    prompts = [torch.randint(3, 380, (n,)).tolist() for n in (7, 90, 33)]
    p = SamplingParams(max_new_tokens=5, temperature=0.8, top_p=0.9, top_k=40, ignore_eos=True)
    outs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("RAGK_PREFILL_LAST_ROWS", knob)
        m = LlamaModel(cfg, LlamaWeights.from_state_dict(cfg, sd, "cpu"), "cpu", max_positions=512)
        eng = LLMEngine(m, num_blocks=32, max_batch=4, max_prefill_tokens=40, max_model_len=512, use_graphs=False)
        outs[knob] = eng.generate(prompts, p, seeds=[1, 2, 3])
        assert eng.stats["prefill_steps"] >= 3  # the 90-token prompt is cut into chunks
    assert outs["1"] == outs["0"]
