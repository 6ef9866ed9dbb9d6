"""The packed step block (engine/step_layout.py): the host array of every variant equals the words the engine
packed before the layout had one definition, every named view reads back what went in, and the graph keys."""
import itertools

import numpy as np
import pytest
import torch

from rag_llm_k8s_amd.engine.kv_manager import BLOCK
from rag_llm_k8s_amd.engine.llm_engine import SamplingParams, Sequence
from rag_llm_k8s_amd.engine.step_layout import BAN_IDS_MAX, GraphKey, StepLayout, graph_key

MB, K, EOS = 3, 64, {2}
F = lambda x: int(np.float32(x).view(np.int32))  # noqa: E731  the int32 word of a float32


def _seqs():
    """One plain row, one more, a processor row with a ban list (history row 1, 71 tokens: its slot lies in its
    second block), a penalty row with two bias entries (history row 0), a logprob row. name -> (sequence, blocks)."""
    def seq(prompt, out, params, seed, hist_row=-1):
        s = Sequence(prompt, params, seed)
        s.out, s.hist_row = list(out), hist_row
        return s
    return {
        "plain": (seq([5, 6, 7], [9], SamplingParams(temperature=0.7, top_p=0.9, top_k=50), 11), [4, 2, 7]),
        "other": (seq([20, 21, 22, 23, 24], [25, 26, 27], SamplingParams(), 99), [0, 10]),
        "ban": (seq(list(range(100, 170)), [3],
                    SamplingParams(do_sample=False, repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=4,
                                   stop_token_ids=(19, 17)), 2 ** 40 + 5, hist_row=1), [1, 6, 3]),
        "pen": (seq([8, 9, 10, 11], [12, 13],
                    SamplingParams(top_k=100, presence_penalty=0.5, frequency_penalty=-1.25,
                                   logit_bias=((3, 1.5), (40, -2.0))), 7, hist_row=0), [5]),
        "lp": (seq([1, 2], [], SamplingParams(temperature=1.0, top_p=1.0, top_k=1, logprobs=3), 3), [9, 8]),
    }


# variant: (processors, penalties, logprobs, the step's two rows, their rows in the in-flight step or None)
VARIANTS = {
    "plain": (False, False, False, ("plain", "other"), (-1, 0)),
    "proc": (True, False, False, ("ban", "plain"), None),
    "proc_lp": (True, False, True, ("ban", "lp"), (1, -1)),
    "pen": (True, True, False, ("pen", "ban"), None),
    "pen_lp": (True, True, True, ("lp", "pen"), (-1, 0)),
}

# The blocks the engine's packing functions produced for these steps before StepLayout replaced them (recorded once
# from them). Rows 4 with 3 blocks: 4n + n * MB is even, no pad word; rows 3: odd, one pad word before the seeds.
EXPECTED = {
    (4, "plain"): [9, 0, 0, 0, 3, 8, 0, 0, 259, 8, 0, 0, 4, 9, 1, 1, 4, 2, 7, 0, 10, 0, 0, 0, 0, 0, 0, 0, 11, 0, 99, 0,
                   0, 0, 0, 0, 1060320051, 1060320051, 0, 0, 1063675494, 1063675494, 1065353216, 1065353216, 50, 50, 1,
                   1, 1, 4, 0, 0, -1, 0, -1, -1],
    (4, "proc"): [3, 9, 0, 0, 70, 3, 0, 0, 390, 259, 0, 0, 71, 4, 1, 1, 1, 6, 3, 4, 2, 7, 0, 0, 0, 0, 0, 0, 5, 256, 11,
                  0, 0, 0, 0, 0, 0, 1060320051, 0, 0, 1063675494, 1063675494, 1065353216, 1065353216, 50, 50, 1, 1, 1,
                  1, 0, 0, -1, -1, -1, -1, 1, -1, -1, -1, 1067869798, 1065353216, 1065353216, 1065353216, 3, 0, 0, 0, 3,
                  0, 0, 0, 2, 17, 19, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                  0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    (4, "proc_lp"): [0, 2, 0, 0, 71, 1, 0, 0, 391, 577, 0, 0, 72, 2, 1, 1, 1, 6, 3, 9, 8, 0, 0, 0, 0, 0, 0, 0, 5, 256,
                     3, 0, 0, 0, 0, 0, 0, 1065353216, 0, 0, 1063675494, 1065353216, 1065353216, 1065353216, 50, 1, 1, 1,
                     2, 0, 0, 0, 1, -1, -1, -1, 1, -1, -1, -1, 1067869798, 1065353216, 1065353216, 1065353216, 3, 0, 0,
                     0, 3, 0, 0, 0, 2, 17, 19, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                     0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                     0, 0, 0, 0, -1, 3, -1, -1],
    (4, "pen"): [13, 3, 0, 0, 5, 70, 0, 0, 325, 390, 0, 0, 6, 71, 1, 1, 5, 0, 0, 1, 6, 3, 0, 0, 0, 0, 0, 0, 7, 0, 5,
                 256, 0, 0, 0, 0, 1060320051, 0, 0, 0, 1063675494, 1063675494, 1065353216, 1065353216, 64, 50, 1, 1, 2,
                 1, 0, 0, -1, -1, -1, -1, 0, 1, -1, -1, 1065353216, 1067869798, 1065353216, 1065353216, 0, 3, 0, 0, 0,
                 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 17, 19, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4,
                 70, 0, 0, 1056964608, 0, 0, 0, -1080033280, 0, 0, 0, 2, 0, 0, 0],
    (4, "pen_lp"): [2, 0, 0, 0, 1, 6, 0, 0, 577, 326, 0, 0, 2, 7, 1, 1, 9, 8, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 7, 0,
                    0, 0, 0, 0, 1065353216, 1060320051, 0, 0, 1065353216, 1063675494, 1065353216, 1065353216, 1, 64, 1,
                    1, 0, 3, 0, 0, -1, 0, -1, -1, -1, 0, -1, -1, 1065353216, 1065353216, 1065353216, 1065353216, 0, 0,
                    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                    0, 0, 0, 0, 0, 4, 0, 0, 0, 1056964608, 0, 0, 0, -1080033280, 0, 0, 0, 2, 0, 0, 3, -1, -1, -1],
    (3, "plain"): [9, 0, 0, 3, 8, 0, 259, 8, 0, 4, 9, 1, 4, 2, 7, 0, 10, 0, 0, 0, 0, 0, 11, 0, 99, 0, 0, 0, 1060320051,
                   1060320051, 0, 1063675494, 1063675494, 1065353216, 50, 50, 1, 1, 4, 0, -1, 0, -1],
    (3, "proc"): [3, 9, 0, 70, 3, 0, 390, 259, 0, 71, 4, 1, 1, 6, 3, 4, 2, 7, 0, 0, 0, 0, 5, 256, 11, 0, 0, 0, 0,
                  1060320051, 0, 1063675494, 1063675494, 1065353216, 50, 50, 1, 1, 1, 0, -1, -1, -1, 1, -1, -1,
                  1067869798, 1065353216, 1065353216, 3, 0, 0, 3, 0, 0, 2, 17, 19, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                  0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    (3, "proc_lp"): [0, 2, 0, 71, 1, 0, 391, 577, 0, 72, 2, 1, 1, 6, 3, 9, 8, 0, 0, 0, 0, 0, 5, 256, 3, 0, 0, 0, 0,
                     1065353216, 0, 1063675494, 1065353216, 1065353216, 50, 1, 1, 2, 0, 0, 1, -1, -1, 1, -1, -1,
                     1067869798, 1065353216, 1065353216, 3, 0, 0, 3, 0, 0, 2, 17, 19, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                     0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                     0, -1, 3, -1],
    (3, "pen"): [13, 3, 0, 5, 70, 0, 325, 390, 0, 6, 71, 1, 5, 0, 0, 1, 6, 3, 0, 0, 0, 0, 7, 0, 5, 256, 0, 0,
                 1060320051, 0, 0, 1063675494, 1063675494, 1065353216, 64, 50, 1, 2, 1, 0, -1, -1, -1, 0, 1, -1,
                 1065353216, 1067869798, 1065353216, 0, 3, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                 2, 17, 19, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4,
                 70, 0, 1056964608, 0, 0, -1080033280, 0, 0, 2, 0, 0],
    (3, "pen_lp"): [2, 0, 0, 1, 6, 0, 577, 326, 0, 2, 7, 1, 9, 8, 0, 5, 0, 0, 0, 0, 0, 0, 3, 0, 7, 0, 0, 0, 1065353216,
                    1060320051, 0, 1065353216, 1063675494, 1065353216, 1, 64, 1, 0, 3, 0, -1, 0, -1, -1, 0, -1,
                    1065353216, 1065353216, 1065353216, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                    0, 4, 0, 0, 1056964608, 0, 0, -1080033280, 0, 0, 2, 0, 3, -1, -1],
}


def _pack(n, variant):
    proc, pen, lp, names, carried = VARIANTS[variant]
    seqs = _seqs()
    tables = {id(s): t for s, t in seqs.values()}

    def bt_row(s, blocks):
        t = tables[id(s)]
        assert blocks <= len(t)  # the row covers the position the step writes
        return np.asarray(t + [0] * (MB - len(t)), dtype=np.int32)

    layout = StepLayout(n, MB, proc, pen, lp)
    host = layout.pack([seqs[k][0] for k in names], carried, top_k_cap=K,
                       stop_ids=lambda p: sorted(EOS | set(p.stop_token_ids)), bt_row=bt_row)
    return layout, host


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n", [4, 3])
def test_packed_block_is_word_for_word_the_recorded_one(n, variant):
    layout, host = _pack(n, variant)
    proc, pen, lp = VARIANTS[variant][:3]
    meta = 4 * n + n * MB
    assert (meta % 2 == 1) == (n == 3)  # the second case has the pad word
    assert layout.words == meta + meta % 2 + 7 * n + ((4 + BAN_IDS_MAX) * n if proc else 0) + (4 * n if pen else 0) \
        + (n if lp else 0)
    assert host.dtype == np.int32 and host.shape == (layout.words,)
    assert host.tolist() == EXPECTED[(n, variant)]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n", [4, 3])
def test_named_views_read_back_what_went_in(n, variant):
    """Through the numpy views of the host array and the torch views of a tensor of it (what the graphs and the
    eager paths read): values, the float32 / int64 reinterpretations and the [n, *] shapes."""
    layout, host = _pack(n, variant)
    proc, pen, lp, names, carried = VARIANTS[variant]
    seqs = [_seqs()[k] for k in names]
    c = [0, 0] if carried is None else [int(r >= 0) for r in carried]
    pad = n - 2
    pos = [s.length - 1 + ci for (s, _), ci in zip(seqs, c)]
    want = dict(
        ids=[0 if ci else s.token_at(q) for (s, _), q, ci in zip(seqs, pos, c)] + [0] * pad,
        pos=pos + [0] * pad,
        slots=[t[q // BLOCK] * BLOCK + q % BLOCK for (_, t), q in zip(seqs, pos)] + [0] * pad,
        kv_lens=[q + 1 for q in pos] + [1] * pad,
        block_table=[t + [0] * (MB - len(t)) for _, t in seqs] + [[0] * MB] * pad,
        seeds=[s.seed for s, _ in seqs] + [0] * pad,
        temps=[s.params.temperature if s.params.do_sample else 0.0 for s, _ in seqs] + [0.0] * pad,
        top_p=[s.params.top_p for s, _ in seqs] + [1.0] * pad,
        top_k=[s.params.top_k if s.params.top_k <= K else K for s, _ in seqs] + [1] * pad,
        steps=[len(s.out) + ci for (s, _), ci in zip(seqs, c)] + [0] * pad,
        carry=list(carried or (-1, -1)) + [-1] * pad,
    )
    if proc:
        on = [s.hist_row >= 0 for s, _ in seqs]
        ban = [sorted(EOS | set(s.params.stop_token_ids))
               if o and len(s.out) + ci < s.params.min_new_tokens else [] for (s, _), o, ci in zip(seqs, on, c)]
        want.update(
            rows=[s.hist_row for s, _ in seqs] + [-1] * pad,
            penalty=[s.params.repetition_penalty if o else 1.0 for (s, _), o in zip(seqs, on)] + [1.0] * pad,
            ngram=[s.params.no_repeat_ngram_size if o else 0 for (s, _), o in zip(seqs, on)] + [0] * pad,
            ban_count=[len(b) for b in ban] + [0] * pad,
            ban_ids=[b + [0] * (BAN_IDS_MAX - len(b)) for b in ban] + [[0] * BAN_IDS_MAX] * pad,
        )
    if pen:
        want.update(
            gen_start=[len(s.prompt) if o else 0 for (s, _), o in zip(seqs, on)] + [0] * pad,
            presence=[s.params.presence_penalty if o else 0.0 for (s, _), o in zip(seqs, on)] + [0.0] * pad,
            frequency=[s.params.frequency_penalty if o else 0.0 for (s, _), o in zip(seqs, on)] + [0.0] * pad,
            bias_count=[len(s.params.logit_bias) if o else 0 for (s, _), o in zip(seqs, on)] + [0] * pad,
        )
    if lp:
        want["nlp"] = [s.params.logprobs if s.logprobs is not None else -1 for s, _ in seqs] + [-1] * pad
    f32 = {"temps", "top_p", "penalty", "presence", "frequency"}
    shapes = {"block_table": (n, MB), "ban_ids": (n, BAN_IDS_MAX)}
    for views, lib in ((layout.views(host), np), (layout.views(torch.from_numpy(host.copy())), torch)):
        assert set(views) == set(want)
        for name, v in views.items():
            dtype = lib.float32 if name in f32 else lib.int64 if name == "seeds" else lib.int32
            assert v.dtype == dtype and tuple(v.shape) == shapes.get(name, (n,)), name
            exp = np.asarray(want[name], dtype=np.float32 if name in f32 else np.int64)
            assert np.array_equal(np.asarray(v), exp), name
    # a view is a view: a word written through it lands in the buffer at the section's place
    t = torch.zeros(layout.words, dtype=torch.int32)
    layout.views(t)["carry"][n - 1] = 7
    assert int(t[4 * n + n * MB + (4 * n + n * MB) % 2 + 7 * n - 1]) == 7 and int(t.sum()) == 7


def test_the_cases_cover_every_kind_of_row():
    s = _seqs()
    assert s["ban"][0].params.uses_processors() and not s["ban"][0].params.uses_penalties()
    assert s["pen"][0].params.uses_penalties() and len(s["pen"][0].params.logit_bias) == 2
    assert s["lp"][0].logprobs is not None and not s["plain"][0].params.uses_processors()
    assert s["ban"][0].length - 1 >= BLOCK  # its slot comes from the second block of its table
    assert any(c is not None and max(c) >= 0 for *_, c in VARIANTS.values())  # carried rows
    assert F(1.3) == 1067869798 and F(-1.25) == -1080033280  # the float words of the recorded blocks


def test_a_block_without_block_table_and_an_empty_step():
    """max_blocks = 0 (the eager sampling of prefill's rows): no table, no slots, everything else as usual; a
    block packed for no sequence is all padding."""
    seqs = _seqs()
    lay = StepLayout(2, 0, True, True, True)
    v = lay.views(lay.pack([seqs["pen"][0], seqs["lp"][0]], top_k_cap=K, stop_ids=lambda p: [2]))
    assert v["block_table"].shape == (2, 0) and v["slots"].tolist() == [0, 0] and v["ids"].tolist() == [0, 0]
    assert v["pos"].tolist() == [5, 1] and v["rows"].tolist() == [0, -1] and v["nlp"].tolist() == [-1, 3]
    assert v["bias_count"].tolist() == [2, 0] and v["seeds"].tolist() == [7, 3]
    empty = StepLayout(2, MB, True).pack([], top_k_cap=K, stop_ids=None)
    v = StepLayout(2, MB, True).views(empty)
    assert v["kv_lens"].tolist() == [1, 1] and v["rows"].tolist() == [-1, -1] and v["carry"].tolist() == [-1, -1]


def test_graph_keys():
    keys = {graph_key(8, *f) for f in itertools.product((False, True), repeat=3)}
    assert len(keys) == 6 and all(isinstance(k, GraphKey) for k in keys)
    assert all(k.processors for k in keys if k.penalties)
    assert graph_key(8) == GraphKey(8, False, False, False) == (8, False, False, False)
    assert graph_key(8, penalties=True) == GraphKey(8, True, False, True)
    assert graph_key(np.int64(8), 1, 0, 0) == GraphKey(8, True) and type(graph_key(np.int64(8)).bucket) is int
    lay = StepLayout(4, MB, penalties=True)
    assert lay.processors and lay.words == StepLayout(4, MB, True, True).words
