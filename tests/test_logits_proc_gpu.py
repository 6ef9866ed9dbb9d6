"""History-dependent logit processors on the GPU: ragk_logits_process / ragk_hist_write bit-for-bit against the
torch backend (canary columns and rows around the logits, poison in the history cells nobody may read), and the
engine with the processors inside the decode graph (graph vs eager, async vs sync, vs the CPU oracle, the
default path untouched)."""
import pytest
import torch

import logits_proc_cases as C
from rag_llm_k8s_amd.engine.llm_engine import LLMEngine, SamplingParams
from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights, llama_tiny
from rag_llm_k8s_amd.utils.synthetic import llama_state_dict

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5  # canary value of the columns past V and of the rows around the batch


def _run(native, case, pad=13):
    """Run the kernel on the case inside a canary frame; the whole frame and the whole history buffer must equal
    the torch backend's result. Returns the processed logits (CPU)."""
    B, V = case["logits"].shape
    frame = torch.full((B + 2, V + pad), SENTINEL)
    frame[1:1 + B, :V] = case["logits"]
    d = frame.cuda()
    hist = case["hist"].cuda()
    dev = {k: case[k].cuda() for k in ("rows", "pos", "penalty", "ngram", "ban_ids", "ban_count")}
    ids = None if case["ids"] is None else case["ids"].cuda()
    native.logits_process(d[1:1 + B, :V], case["vocab_offset"], ids, dev["rows"], dev["pos"], hist, dev["penalty"],
                          dev["ngram"], dev["ban_ids"], dev["ban_count"])
    torch.cuda.synchronize()
    want_l, want_h = C.reference(case)
    want = frame.clone()
    want[1:1 + B, :V] = want_l
    got = d.cpu()
    assert torch.equal(got[0], want[0]) and torch.equal(got[-1], want[-1]) and torch.equal(got[:, V:], want[:, V:])
    assert torch.equal(got, want)
    assert torch.equal(hist.cpu(), want_h)
    return got[1:1 + B, :V]


def _rand_seq(L, V, seed):
    return torch.randint(2, V, (L,), generator=torch.Generator().manual_seed(seed)).tolist()


@pytest.mark.parametrize("V", [1001, 4099])
def test_history_lengths_and_canaries(native, V):
    """Lengths 1, 2, 255, 256, 257, 1025 and the largest the wrapper accepts, all three processors on."""
    mx = native.logits_proc_max_hist()
    lens = [1, 2, 255, 256, 257, 1025, mx]
    seqs = [_rand_seq(L, min(V, 300), 10 * V + L) for L in lens]
    x = C.make_logits(len(lens), V, V)
    case = C.make_case(x, seqs, 1.3, 3, bans=[[3, V - 1, 17]] * len(lens), rows=[6, 0, 3, 1, 8, 2, 5],
                       hist_rows=9, ld=mx)
    out = _run(native, case)
    assert not torch.equal(out, x)


def test_history_wider_than_the_staging_is_refused(native):
    mx = native.logits_proc_max_hist()
    case = C.make_case(C.make_logits(1, 1001, 1), [[5, 6, 7]], 1.3, 2, hist_rows=2, ld=mx + 1)
    d = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
    before = d["logits"].clone()
    with pytest.raises(ValueError):
        native.logits_process(d["logits"], 0, None, d["rows"], d["pos"], d["hist"], d["penalty"], d["ngram"],
                              d["ban_ids"], d["ban_count"])
    torch.cuda.synchronize()
    assert torch.equal(d["logits"], before)  # refused before any launch
    ok = C.make_case(C.make_logits(1, 1001, 1), [[5, 6, 7]], 1.3, 2, hist_rows=2, ld=mx)
    _run(native, ok)


def test_duplicate_ids_penalised_once(native):
    """One id 300 times, and a cycle through 7 ids: every original logit is read before any is written, so the
    penalty lands once per distinct id."""
    V = 1001
    x = C.make_logits(2, V, 3)
    cyc = [40, 41, 42, 43, 44, 45, 46]
    x[0, 9], x[1, 40], x[1, 41], x[1, 42] = 6.5, -3.0, 2.0, 0.0
    case = C.make_case(x, [[9] * 300, [cyc[i % 7] for i in range(300)]], [1.3, 0.5], 0)
    out = _run(native, case)
    p13, p05 = torch.tensor(1.3, dtype=torch.float32), torch.tensor(0.5, dtype=torch.float32)
    assert out[0, 9] == torch.tensor(6.5) / p13
    assert out[1, 40] == torch.tensor(-3.0) * p05 and out[1, 41] == torch.tensor(2.0) / p05 and out[1, 42] == 0.0
    changed = (out != x) & ~(torch.isinf(out) & torch.isinf(x))
    assert set(changed[0].nonzero().flatten().tolist()) == {9}
    assert set(changed[1].nonzero().flatten().tolist()) <= set(cyc)


@pytest.mark.parametrize("n", list(range(1, 9)))
def test_ngram_ban_every_size(native, n):
    """Lengths n-2, n-1, n and n+5 with suffix matches at j = 0, at the last legal j and at overlapping positions
    (logits_proc_cases.ngram_histories), one launch per n."""
    V = 1001
    seqs = [h for L in (n - 2, n - 1, n, n + 5) if L >= 1 for h in C.ngram_histories(n, L)]
    x = C.make_logits(len(seqs), V, 50 + n)
    x[:, :60] = torch.randn(len(seqs), 60, generator=torch.Generator().manual_seed(n))  # history ids: finite logits
    case = C.make_case(x, seqs, 1.0, n, rows=list(reversed(range(len(seqs)))))
    out = _run(native, case)
    for b, s in enumerate(seqs):  # what must be banned, spelled out: constant history of length >= n bans its id
        if s == [7] * len(s):
            assert torch.isinf(out[b, 7]) == (len(s) >= n)
        assert torch.equal(out[b], C.python_row(x[b], s, 1.0, n, []))


def test_vocab_shards_concatenate(native):
    """Shards (offset 0, width 501) and (offset 501, width 500) of one case == the unsharded result; history ids
    and ban ids outside a shard leave it untouched."""
    V = 1001
    seqs = [_rand_seq(400, V, 1), [600, 700, 600, 700, 600], [10, 20, 10, 20, 10]]
    x = C.make_logits(3, V, 8)
    case = C.make_case(x, seqs, [1.3, 0.5, 1.3], [2, 2, 2], bans=[[0, 500, 501, 1000], [900], [100]])
    full = _run(native, case)
    parts = []
    for off, w in ((0, 501), (501, 500)):
        parts.append(_run(native, dict(case, logits=x[:, off:off + w].clone(), vocab_offset=off), pad=7))
    assert torch.equal(torch.cat(parts, 1), full)
    assert torch.equal(parts[0][1], x[1, :501])  # row 1: every history and ban id lives in the upper shard
    assert torch.equal(parts[1][2], x[2, 501:])  # row 2: every id lives in the lower shard


def test_mixed_rows_scattered_history(native):
    """Rows without a history row (-1) and rows with neutral parameters are bit-identical to their input; active
    rows sit in scattered history rows, the rows between them hold a poison id nobody may read."""
    V = 4099
    seqs = [_rand_seq(700, V, 2), None, _rand_seq(33, V, 3), _rand_seq(257, V, 4), None, [5, 6, 5, 6, 5]]
    x = C.make_logits(6, V, 9)
    case = C.make_case(x, seqs, [1.3, 1.3, 1.0, 0.5, 2.0, 1.0], [3, 3, 0, 2, 2, 2],
                       bans=[[4, 5], [4, 5], [], [4000], [7], []], rows=[9, 0, 4, 1, 0, 7], hist_rows=11)
    out = _run(native, case)
    for b in (1, 2, 4):
        assert torch.equal(out[b], x[b])
    assert torch.equal(out[:, C.POISON], x[:, C.POISON])


def test_decode_form_stores_one_history_cell(native):
    """With ids the kernel stores hist[row][pos] = id first (the cell held poison) and nothing else in hist."""
    V = 1001
    seqs = [_rand_seq(L, 40, L) for L in (1, 2, 256, 257, 900)] + [None, [8, 9, 8, 9, 8]]
    x = C.make_logits(7, V, 11)
    case = C.make_case(x, seqs, 1.3, 2, bans=[[3]] * 7, rows=[3, 8, 0, 5, 1, 2, 6], hist_rows=10, decode=True)
    case["ids"][5] = 77  # the id of a row without history must not be stored anywhere
    _run(native, case)
    assert C.reference(case)[1][6, 4] == 8 and case["hist"][6, 4] == C.POISON


def test_hist_write_scatter(native):
    R, ld, T = 5, 300, 777
    g = torch.Generator().manual_seed(5)
    rows = torch.randint(-1, R, (T,), generator=g, dtype=torch.int32)
    pos = torch.randint(0, ld, (T,), generator=g, dtype=torch.int32)
    key = torch.where(rows >= 0, rows * ld + pos, torch.full_like(rows, -1))
    first = {}
    for i, k in enumerate(key.tolist()):  # one write per cell: the scatter's order is not defined for duplicates
        if k >= 0 and k in first:
            rows[i] = -1
        first.setdefault(k, i)
    ids = torch.randint(2, 100000, (T,), generator=g, dtype=torch.int32)
    hist = torch.full((R, ld), C.POISON, dtype=torch.int32)
    from rag_llm_k8s_amd.ops.backend import TorchBackend

    want = TorchBackend("cpu").hist_write(ids, rows, pos, hist.clone())
    assert (want != C.POISON).sum() == (rows >= 0).sum() > 100 and (rows < 0).sum() > 50
    got = native.hist_write(ids.cuda(), rows.cuda(), pos.cuda(), hist.cuda())
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)


# ----------------------------------------------------------------------------- engine level (tiny model)
def _engine(cfg, sd, device, graphs, mb=4, **kw):
    w = LlamaWeights.from_state_dict(cfg, sd, device)
    m = LlamaModel(cfg, w, device, max_positions=2048)
    return LLMEngine(m, num_blocks=64, max_batch=mb, max_prefill_tokens=300, max_model_len=2048, use_graphs=graphs,
                     **kw)


@pytest.fixture(scope="module")
def tiny_llama():
    cfg = llama_tiny(vocab=1024, layers=2, hidden=512, heads=4, kv_heads=1, inter=512)
    return cfg, llama_state_dict(cfg, seed=3, std=0.05)


def _prompts(seed, lens):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in lens:
        base = torch.randint(3, 1000, (max(3, n // 3),), generator=g).tolist()
        out.append((base * 4)[:n])  # prompts that repeat themselves: the processors have something to do
    return out


STOP = tuple(range(3, 1000, 67))  # 15 stop ids


def _mixed_params():
    proc = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=5, stop_token_ids=STOP)
    return [SamplingParams(max_new_tokens=m, temperature=0.9, top_p=0.95, top_k=50, **(proc if on else
                                                                                       dict(stop_token_ids=STOP)))
            for m, on in ((12, True), (5, False), (20, True), (7, True), (16, False), (6, True), (9, True))]


def _run_mixed(eng, prompts, params):
    seqs = [eng.add_request(pr, pa, seed=10 + i) for i, (pr, pa) in enumerate(zip(prompts, params))]
    eng.run_until_done()
    assert eng._inflight is None and not eng.running
    assert eng.bm.free_blocks() == 64 - 1 and sorted(eng._hist_free) == list(range(eng.max_batch))
    return [(s.out, s.finish_reason) for s in seqs]


def test_graph_eager_async_sync_identical(native, tiny_llama):
    """Sampled requests, processors on for five of seven (more requests than batch slots, early stops): hipGraph
    decode == eager decode, async pipeline == sync, and a second identical run on the engine whose processor
    graphs were captured lazily mid-pipeline gives the same tokens again."""
    cfg, sd = tiny_llama
    prompts, params = _prompts(4, (9, 40, 200, 5, 77, 130, 31)), _mixed_params()
    outs = {}
    for name, graphs, async_ in (("async", True, True), ("sync", True, False), ("eager", False, False)):
        eng = _engine(cfg, sd, "cuda", graphs)
        eng.async_decode = async_ and eng.async_decode
        eng.mixed_steps = False  # as test_e2e_gpu.test_async_decode_equals_sync: isolate the decode pipeline
        outs[name] = _run_mixed(eng, prompts, params)
        assert eng.stats["logit_proc_steps"] > 0
        if name == "async":
            assert any(k.processors for k in eng.graphs) and any(not k.processors for k in eng.graphs)
            outs["again"] = _run_mixed(eng, prompts, params)
    assert outs["async"] == outs["sync"] == outs["eager"] == outs["again"]
    for (out, reason), pr, pa in zip(outs["async"], prompts, params):
        if pa.uses_processors():
            assert reason != "stop" or len(out) >= pa.min_new_tokens
            assert not any(t in STOP for t in out[:pa.min_new_tokens])
            assert C.no_ngram_repeats(pr + out, 3, start=len(pr))


def _oracle_logits(cfg, sd, ids):
    """fp32-accumulating CPU oracle: logits [T, V] of every position of `ids` (one prefill), as test_e2e_gpu."""
    from rag_llm_k8s_amd.models.llama import StepInput
    from rag_llm_k8s_amd.ops.backend import AttnMeta

    eng = _engine(cfg, sd, "cpu", graphs=False)
    n = len(ids)
    eng.bm.ensure(99, n + 1)
    tbl = eng.bm.table(99)
    slots = torch.tensor([tbl[q // 64] * 64 + q % 64 for q in range(n)], dtype=torch.int32)
    bt = torch.tensor([tbl + [0] * (eng.max_blocks - len(tbl))], dtype=torch.int32)
    meta = AttnMeta("prefill", torch.tensor([n], dtype=torch.int32), bt, cu_q=torch.tensor([0, n], dtype=torch.int32),
                    host_kv_lens=[n])
    inp = StepInput(torch.tensor(ids, dtype=torch.int32), torch.arange(n, dtype=torch.int32), slots, meta, None)
    return eng.model.forward(inp).float()


def test_gpu_greedy_with_processors_vs_cpu_oracle(native, tiny_llama):
    """The comparison of test_e2e_gpu._check_greedy (teacher forced on the GPU's own tokens; every token the
    oracle's argmax or within 0.02 x the row's logit spread of it), with the oracle's row passed through the torch
    processors first; the spread is taken over the finite logits (banned ids are -inf). Also, on the returned
    tokens alone: nothing stops before min_new_tokens, no 3-gram is generated twice. Without the processors the
    same prompts stop at their first token (the stop ids are those first tokens)."""
    cfg, sd = tiny_llama
    prompts = _prompts(0, (5, 77, 130, 300, 513))
    eng = _engine(cfg, sd, "cuda", True, mb=8)
    plain = eng.generate(prompts, SamplingParams(max_new_tokens=2, do_sample=False, ignore_eos=True))
    stop = tuple(sorted({o[0] for o in plain}))
    K = 6
    p = SamplingParams(max_new_tokens=10, do_sample=False, stop_token_ids=stop, repetition_penalty=1.3,
                       no_repeat_ngram_size=3, min_new_tokens=K)
    early = [eng.add_request(pr, SamplingParams(max_new_tokens=10, do_sample=False, stop_token_ids=stop), seed=1)
             for pr in prompts]
    eng.run_until_done()
    assert all(s.finish_reason == "stop" and len(s.out) == 1 for s in early)
    seqs = [eng.add_request(pr, p, seed=1) for pr in prompts]
    eng.run_until_done()
    exact = total = 0
    for pr, s in zip(prompts, seqs):
        out = s.out
        assert len(out) >= K and (s.finish_reason != "stop" or out[-1] in stop)
        assert not any(t in stop for t in out[:K])
        assert C.no_ngram_repeats(pr + out, 3, start=len(pr))
        lg = _oracle_logits(cfg, sd, pr + out[:-1])
        for k, tok in enumerate(out):
            seq = pr + out[:k]
            row = lg[len(pr) - 1 + k].clone()[None]
            case = C.make_case(row, [seq], 1.3, 3, bans=[list(stop) if k < K else []])
            row = C.reference(case)[0][0]
            top = float(row.max())
            gap = top - float(row[tok])
            spread = top - float(row[torch.isfinite(row)].min())
            assert gap <= 0.02 * spread, (k, tok, int(row.argmax()), gap, spread)
            exact += int(gap == 0.0)
            total += 1
    assert exact >= 0.7 * total, (exact, total)


def test_default_path_untouched_by_a_processor_request(native, tiny_llama):
    """A batch of plain requests before and after a processor request on the same engine: identical tokens,
    logit_proc_steps unchanged by the plain batch, the (B, False) graph entries the same objects."""
    cfg, sd = tiny_llama
    prompts = _prompts(7, (9, 40, 200))
    p = SamplingParams(max_new_tokens=8, temperature=0.8, top_p=0.9, top_k=40, ignore_eos=True)
    eng = _engine(cfg, sd, "cuda", True)
    a = eng.generate(prompts, p, seeds=[1, 2, 3])
    assert eng.stats["logit_proc_steps"] == 0 and eng._hist is None and all(not k.processors for k in eng.graphs)
    entries = {k: v for k, v in eng.graphs.items()}
    eng.generate(prompts[:2], SamplingParams(max_new_tokens=8, temperature=0.8, top_p=0.9, top_k=40, ignore_eos=True,
                                             repetition_penalty=1.3, no_repeat_ngram_size=2), seeds=[4, 5])
    n = eng.stats["logit_proc_steps"]
    assert n > 0 and any(k.processors for k in eng.graphs)
    b = eng.generate(prompts, p, seeds=[1, 2, 3])
    assert a == b and eng.stats["logit_proc_steps"] == n
    assert all(eng.graphs[k] is v for k, v in entries.items())
