"""Presence / frequency penalties and logit_bias on the GPU: ragk_logits_process_pen bit-for-bit against the torch
backend inside canary frames (sentinel columns and rows around the logits, poison in the history cells and bias
table cells nobody may read), the old entry point unchanged, and the engine with the penalty form inside its own
decode-graph variant (graph vs eager vs async, vs the CPU oracle, the other variants untouched)."""
import dataclasses

import pytest
import torch

import logits_proc_cases as C
import penalties_cases as P
from rag_llm_k8s_amd.engine.llm_engine import LLMEngine, SamplingParams
from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights, llama_tiny
from rag_llm_k8s_amd.utils.synthetic import llama_state_dict

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5  # canary value of the columns past V and of the rows around the batch
GPU_LOGITS_REL_TOL = 3e-2  # tests/test_logprobs_gpu.py: logprobs are held to twice it (relative norm)
R = 12  # history rows of the kernel cases


def _launch(native, case, pad=13, gen_bound=None, old=False):
    """One launch on the case inside a canary frame. Returns (frame, hist, bias_ids, bias_vals) on the CPU."""
    B, V = case["logits"].shape
    frame = torch.full((B + 2, V + pad), SENTINEL)
    frame[1:1 + B, :V] = case["logits"]
    d = frame.cuda()
    hist = case["hist"].cuda()
    dev = {k: case[k].cuda() for k in ("rows", "pos", "penalty", "ngram", "ban_ids", "ban_count")}
    ids = None if case["ids"] is None else case["ids"].cuda()
    kw = {}
    if not old:
        kw = {k: case[k].cuda() for k in P.KEYS}
        kw["gen_bound"] = P.gen_bound(case) if gen_bound is None else gen_bound
    native.logits_process(d[1:1 + B, :V], case["vocab_offset"], ids, dev["rows"], dev["pos"], hist, dev["penalty"],
                          dev["ngram"], dev["ban_ids"], dev["ban_count"], **kw)
    torch.cuda.synchronize()
    tables = (kw["bias_ids"].cpu(), kw["bias_vals"].cpu()) if kw else (None, None)
    return (d.cpu(), hist.cpu()) + tables


def _run(native, case, pad=13):
    """The whole frame, the whole history buffer and the bias tables must equal the torch backend's result.
    Returns the processed logits (CPU)."""
    B, V = case["logits"].shape
    got, hist, bi, bv = _launch(native, case, pad)
    want_l, want_h = P.reference(case)
    want = torch.full((B + 2, V + pad), SENTINEL)
    want[1:1 + B, :V] = want_l
    assert torch.equal(got[0], want[0]) and torch.equal(got[-1], want[-1]) and torch.equal(got[:, V:], want[:, V:])
    bad = (got != want) & ~(torch.isnan(got) & torch.isnan(want))
    assert not bool(bad.any()), bad.nonzero()[:8].tolist()
    assert torch.equal(got, want)
    assert torch.equal(hist, want_h)
    assert torch.equal(bi, case["bias_ids"]) and torch.equal(bv, case["bias_vals"])  # the tables are only read
    return got[1:1 + B, :V]


def _rand_seq(L, lo, hi, seed):
    return torch.randint(lo, hi, (L,), generator=torch.Generator().manual_seed(seed)).tolist()


SPANS = (0, 1, 2, 63, 64, 65, 150, 1025)
ROWS8 = [6, 0, 3, 11, 8, 2, 5, 9]


@pytest.mark.parametrize("V", [1001, 4099])
@pytest.mark.parametrize("g0", [0, 7])
def test_generated_spans_and_canaries(native, V, g0):
    """Generated spans 0, 1, 2, 63, 64, 65, 150, 1025 in one launch of 8 rows scattered over a 12-row history, all
    six processors on; with g0 = 7 the prompt holds ids the span never does, and they stay untouched. A span of 0
    behind an empty prompt is no row at all, so that one gets a one-token prompt."""
    seqs = []
    for i, n in enumerate(SPANS):
        prompt = _rand_seq(max(g0, 1 if n == 0 else 0), V - 40, V, 100 * i + g0)  # prompt ids: the top 40
        seqs.append(prompt + _rand_seq(n, 2, min(V - 40, 300), 10 * V + n))
    starts = [len(s) - n for s, n in zip(seqs, SPANS)]
    x = C.make_logits(len(SPANS), V, V + g0)
    bias = [{2: 1.5, 5: -100.0, V - 1: 100.0, V - 41: 0.25} if i % 2 else {} for i in range(len(SPANS))]
    case = P.make_case(x, seqs, starts, [0.4, -0.3, 0.0, 1.0, 2.0, -2.0, 0.6, 0.1],
                       [0.7, 0.0, 1.1, -0.5, 2.0, -2.0, 0.3, 0.9], bias=bias, penalty=1.3, ngram=3,
                       bans=[[3, V - 1, 17]] * len(SPANS), rows=ROWS8, hist_rows=R)
    out = _run(native, case)
    assert not torch.equal(out, x)
    plain = P.reference(dict(case, presence=torch.zeros(8), frequency=torch.zeros(8)))[0]
    assert not torch.equal(out[3:], plain[3:])  # the penalties did something
    if g0:
        quiet = P.make_case(x, seqs, starts, 0.5, 0.5, rows=ROWS8, hist_rows=R)  # penalties alone
        out = _run(native, quiet)
        for b, s in enumerate(seqs):
            only_prompt = sorted(set(s[:starts[b]]) - set(s[starts[b]:]))
            assert only_prompt and torch.equal(out[b, only_prompt], x[b, only_prompt])


def test_span_8192_one_id_all_distinct_and_long_prompts(native):
    """The largest span, V = 8209: the whole span one id (count 8192), 8192 distinct ids (the table at load 1/2),
    random ids behind prompts of 1 and of 5200 tokens, and a span of 8192 with gen_start 0."""
    V, N = 8209, P.GEN_MAX
    distinct = (torch.randperm(V - 2, generator=torch.Generator().manual_seed(1)) + 2)[:N].tolist()
    seqs = [[9] * N, distinct, [V - 1] + _rand_seq(N, 2, 700, 3), _rand_seq(5200, 4000, V, 4) + _rand_seq(N, 2, 3000, 5),
            [4001] * 5200 + [9] * N]
    starts = [0, 0, 1, 5200, 5200]
    x = C.make_logits(5, V, 77)
    x[0, 9], x[4, 9], x[4, 4001] = 3.5, -1.25, 2.0
    case = P.make_case(x, seqs, starts, [0.25, -0.5, 0.0, 1.0, 2.0], [0.5, 0.125, -1.5, 0.3, 2.0],
                       bias=[{9: 10.0}, {}, {}, {2: -3.0}, {}], penalty=[1.0, 1.3, 1.0, 1.2, 1.0], ngram=[0, 0, 2, 0, 0],
                       rows=[10, 1, 4, 7, 0], hist_rows=R)
    assert P.gen_bound(case) == N
    out = _run(native, case)
    f32 = torch.float32
    assert out[0, 9] == ((torch.tensor(3.5) + 10.0) - torch.tensor(0.5, dtype=f32) * 8192.0) - 0.25
    assert out[4, 9] == (torch.tensor(-1.25) - torch.tensor(2.0) * 8192.0) - 2.0 and out[4, 4001] == 2.0
    changed = (out[1] != x[1]) & torch.isfinite(x[1])
    assert int(changed.sum()) == int(torch.isfinite(x[1, distinct]).sum())


def test_one_more_generated_token_is_refused(native):
    """gen_bound 8193: refused with no launch. A row whose real span is over the bound: refused as well."""
    V, N = 1001, P.GEN_MAX
    case = P.make_case(C.make_logits(1, V, 1), [[5, 6, 7] * 10], 0, 0.5, 0.5, rows=[1], hist_rows=2)
    for bound in (N + 1, 29):
        d = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
        before = d["logits"].clone()
        with pytest.raises(ValueError):
            native.logits_process(d["logits"], 0, None, d["rows"], d["pos"], d["hist"], d["penalty"], d["ngram"],
                                  d["ban_ids"], d["ban_count"], gen_bound=bound, **{k: d[k] for k in P.KEYS})
        torch.cuda.synchronize()
        assert torch.equal(d["logits"], before)
    for bad in (dict(gen_start=torch.tensor([31], dtype=torch.int32)), dict(gen_start=torch.tensor([-1], dtype=torch.int32)),
                dict(bias_count=torch.tensor([301], dtype=torch.int32)),
                dict(bias_ids=case["bias_ids"][:1].contiguous()), dict(presence=torch.zeros(1, dtype=torch.float64)),
                dict(frequency=torch.zeros(2)), dict(bias_vals=None)):
        c = dict(case, **bad)
        d = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
        before = d["logits"].clone()
        with pytest.raises(ValueError):
            native.logits_process(d["logits"], 0, None, d["rows"], d["pos"], d["hist"], d["penalty"], d["ngram"],
                                  d["ban_ids"], d["ban_count"], **{k: d[k] for k in P.KEYS})
        torch.cuda.synchronize()
        assert torch.equal(d["logits"], before), bad
    big = P.make_case(C.make_logits(1, V, 2), [[5] * (N + 1)], 0, 0.5, 0.5, rows=[0], hist_rows=1)
    d = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in big.items()}
    with pytest.raises(ValueError):
        native.logits_process(d["logits"], 0, None, d["rows"], d["pos"], d["hist"], d["penalty"], d["ngram"],
                              d["ban_ids"], d["ban_count"], **{k: d[k] for k in P.KEYS})
    _run(native, case)


@pytest.mark.parametrize("V", [1001, 4099])
def test_long_probe_runs(native, V):
    """The hash is multiplicative, not a modulus: ids whose first probes fall on the last two slots of the row's
    table (found with the same hash) make one probe run as long as the span, wrapped over the table's end; in a
    128-slot table (span 64), a 512-slot one (span 150) and with every id twice. Ids a table-size apart as well."""
    run64 = P.colliding_ids(V, P.table_slots(64), 64)
    run150 = P.colliding_ids(V, P.table_slots(150), 150)
    stride = [2 + 128 * i for i in range((V - 2) // 128)]
    seqs = [run64, run150, run64[:32] * 2, list(reversed(run150[:75])) + run150[:75], (stride * 20)[:100]]
    x = C.make_logits(5, V, 5)
    out = _run(native, P.make_case(x, seqs, 0, 0.3, 0.8, rows=[4, 9, 0, 11, 2], hist_rows=R))
    assert int(((out[0] != x[0]) & torch.isfinite(x[0])).sum()) == int(torch.isfinite(x[0, run64]).sum())


@pytest.mark.parametrize("V", [1001, 4099])
def test_bias_entry_counts_edges_and_poison(native, V):
    """0, 1, 299 and 300 entries (the table rows hold poison past the count, and the rows of nobody hold only
    poison); ids 0 and V - 1; biased ids that are also repeated in the span; both penalties zero with a bias."""
    g = torch.Generator().manual_seed(V)
    seqs, bias = [], []
    for n in (0, 1, 299, 300, 300):
        ids = (torch.randperm(V - 2, generator=g)[:n] + 2).tolist()  # never the poison id 1
        if n >= 2:
            ids[0], ids[1] = 0, V - 1
        bias.append({t: float(v) for t, v in zip(ids, (torch.rand(n, generator=g) * 200 - 100).tolist())})
        seqs.append([7, 8] + (ids[:40] * 3 if ids else [5, 5, 6]))
    bias[3][seqs[3][2]] = 100.0
    bias[3][seqs[3][3]] = -100.0
    x = C.make_logits(5, V, 3)
    case = P.make_case(x, seqs, 2, [0.5, 0.5, 0.5, 0.0, 0.0], [0.25, 0.25, -1.0, 0.0, 0.0], bias=bias,
                       penalty=[1.0, 1.0, 1.3, 1.0, 1.3], rows=[3, 10, 0, 7, 5], hist_rows=R)
    assert case["bias_count"].tolist() == [0, 1, 299, 300, 300]
    assert bool((case["bias_ids"][[1, 2, 4, 6, 8, 9, 11]] == C.POISON).all())
    out = _run(native, case)
    assert out[3, 0] == x[3, 0] + torch.tensor(bias[3][0]) and torch.equal(out[:, C.POISON], x[:, C.POISON])
    touched = (out[3] != x[3]) & torch.isfinite(x[3])
    assert set(touched.nonzero().flatten().tolist()) <= set(bias[3])


@pytest.mark.parametrize("V", [1001, 4099])
def test_penalty_kinds_on_every_kind_of_logit(native, V):
    """Presence only, frequency only, both, negative, and zero penalties, each over ids whose logits are positive,
    negative, zero and -inf (which stays -inf)."""
    gen = [10, 11, 12, 13, 10, 10, 11, 13, 13, 13, 13]
    x = C.make_logits(6, V, 9)
    x[:, 10], x[:, 11], x[:, 12], x[:, 13] = 2.5, -3.0, 0.0, float("-inf")
    case = P.make_case(x, [[40, 41] + gen] * 6, 2, [0.7, 0.0, 0.4, -2.0, 0.0, 2.0], [0.0, 0.9, 1.3, -2.0, 0.0, 2.0],
                       rows=[1, 3, 5, 7, 9, 11], hist_rows=R)
    out = _run(native, case)
    assert torch.equal(out[4], x[4]) and bool((out[:, 13] == float("-inf")).all())
    assert out[0, 10] == torch.tensor(2.5) - torch.tensor(0.7) and out[0, 12] == -torch.tensor(0.7)
    assert out[1, 10] == torch.tensor(2.5) - torch.tensor(0.9) * 3.0
    assert out[2, 11] == (torch.tensor(-3.0) - torch.tensor(1.3) * 2.0) - torch.tensor(0.4)
    assert out[3, 10] == (torch.tensor(2.5) + 6.0) + 2.0
    assert torch.equal(out[:, 40:42], x[:, 40:42])  # prompt ids


def test_vocab_shards_concatenate(native):
    """Shards (offset 0, width 501) and (offset 501, width 500) of one case == the unsharded result; bias ids on
    both sides of the cut and at the vocabulary's ends; ids outside a shard leave it untouched."""
    V = 1001
    seqs = [_rand_seq(400, 2, V, 1), [600, 700, 600, 700, 600], [10, 20, 10, 20, 10]]
    x = C.make_logits(3, V, 8)
    bias = [{0: 1.0, 500: -2.0, 501: 3.0, 1000: -4.0, 250: 100.0}, {900: 5.0, 600: -1.0}, {20: 2.0}]
    case = P.make_case(x, seqs, [100, 1, 0], [0.3, 0.5, -0.4], [0.6, 1.0, 0.2], bias=bias, penalty=[1.3, 0.5, 1.3],
                       ngram=[2, 2, 2], bans=[[0, 500, 501, 1000], [900], [100]])
    full = _run(native, case)
    parts = []
    for off, w in ((0, 501), (501, 500)):
        parts.append(_run(native, dict(case, logits=x[:, off:off + w].clone(), vocab_offset=off), pad=7))
    assert torch.equal(torch.cat(parts, 1), full)
    assert torch.equal(parts[0][1], x[1, :501])  # row 1: every history, bias and ban id lives in the upper shard
    assert torch.equal(parts[1][2], x[2, 501:])  # row 2: every id lives in the lower shard


def test_mixed_batch_old_rows_equal_the_old_entry_point(native):
    """Plain rows (-1), rows with the old processors only and rows with the new fields in one launch: the plain rows
    are untouched, the old-only rows are bit-identical to ragk_logits_process on the same inputs."""
    V = 4099
    seqs = [_rand_seq(700, 2, V, 2), None, _rand_seq(33, 2, 60, 3), _rand_seq(257, 2, V, 4), None, [5, 6, 5, 6, 5],
            _rand_seq(300, 2, 50, 6), _rand_seq(64, 2, V, 7)]
    x = C.make_logits(8, V, 9)
    kw = dict(penalty=[1.3, 1.3, 1.0, 0.5, 2.0, 1.0, 1.2, 1.3], ngram=[3, 3, 0, 2, 2, 2, 0, 3],
              bans=[[4, 5], [4, 5], [], [4000], [7], [], [9], []], rows=[9, 0, 4, 1, 0, 7, 11, 2], hist_rows=R)
    new_rows = (2, 6)  # rows 0, 3, 5, 7: old processors only
    case = P.make_case(x, seqs, [0, 0, 3, 0, 0, 0, 100, 0], [0.0, 0.0, 0.5, 0.0, 0.0, 0.0, -1.0, 0.0],
                       [0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 2.0, 0.0], bias=[{}, {}, {}, {}, {}, {}, {3: 4.0, 4098: -9.0}, {}],
                       **kw)
    out = _run(native, case)
    old = C.make_case(x, seqs, kw["penalty"], kw["ngram"], bans=kw["bans"], rows=kw["rows"], hist_rows=R)
    old_out = _launch(native, old, old=True)[0][1:9, :V]
    assert torch.equal(old_out, C.reference(old)[0])
    for b in range(8):
        if b in new_rows:
            assert not torch.equal(out[b], old_out[b])
        else:
            assert torch.equal(out[b], old_out[b])
    for b in (1, 4):
        assert torch.equal(out[b], x[b])
    assert torch.equal(out[:, C.POISON], x[:, C.POISON])


def test_decode_form_stores_one_history_cell(native):
    """With ids the kernel stores hist[row][pos] = id first (the cell held poison), counts it with the span, and
    writes nothing else in hist."""
    V = 1001
    seqs = [_rand_seq(L, 2, 40, L) for L in (1, 2, 256, 257, 900)] + [None, [8, 9, 8, 9, 8]]
    x = C.make_logits(7, V, 11)
    x[6, 8] = 4.0
    case = P.make_case(x, seqs, [0, 1, 100, 0, 450, 0, 2], 0.5, 0.75, bias=[{3: 1.0}] * 7, penalty=1.3, ngram=2,
                       bans=[[3]] * 7, rows=[3, 8, 0, 5, 1, 2, 6], hist_rows=10, decode=True)
    case["ids"][5] = 77  # the id of a row without history must not be stored anywhere
    out = _run(native, case)
    assert P.reference(case)[1][6, 4] == 8 and case["hist"][6, 4] == C.POISON
    # the stored id is the second generated 8 of row 6: count 2
    assert out[6, 8] == (torch.tensor(4.0) / torch.tensor(1.3) - torch.tensor(0.75) * 2.0) - torch.tensor(0.5)


def test_two_launches_are_bit_identical(native):
    """The slot an id claims may differ from launch to launch; no output may."""
    V = 4099
    seqs = [_rand_seq(5200, 2, V, 1) + _rand_seq(P.GEN_MAX, 2, 900, 2), _rand_seq(150, 2, 40, 3),
            P.colliding_ids(V, 512, 150)]
    x = C.make_logits(3, V, 4)
    case = P.make_case(x, seqs, [5200, 0, 0], [0.3, -0.7, 1.0], [1.7, 0.9, -0.1], bias=[{5: 2.0}, {}, {}], penalty=1.1,
                       rows=[7, 2, 10], hist_rows=R)
    a = _launch(native, case)[0]
    b = _launch(native, case)[0]
    assert torch.equal(a, b)
    _run(native, case)


def test_old_entry_point_unchanged(native):
    """ragk_logits_process (no new keyword) on cases of the logit-processor tests == the torch backend's old chain,
    which the CPU suite pins to the parent's results."""
    V = 1001
    mx = native.logits_proc_max_hist()
    lens = [1, 2, 255, 256, 257, 1025, mx]
    seqs = [_rand_seq(L, 2, 300, 10 * V + L) for L in lens]
    x = C.make_logits(len(lens), V, V)
    for decode in (False, True):
        case = C.make_case(x, seqs, 1.3, 3, bans=[[3, V - 1, 17]] * len(lens), rows=[6, 0, 3, 1, 8, 2, 5], hist_rows=9,
                           ld=mx, decode=decode)
        got, hist = _launch(native, case, old=True)[:2]
        want_l, want_h = C.reference(case)
        assert torch.equal(got[1:-1, :V], want_l) and torch.equal(hist, want_h)
        assert bool((got[0] == SENTINEL).all()) and bool((got[-1] == SENTINEL).all()) and bool((got[:, V:] == SENTINEL).all())


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
        out.append((base * 4)[:n])
    return out


STOP = tuple(range(3, 1000, 67))
BIAS = tuple((t, (-100.0, 6.0, -2.5)[i % 3]) for i, t in enumerate(range(4, 1000, 9)))  # 111 entries


def _mixed_params():
    """Plain rows, rows with the old processors only, rows with the new fields (alone and with the old ones)."""
    old = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=5)
    kinds = [dict(old, frequency_penalty=1.5, presence_penalty=0.5, logit_bias=BIAS), {}, old,
             dict(frequency_penalty=-1.0, presence_penalty=-0.5), dict(logit_bias=BIAS[:7]), {},
             dict(old, presence_penalty=2.0, logprobs=3)]
    return [SamplingParams(max_new_tokens=m, temperature=0.9, top_p=0.95, top_k=50, stop_token_ids=STOP, **k)
            for m, k in zip((12, 5, 20, 7, 16, 6, 9), kinds)]


def _run_mixed(eng, prompts, params):
    seqs = [eng.add_request(pr, pa, seed=10 + i) for i, (pr, pa) in enumerate(zip(prompts, params))]
    eng.run_until_done()
    assert eng._inflight is None and not eng.running
    assert eng.bm.free_blocks() == 64 - 1 and sorted(eng._hist_free) == list(range(eng.max_batch))
    return [(s.out, s.finish_reason, s.logprobs) for s in seqs]


def test_graph_eager_async_sync_identical(native, tiny_llama):
    """Sampled requests of every kind in one schedule (more requests than batch slots, early stops): hipGraph
    decode == eager decode, async pipeline == sync, and a second run on the same engine gives the same tokens.
    stats["penalty_steps"] counts the steps with a penalty row, and only those."""
    cfg, sd = tiny_llama
    prompts, params = _prompts(4, (9, 40, 200, 5, 77, 130, 31)), _mixed_params()
    outs = {}
    for name, graphs, async_ in (("async", True, True), ("sync", True, False), ("eager", False, False)):
        eng = _engine(cfg, sd, "cuda", graphs)
        eng.async_decode = async_ and eng.async_decode
        eng.mixed_steps = False
        outs[name] = _run_mixed(eng, prompts, params)
        assert 0 < eng.stats["penalty_steps"] <= eng.stats["logit_proc_steps"]
        if name == "async":
            assert any(k.penalties for k in eng.graphs)  # the penalty variant was captured and replayed
            outs["again"] = _run_mixed(eng, prompts, params)
    tok = {k: [(o, r) for o, r, _ in v] for k, v in outs.items()}
    assert tok["async"] == tok["sync"] == tok["eager"] == tok["again"]
    assert outs["async"][6][2] == outs["sync"][6][2] == outs["again"][6][2]  # logprob values: graph paths agree
    banned = {t for t, v in BIAS if v == -100.0}
    assert not banned & set(outs["async"][0][0])
    assert not {t for t, v in BIAS[:7] if v == -100.0} & set(outs["async"][4][0])


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


def test_gpu_greedy_and_logprobs_vs_cpu_oracle(native, tiny_llama):
    """The comparison of test_logits_proc_gpu's greedy test (teacher forced on the GPU's own tokens; every token the
    oracle's argmax or within 0.02 x the row's finite logit spread of it, the -100 entries left out of the spread)
    with the oracle's row passed through the torch backend's full chain first, and the logprobs (chosen and alternatives) against log_softmax of that row
    within twice the GPU-vs-CPU logits tolerance (relative norm), as tests/test_logprobs_gpu.py holds them."""
    cfg, sd = tiny_llama
    prompts = _prompts(0, (5, 77, 130, 300, 513))
    eng = _engine(cfg, sd, "cuda", True, mb=8)
    plain = eng.generate(prompts, SamplingParams(max_new_tokens=2, do_sample=False, ignore_eos=True))
    bias = {o[0]: -100.0 for o in plain}
    bias.update({o[1]: 4.0 for o in plain if o[1] not in bias})
    p = SamplingParams(max_new_tokens=10, do_sample=False, ignore_eos=True, repetition_penalty=1.2,
                       frequency_penalty=1.5, presence_penalty=-0.75, logit_bias=tuple(sorted(bias.items())),
                       logprobs=5)
    seqs = [eng.add_request(pr, p, seed=1) for pr in prompts]
    eng.run_until_done()
    assert eng.stats["penalty_steps"] >= 10
    exact = total = 0
    got, want, got_alt, want_alt = [], [], [], []
    down = sorted(t for t, v in bias.items() if v < 0)
    for pr, s, pl in zip(prompts, seqs, plain):
        out = s.out
        assert len(out) == 10 and out[0] != pl[0] and not set(down) & set(out)
        lg = _oracle_logits(cfg, sd, pr + out[:-1])
        for k, tok in enumerate(out):
            row = lg[len(pr) - 1 + k].clone()[None]
            case = P.make_case(row, [pr + out[:k]], len(pr), -0.75, 1.5, bias=[bias], penalty=1.2)
            row = P.reference(case)[0][0]
            top = float(row.max())
            gap = top - float(row[tok])
            keep = torch.isfinite(row)
            keep[down] = False  # the -100 entries would stretch the spread the tolerance is taken from
            spread = top - float(row[keep].min())
            assert gap <= 0.02 * spread, (k, tok, int(row.argmax()), gap, spread)
            exact += int(gap == 0.0)
            total += 1
            ref = torch.log_softmax(row, 0)
            assert s.top_logprobs[k][0] == (tok, s.logprobs[k])
            got.append(s.logprobs[k]), want.append(float(ref[tok]))
            for i, v in s.top_logprobs[k]:
                got_alt.append(v), want_alt.append(float(ref[i]))
    assert exact >= 0.7 * total, (exact, total)
    for a, b, what in ((got, want, "chosen"), (got_alt, want_alt, "alternatives")):
        a, b = torch.tensor(a), torch.tensor(b)
        rel = float((a - b).norm() / b.norm())
        print("%s logprobs with penalties, GPU engine vs CPU oracle: rel %.5f" % (what, rel))
        assert rel < 2 * GPU_LOGITS_REL_TOL, (what, rel)


def test_eos_bias_keeps_every_sequence_running(native, tiny_llama):
    """logit_bias {eos: -100} for every id plain decoding stops on, ignore_eos off: no sequence stops before
    max_new_tokens (without the bias every one stops at its first token)."""
    cfg, sd = tiny_llama
    prompts = _prompts(0, (5, 77, 130, 300))
    eng = _engine(cfg, sd, "cuda", True, mb=4)
    plain = eng.generate(prompts, SamplingParams(max_new_tokens=1, do_sample=False, ignore_eos=True))
    eos = sorted({o[0] for o in plain})
    eng = _engine(cfg, sd, "cuda", True, mb=4, eos_ids=eos)
    early = [eng.add_request(pr, SamplingParams(max_new_tokens=12, do_sample=False), seed=1) for pr in prompts]
    eng.run_until_done()
    assert all(s.finish_reason == "stop" and len(s.out) == 1 for s in early)
    p = SamplingParams(max_new_tokens=12, temperature=0.9, top_p=0.95, top_k=50,
                       logit_bias=tuple((t, -100.0) for t in eos))
    seqs = [eng.add_request(pr, p, seed=3 + i) for i, pr in enumerate(prompts)]
    eng.run_until_done()
    assert all(s.finish_reason == "length" and len(s.out) == 12 and not set(eos) & set(s.out) for s in seqs)


def test_other_graph_variants_untouched_by_a_penalty_request(native, tiny_llama):
    """Plain and old-processor batches before and after a penalty request on one engine: identical tokens, the
    (B, False) and (B, True) entries the same objects, the penalty variant under a key of its own."""
    cfg, sd = tiny_llama
    prompts = _prompts(7, (9, 40, 200))
    p = SamplingParams(max_new_tokens=8, temperature=0.8, top_p=0.9, top_k=40, ignore_eos=True)
    q = dataclasses.replace(p, repetition_penalty=1.3, no_repeat_ngram_size=2)
    eng = _engine(cfg, sd, "cuda", True)
    a = eng.generate(prompts, p, seeds=[1, 2, 3])
    b = eng.generate(prompts[:2], q, seeds=[4, 5])
    assert eng.stats["penalty_steps"] == 0 and not any(k.logprobs or k.penalties for k in eng.graphs)
    assert {k.processors for k in eng.graphs} == {False, True}
    entries = dict(eng.graphs)
    n_proc = eng.stats["logit_proc_steps"]
    eng.generate(prompts[:2], dataclasses.replace(q, frequency_penalty=1.0, logit_bias=((5, 1.0),)), seeds=[4, 5])
    eng.generate(prompts[:1], dataclasses.replace(p, presence_penalty=1.0, logprobs=2), seeds=[6])
    n_pen = eng.stats["penalty_steps"]
    new = set(eng.graphs) - set(entries)
    assert n_pen >= 14 and new and all(k.processors is True and k.penalties is True for k in new)
    assert {k.logprobs for k in new} == {False, True}
    assert eng.stats["logit_proc_steps"] == n_proc + n_pen
    assert eng.generate(prompts, p, seeds=[1, 2, 3]) == a and eng.generate(prompts[:2], q, seeds=[4, 5]) == b
    assert eng.stats["penalty_steps"] == n_pen
    assert all(eng.graphs[k] is v for k, v in entries.items())
