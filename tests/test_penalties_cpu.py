"""Presence / frequency penalties and logit_bias on CPU: the torch backend vs a Counter oracle and transformers'
SequenceBiasLogitsProcessor, the old call unchanged, the engine vs transformers' generate(), discard / recompute,
the bias table across history-row reuse, TP=2 over gloo, admission, and the service / Flask surface."""
import dataclasses
import os
import tempfile

import pytest
import torch

import logits_proc_cases as C
import penalties_cases as P
from rag_llm_k8s_amd.engine.llm_engine import (LOGIT_BIAS_MAX, PENALTY_GEN_MAX, LLMEngine, SamplingParams,
                                               normalize_logit_bias)
from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights
from rag_llm_k8s_amd.utils.synthetic import llama_state_dict
# the tiny model, the HF twin and the service of the logit-processor tests (fixtures included)
from test_logits_proc_cpu import (CFG, WORLD, _engine, _free_port, _hf_generate, _prompt_and_eos, _service,  # noqa: F401
                                  assets, tiny)

V = 211
SPANS = (0, 1, 2, 150, 300)


def _seq(L, lo, hi, seed):
    return torch.randint(lo, hi, (L,), generator=torch.Generator().manual_seed(seed)).tolist()


def test_constants():
    assert (LOGIT_BIAS_MAX, PENALTY_GEN_MAX) == (P.BIAS_W, P.GEN_MAX) == (300, 8192)


# ----------------------------------------------------------------------------- op level
def test_frequency_presence_equal_the_counter_oracle():
    """Generated spans 0, 1, 2, 150, 300 behind prompts of 0 and 40 tokens; one id for the whole span, all ids
    distinct, random ids; positive, negative and one-sided penalties. Prompt-only ids stay bit-identical. The
    logits hold positive, negative, zero and -inf entries, and -inf stays -inf."""
    checked = 0
    for si, span in enumerate(SPANS):
        for g0 in (0, 40):
            prompt = _seq(g0, 150, V, 7 * si + g0)  # prompt ids 150..210, generated ids 2..149: disjoint
            for kind in ("same", "distinct", "random"):
                if kind == "distinct" and span > 148:
                    continue
                gen = {"same": [9] * span, "distinct": list(range(2, 2 + span)),
                       "random": _seq(span, 2, 30, span + g0)}[kind]
                seq = prompt + gen
                if not seq:
                    continue
                x = C.make_logits(1, V, 31 * si + g0)
                if gen:
                    x[0, gen[0]] = (0.0, -2.5, 3.25, float("-inf"))[(si + g0) % 4]
                for f, p in ((0.7, 0.3), (-1.5, -0.25), (0.0, 2.0), (2.0, 0.0), (0.0, 0.0)):
                    case = P.make_case(x, [seq], g0, p, f, rows=[2], hist_rows=4)
                    got, hist = P.reference(case)
                    assert torch.equal(hist, case["hist"])
                    want = P.counter_row(x[0], seq, g0, f, p)
                    assert torch.equal(got[0], want), (span, g0, kind, f, p)
                    untouched = sorted(set(range(V)) - set(gen))
                    assert torch.equal(got[0, untouched], x[0, untouched])  # prompt-only ids among them
                    assert bool(torch.isinf(got[0][torch.isinf(x[0])]).all())
                    if gen and (f, p) != (0.0, 0.0) and torch.isfinite(x[0, gen[0]]):
                        assert got[0, gen[0]] != x[0, gen[0]]
                    checked += 1
    assert checked >= 100
    # count 300 of one id, spelled out
    x = torch.zeros(1, V)
    x[0, 9] = 5.0
    got, _ = P.reference(P.make_case(x, [[9] * 300], 0, 0.5, 0.25))
    assert got[0, 9] == (torch.tensor(5.0) - torch.tensor(0.25) * 300.0) - 0.5


def test_bias_equals_transformers_sequence_bias():
    """0, 1 and 300 entries, +-100, on every kind of logit; the table row's cells past bias_count hold poison."""
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import SequenceBiasLogitsProcessor

    V2 = 1001
    g = torch.Generator().manual_seed(3)
    for n in (0, 1, 2, 299, 300):
        ids = torch.randperm(V2 - 2, generator=g)[:n].add(2).tolist()
        vals = (torch.rand(n, generator=g) * 200 - 100).tolist()
        if n >= 2:
            vals[0], vals[1] = 100.0, -100.0
        bias = dict(zip(ids, vals))
        x = C.make_logits(1, V2, n)
        case = P.make_case(x, [[5, 6, 7]], 3, 0.0, 0.0, bias=[bias], rows=[1], hist_rows=3)
        got, _ = P.reference(case)
        want = x if n == 0 else SequenceBiasLogitsProcessor([[[t], v] for t, v in bias.items()])(
            torch.tensor([[5, 6, 7]]), x.clone())
        assert torch.equal(got, want), n
        assert got[0, C.POISON] == x[0, C.POISON]


def test_full_chain_equals_transformers_chain():
    """SequenceBias -> RepetitionPenalty -> Counter oracle -> NoRepeatNGram -> MinNewTokens, over the spans, with
    an id that is biased, repeated and banned (the ban wins) and +-100 biases."""
    pytest.importorskip("transformers")
    stop = [5, 9, 200]
    checked = 0
    for si, span in enumerate(SPANS):
        for g0 in (1, 40):
            seq = _seq(g0, 2, 40, 5 * si + g0) + ([9, 11] * span)[:span // 2] + _seq(span - span // 2, 2, 40, span)
            x = C.make_logits(1, V, 50 + 3 * si + g0)
            x[0, 9], x[0, 11] = 2.5, -1.5
            bias = {9: 100.0, 11: -100.0, 12: 3.5, 200: -0.75, V - 1: 50.0, 2: -7.0}
            for pen, f, p, n, min_new in ((1.3, 0.7, 0.3, 3, span + 1), (1.0, -0.5, 1.0, 0, 0), (0.5, 0.0, 0.0, 2, 0),
                                          (1.0, 0.0, 0.0, 0, 0), (1.3, 2.0, -2.0, 1, span + 1)):
                bans = stop if span < min_new else []
                case = P.make_case(x, [seq], g0, p, f, bias=[bias], penalty=pen, ngram=n, bans=[bans], rows=[2],
                                   hist_rows=4)
                got, _ = P.reference(case)
                want = P.chain_row(x[0], seq, g0, bias, pen, f, p, n, min_new, stop)
                assert torch.equal(got[0], want), (span, g0, pen, f, p, n, min_new)
                if bans:
                    assert got[0, 9] == float("-inf")  # biased +100, repeated, penalised and banned: the ban wins
                if n == 1 and span >= 2:
                    assert got[0, 11] == float("-inf")
                checked += 1
    assert checked == 50


def test_old_call_unchanged_by_neutral_keywords():
    """Every new keyword None == the old call; zero penalties and no bias == the old call, bit for bit, on cases of
    the logit-processor tests (all three old processors on, mixed rows, the decode form's store)."""
    x = C.make_logits(4, V, 7)
    seqs = [[3, 4, 3, 4, 3], None, [8] * 30, [2, 6, 2, 6, 9, 2, 6]]
    for decode in (False, True):
        kw = dict(penalty=[1.3, 1.3, 1.0, 0.5], ngram=[2, 2, 0, 3], bans=[[5, 150], [5], [], [210]],
                  rows=[5, 0, 1, 3], hist_rows=7, decode=decode)
        old = C.make_case(x, seqs, kw["penalty"], kw["ngram"], **{k: v for k, v in kw.items()
                                                               if k not in ("penalty", "ngram")})
        want, want_h = C.reference(old)
        got, got_h = P.reference(P.make_case(x, seqs, [2, 0, 5, 3], 0.0, 0.0, **kw))
        assert torch.equal(got, want) and torch.equal(got_h, want_h)
        from rag_llm_k8s_amd.ops.backend import TorchBackend

        lg, h = old["logits"].clone(), old["hist"].clone()
        TorchBackend("cpu").logits_process(lg, 0, old["ids"], old["rows"], old["pos"], h, old["penalty"], old["ngram"],
                                           old["ban_ids"], old["ban_count"], gen_start=None, presence=None,
                                           frequency=None, bias_ids=None, bias_vals=None, bias_count=None)
        assert torch.equal(lg, want) and torch.equal(h, want_h)


def test_shards_and_host_refusals():
    """Two vocab shards concatenate to the unsharded row (a bias id at both shard edges); the torch backend
    refuses a partial keyword set, a narrow table, a span over PENALTY_GEN_MAX and a gen_start past pos + 1."""
    seq = _seq(20, 90, 120, 1) + [100, 101, 100, 5, 210, 100]
    x = C.make_logits(1, V, 4)
    bias = {0: 1.5, 100: -2.0, 101: 4.0, 210: 8.0}
    case = P.make_case(x, [seq], 20, 0.4, 0.9, bias=[bias], penalty=1.2, ngram=2, bans=[[100, 7]])
    full, _ = P.reference(case)
    parts = [P.reference(dict(case, logits=x[:, o:o + w].clone(), vocab_offset=o))[0] for o, w in ((0, 101), (101, 110))]
    assert torch.equal(torch.cat(parts, 1), full)
    with pytest.raises(ValueError):
        P.reference(case, bias_ids=None)
    with pytest.raises(ValueError):
        P.reference(dict(case, bias_ids=case["bias_ids"][:, :3].contiguous(), bias_vals=case["bias_vals"][:, :3].contiguous()))
    with pytest.raises(ValueError):
        P.reference(case, gen_bound=PENALTY_GEN_MAX + 1)
    with pytest.raises(ValueError):
        P.reference(case, gen_bound=5)  # the row's span is 6
    P.reference(case, gen_bound=6)
    with pytest.raises(ValueError):
        P.reference(dict(case, gen_start=torch.tensor([len(seq) + 1], dtype=torch.int32)))
    with pytest.raises(ValueError):
        P.reference(dict(case, gen_start=torch.tensor([-1], dtype=torch.int32)))


# ----------------------------------------------------------------------------- engine vs transformers
K_MIN, N_NEW = 6, 14


def _counter_processor(prompt_len, f, p):
    from transformers import LogitsProcessor

    class CounterOracle(LogitsProcessor):
        def __call__(self, input_ids, scores):
            out = scores.clone()
            for i in range(scores.shape[0]):
                out[i] = P.counter_row(scores[i].float(), input_ids[i].tolist(), prompt_len, f, p)
            return out

    return CounterOracle()


@pytest.mark.parametrize("rep_pen,f_pen,p_pen", [(1.1, 1.5, 0.5), (1.3, -2.0, -1.5)])
def test_engine_greedy_equals_transformers_generate(tiny, rep_pen, f_pen, p_pen):
    """Engine greedy tokens == HF generate(sequence_bias=..., repetition_penalty=..., logits_processor=[the Counter
    oracle]) with the prompt split over four prefill chunks and a plain request in the same batch, whose tokens
    equal its tokens in a batch without penalty rows. The bias forbids plain decoding's first token (-100).
    Positive penalties (a repeat HF makes without them goes away) and negative ones (counts grow to 9 and the
    3-gram ban has to break the runs)."""
    cfg, hf, sd = tiny
    prompt, eos, plain = _prompt_and_eos(hf)
    bias = {plain[0]: -100.0, 17: 2.0, 300: -3.5}
    hf_kw = dict(max_new_tokens=N_NEW, eos_token_id=eos, repetition_penalty=rep_pen, no_repeat_ngram_size=3,
                 min_new_tokens=K_MIN, sequence_bias=[[[t], v] for t, v in bias.items()])
    want = _hf_generate(hf, prompt, logits_processor=[_counter_processor(len(prompt), f_pen, p_pen)], **hf_kw)
    no_pen = _hf_generate(hf, prompt, **hf_kw)
    assert want[0] != plain[0] and want != no_pen[:len(want)] and len(want) >= K_MIN  # the penalties matter
    other = torch.randint(3, 384, (23,), generator=torch.Generator().manual_seed(2)).tolist()
    p_plain = SamplingParams(max_new_tokens=N_NEW, do_sample=False)
    p_pen = SamplingParams(max_new_tokens=N_NEW, do_sample=False, repetition_penalty=rep_pen, no_repeat_ngram_size=3,
                           min_new_tokens=K_MIN, frequency_penalty=f_pen, presence_penalty=p_pen,
                           logit_bias=normalize_logit_bias(bias))
    assert p_pen.uses_penalties() and p_pen.uses_processors() and not p_plain.uses_penalties()
    assert isinstance(hash(p_pen.logit_bias), int) and dataclasses.asdict(p_pen)["logit_bias"] == p_pen.logit_bias

    eng = _engine(cfg, sd, max_prefill_tokens=16, eos_ids=[eos])
    a = eng.add_request(other, p_plain, seed=1)
    b = eng.add_request(prompt, p_pen, seed=2)
    eng.run_until_done()
    assert b.out == want, (b.out, want)
    assert eng.stats["penalty_steps"] > 0 and eng.stats["penalty_steps"] <= eng.stats["logit_proc_steps"]
    assert sorted(eng._hist_free) == list(range(4))

    ref = _engine(cfg, sd, max_prefill_tokens=16, eos_ids=[eos])
    a2 = ref.add_request(other, p_plain, seed=1)
    ref.add_request(prompt, dataclasses.replace(p_pen, frequency_penalty=0.0, presence_penalty=0.0, logit_bias=()),
                    seed=2)
    ref.run_until_done()
    assert a.out == a2.out and a.finish_reason == a2.finish_reason
    assert ref.stats["penalty_steps"] == 0 and ref.stats["logit_proc_steps"] > 0

    # presence / frequency alone (no old processor): only generated tokens count, so the first token is plain's
    only = _engine(cfg, sd, eos_ids=[])
    c = only.add_request(prompt, SamplingParams(max_new_tokens=N_NEW, do_sample=False, ignore_eos=True,
                                                frequency_penalty=2.0, presence_penalty=2.0), seed=1)
    only.run_until_done()
    want_c = _hf_generate(hf, prompt, max_new_tokens=N_NEW,
                          logits_processor=[_counter_processor(len(prompt), 2.0, 2.0)])
    assert c.out == want_c and c.out[0] == plain[0]


def test_discarded_step_recomputed_with_penalties(tiny):
    """A decode step that is discarded and recomputed leaves the outputs unchanged: the counts are rebuilt from the
    idempotent history every step."""
    cfg, hf, sd = tiny
    torch.manual_seed(11)
    base = torch.randint(3, cfg.vocab_size, (9,)).tolist()
    prompts = [base * 3, torch.randint(3, cfg.vocab_size, (29,)).tolist()]
    params = [SamplingParams(max_new_tokens=9, temperature=0.8, top_p=0.9, top_k=20, ignore_eos=True,
                             repetition_penalty=1.2, frequency_penalty=1.5, presence_penalty=-0.5,
                             logit_bias=((base[0], -100.0), (base[1], 6.0))),
              SamplingParams(max_new_tokens=9, do_sample=False, ignore_eos=True, frequency_penalty=2.0)]
    outs = []
    for fault_at in (None, 3, 1):
        eng = _engine(cfg, sd)
        if fault_at is not None:
            seen = []

            def fault(eng=eng, seen=seen, at=fault_at):
                if eng.stats["decode_steps"] + 1 == at and not seen:
                    seen.append(1)
                    return 2
                return 0

            eng._kernel_fault = fault
        seqs = [eng.add_request(p, q, seed=5 + i) for i, (p, q) in enumerate(zip(prompts, params))]
        eng.run_until_done()
        outs.append([s.out for s in seqs])
        assert all(len(o) == 9 for o in outs[-1]) and base[0] not in outs[-1][0]
        assert eng.stats.get("engine_faults", 0) == (0 if fault_at is None else 1)
        assert sorted(eng._hist_free) == list(range(4))
    assert outs[1] == outs[0] and outs[2] == outs[0]


def test_bias_table_not_inherited_with_the_history_row(tiny):
    """One history row, three sequential requests: a biased one, then one with a penalty but no bias, then one with
    a different, shorter bias. The second equals its run on a fresh engine; the third sees only its own entries."""
    cfg, hf, sd = tiny
    prompt = torch.randint(3, 384, (12,), generator=torch.Generator().manual_seed(5)).tolist()
    plain = _engine(cfg, sd, max_batch=1).generate([prompt], SamplingParams(max_new_tokens=6, do_sample=False,
                                                                           ignore_eos=True))[0]
    first = SamplingParams(max_new_tokens=6, do_sample=False, ignore_eos=True,
                           logit_bias=tuple((t, -100.0) for t in sorted(set(plain))))
    second = SamplingParams(max_new_tokens=6, do_sample=False, ignore_eos=True, presence_penalty=1e-3)
    third = SamplingParams(max_new_tokens=6, do_sample=False, ignore_eos=True, logit_bias=((0, 1.0),))
    eng = _engine(cfg, sd, max_batch=1)
    outs = [eng.generate([prompt], p)[0] for p in (first, second, third)]
    assert not set(outs[0]) & set(plain) and eng._hist.shape[0] == 1
    fresh = [_engine(cfg, sd, max_batch=1).generate([prompt], p)[0] for p in (second, third)]
    assert outs[1:] == fresh and outs[1][0] == plain[0] and outs[2][0] == plain[0]
    assert eng._bias_ids.shape == (1, LOGIT_BIAS_MAX) and eng._bias_vals.dtype == torch.float32


# ----------------------------------------------------------------------------- TP = 2 over gloo
TP_PARAMS = dict(max_new_tokens=8, do_sample=False, ignore_eos=True, repetition_penalty=1.2, frequency_penalty=1.25,
                 presence_penalty=0.5, logit_bias=((3, 4.0), (159, 100.0), (160, -100.0), (319, 2.5)))


def _entry(rank, port, d, sd, prompts):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD),
                      LOCAL_RANK=str(rank), HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    torch.set_num_threads(2)
    from rag_llm_k8s_amd.parallel.comm import TPComm
    from rag_llm_k8s_amd.parallel.dist import init_distributed

    ctx = init_distributed(tp=2, backend="gloo")
    try:
        w = LlamaWeights.from_state_dict(CFG, sd, "cpu", ctx.tp_rank, ctx.tp)
        m = LlamaModel(CFG, w, "cpu", comm=TPComm(ctx.tp_group, ctx.tp, ctx.tp_rank, "cpu"), max_positions=512)
        eng = LLMEngine(m, num_blocks=32, max_batch=4, max_prefill_tokens=24, max_model_len=512, use_graphs=False,
                        tp_group=ctx.tp_group)
        # a bias id of the other rank's shard passes admission: the bound is the whole vocabulary
        outs = eng.generate(prompts, SamplingParams(**TP_PARAMS))
        torch.save((outs, eng.stats["penalty_steps"]), os.path.join(d, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_tp2_engine_tokens_equal_tp1():
    """Vocab-parallel TP=2 (each rank writes its logit shard from the replicated history and bias tables) == TP=1;
    bias ids at both edges of both shards (vocab 320: shards 0..159 and 160..319)."""
    import torch.multiprocessing as mp

    from rag_llm_k8s_amd.engine.llm_engine import Sequence
    from rag_llm_k8s_amd.parallel.tp import _decode, _encode

    sd = llama_state_dict(CFG, seed=4, std=0.05)
    g = torch.Generator().manual_seed(8)
    base = torch.randint(3, 320, (7,), generator=g).tolist()
    prompts = [base * 5, torch.randint(3, 320, (40,), generator=g).tolist()]
    m = LlamaModel(CFG, LlamaWeights.from_state_dict(CFG, sd, "cpu"), "cpu", max_positions=512)
    eng = LLMEngine(m, num_blocks=32, max_batch=4, max_prefill_tokens=24, max_model_len=512, use_graphs=False)
    want = eng.generate(prompts, SamplingParams(**TP_PARAMS))
    assert all(len(o) == 8 and 160 not in o for o in want) and all(o[0] == 159 for o in want)
    port = _free_port()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_entry, args=(port, d, sd, prompts), nprocs=WORLD, join=True)
        got = [torch.load(os.path.join(d, "r%d.pt" % r), weights_only=False) for r in range(WORLD)]
    assert got[0][0] == want and got[1][0] == want
    assert got[0][1] == got[1][1] == eng.stats["penalty_steps"] > 0
    s = Sequence(prompts[0], SamplingParams(**TP_PARAMS), 3)
    new, _ = _decode(_encode([s]))
    assert new[0][2] == s.params and isinstance(new[0][2].logit_bias, tuple) and hash(new[0][2].logit_bias)


# ----------------------------------------------------------------------------- admission
def test_validation_at_admission(tiny):
    cfg, hf, sd = tiny
    eng = _engine(cfg, sd, eos_ids=[7], max_model_len=512)
    big = _engine(cfg, sd, eos_ids=[7], max_model_len=16384, num_blocks=300)
    vocab = cfg.vocab_size
    bad = [(dict(presence_penalty=2.5), "presence_penalty"), (dict(frequency_penalty=-2.01), "frequency_penalty"),
           (dict(presence_penalty=float("nan")), "presence_penalty"),
           (dict(frequency_penalty=float("inf")), "frequency_penalty"), (dict(presence_penalty=True), "presence_penalty"),
           (dict(frequency_penalty="1"), "frequency_penalty"),
           (dict(logit_bias=((5, 1.0), (5, 2.0))), "logit_bias"), (dict(logit_bias=((vocab, 1.0),)), "vocabulary"),
           (dict(logit_bias=((-1, 1.0),)), "vocabulary"), (dict(logit_bias=((5, 100.5),)), "-100..100"),
           (dict(logit_bias=((5, float("nan")),)), "finite"), (dict(logit_bias=((5, True),)), "number"),
           (dict(logit_bias=((5.5, 1.0),)), "integer"), (dict(logit_bias=((6, 1.0), (5, 1.0))), "sorted"),
           (dict(logit_bias={5: 1.0}), "tuple"),
           (dict(logit_bias=tuple((i, 0.5) for i in range(LOGIT_BIAS_MAX + 1))), "at most 300")]
    for kw, word in bad:
        for fn in (lambda p: eng.add_request([5, 6], p), lambda p: eng.make_sequence([5, 6], p, 0)):
            with pytest.raises(ValueError) as e:
                fn(SamplingParams(max_new_tokens=10, **kw))
            assert word in str(e.value), (kw, str(e.value))
    for kw in (dict(presence_penalty=0.1), dict(frequency_penalty=-0.1)):
        with pytest.raises(ValueError) as e:
            big.add_request([5, 6], SamplingParams(max_new_tokens=PENALTY_GEN_MAX + 1, **kw))
        assert "8192" in str(e.value)
        big.make_sequence([5, 6], SamplingParams(max_new_tokens=PENALTY_GEN_MAX, **kw), 0)
    big.make_sequence([5, 6], SamplingParams(max_new_tokens=PENALTY_GEN_MAX + 1, logit_bias=((5, 1.0),)), 0)  # bias only
    ok = SamplingParams(max_new_tokens=10, presence_penalty=-2, frequency_penalty=2.0,
                        logit_bias=tuple((i, -100.0 if i % 2 else 100.0) for i in range(LOGIT_BIAS_MAX)))
    eng.add_request([5, 6], ok)
    assert not eng.running and eng._hist is None
    with pytest.raises(ValueError):
        normalize_logit_bias({5: 1.0, "6": 2.0})
    assert normalize_logit_bias({9: 1, 3: -2.5}) == ((3, -2.5), (9, 1.0))
    for p, (proc, pen) in ((SamplingParams(), (False, False)), (SamplingParams(presence_penalty=0.5), (True, True)),
                           (SamplingParams(frequency_penalty=-1.0), (True, True)),
                           (SamplingParams(logit_bias=((1, 0.0),)), (True, True)),
                           (SamplingParams(repetition_penalty=1.1), (True, False))):
        assert (p.uses_processors(), p.uses_penalties()) == (proc, pen)


# ----------------------------------------------------------------------------- service / Flask
def test_flask_fields_and_refusals(assets, tmp_path_factory):
    from rag_llm_k8s_amd.server.app import create_app

    svc = _service(assets, tmp_path_factory.mktemp("index"))
    try:
        c = create_app(svc).test_client()
        seen = []
        submit = svc.loop.submit
        svc.loop.submit = lambda ids, params, seed=None: (seen.append((list(ids), params)), submit(ids, params, seed=seed))[1]
        q = {"prompt": "Pleabra tisho quar?"}

        def post(route="/generate", **kw):
            svc._seed = 1
            return c.post(route, json=dict(q, **kw))

        r0 = post()
        r1 = post(presence_penalty=0, frequency_penalty=0.0, logit_bias={})
        assert r0.status_code == r1.status_code == 200 and r0.data == r1.data  # neutral values: the same bytes
        assert seen[1][1] == svc.params and svc.engine.stats["penalty_steps"] == 0
        for route in ("/generate", "/query"):
            r = post(route, presence_penalty=0.5, frequency_penalty=-1, logit_bias={"7": -100, "3": 2.5})
            assert r.status_code == 200 and set(r.get_json()) == {"generated_text", "context"}
            p = seen[-1][1]
            assert (p.presence_penalty, p.frequency_penalty, p.logit_bias) == (0.5, -1.0, ((3, 2.5), (7, -100.0)))
            assert p.max_new_tokens == svc.params.max_new_tokens and p is not svc.params
        assert svc.engine.stats["penalty_steps"] > 0 and svc.params.logit_bias == ()
        n = len(seen)
        vocab = svc.engine.model.cfg.vocab_size
        for bad in (dict(presence_penalty=2.5), dict(frequency_penalty=-3), dict(presence_penalty="0.5"),
                    dict(frequency_penalty=True), dict(logit_bias={"x": 1}), dict(logit_bias={"1.5": 1}),
                    dict(logit_bias={"-1": 1}), dict(logit_bias={"5": True}), dict(logit_bias={"5": "1"}),
                    dict(logit_bias={"5": 101}), dict(logit_bias={str(vocab): 1}), dict(logit_bias=[[5, 1.0]]),
                    dict(logit_bias={"5": 1, "05": 2}), dict(logit_bias={str(i): 1 for i in range(301)}),
                    dict(logit_bias="{}"), dict(logit_bias=7)):
            r = post(**bad)
            assert r.status_code == 400 and "error" in r.get_json(), bad
        assert len(seen) == n  # refused before anything was queued
        with pytest.raises(ValueError):
            svc.request_params({"nonsense": 1})
    finally:
        svc.shutdown()


def test_logit_bias_forbids_the_greedy_first_token(assets, tmp_path_factory):
    svc = _service(assets, tmp_path_factory.mktemp("index"))
    try:
        seen = []
        submit = svc.loop.submit

        def spy(ids, params, seed=None):
            s = submit(ids, params, seed=seed)
            seen.append(s)
            return s

        svc.loop.submit = spy
        svc._seed = 1
        svc.generate("Pleabra tisho quar?")
        first = seen[0].out[0]
        svc._seed = 1
        svc.generate("Pleabra tisho quar?", params=svc.request_params({"logit_bias": {str(first): -100}}))
        assert seen[1].prompt == seen[0].prompt and seen[1].out[0] != first and first not in seen[1].out[:1]
        svc._seed = 1
        svc.generate("Pleabra tisho quar?", params=svc.request_params({"frequency_penalty": 2.0}))
        assert seen[2].out[0] == first  # nothing generated yet at the first token: the penalties are a no-op there
    finally:
        svc.shutdown()


def test_env_defaults_feed_the_service(assets, tmp_path_factory, monkeypatch):
    from rag_llm_k8s_amd.config import RagConfig

    base = RagConfig.from_env()
    assert (base.presence_penalty, base.frequency_penalty, base.logit_bias) == (0.0, 0.0, "")
    monkeypatch.setenv("PRESENCE_PENALTY", "0.25")
    monkeypatch.setenv("FREQUENCY_PENALTY", "-0.5")
    monkeypatch.setenv("LOGIT_BIAS", '{"11": -100, "4": 1.5}')
    cfg = RagConfig.from_env()
    assert (cfg.presence_penalty, cfg.frequency_penalty, cfg.logit_bias) == (0.25, -0.5, '{"11": -100, "4": 1.5}')
    svc = _service(assets, tmp_path_factory.mktemp("index"), presence_penalty=cfg.presence_penalty,
                   frequency_penalty=cfg.frequency_penalty, logit_bias=cfg.logit_bias)
    try:
        p = svc.params
        assert (p.presence_penalty, p.frequency_penalty, p.logit_bias) == (0.25, -0.5, ((4, 1.5), (11, -100.0)))
        out = svc.generate("Pleabra tisho quar?")
        assert isinstance(out["generated_text"], str) and svc.engine.stats["penalty_steps"] > 0
    finally:
        svc.shutdown()
    for bad in (dict(presence_penalty=3.0), dict(logit_bias='{"a": 1}'), dict(logit_bias="[1]"),
                dict(logit_bias="{not json")):
        with pytest.raises(ValueError):
            _service(assets, tmp_path_factory.mktemp("index"), **bad)
