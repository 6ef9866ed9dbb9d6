"""Per-token logprobs on CPU: the torch reference ops on the shared kernel cases, the engine vs transformers'
generate(output_scores=True), sampled / mixed / discarded / full-vocabulary steps, TP=2 over gloo, and the
service / Flask surface (SamplingParams.logprobs, the "logprobs" field and response object, LOGPROBS)."""
import math
import os
import socket
import tempfile

import pytest
import torch

import logprobs_cases as C
from rag_llm_k8s_amd.engine.llm_engine import LOGPROBS_MAX, LLMEngine, SamplingParams
from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights, llama_tiny
from rag_llm_k8s_amd.ops.backend import TorchBackend
from rag_llm_k8s_amd.utils.synthetic import llama_state_dict

# engine-vs-HF logits tolerance of tests/test_llama_cpu.py (relative norm); a logprob is a logit minus an lse,
# so chosen-token logprobs are held to twice it, in the same metric
HF_LOGITS_REL_TOL = 3e-2


# ----------------------------------------------------------------------------- op level (torch reference)
@pytest.mark.parametrize("name,case", C.kernel_cases(), ids=[n for n, _ in C.kernel_cases()])
def test_reference_kernel_cases(name, case):
    worst = C.check_case(TorchBackend("cpu"), "cpu", case)
    print("lse error / bound: %.3f" % worst)
    assert worst <= 1.0


def test_reference_two_vocab_shards():
    worst = C.check_two_shards(TorchBackend("cpu"), "cpu")
    print("lse error / bound: %.3f" % worst)


def test_reference_token_outside_the_lists_is_nan_and_refusals():
    be = TorchBackend("cpu")
    x = C.make_rows(1001, 3, "ties", 1)[:2]
    cv, ci = C.chunk_candidates(x, 3, 64)
    part = be.lse_partials(x, 3)
    missing = int(torch.sort(x[0], descending=True, stable=True).indices[-1])  # the row's last id by rank
    assert missing not in ci[0].tolist()
    outs = C.run_finish(be, "cpu", part, cv, ci, 64, torch.tensor([missing, int(ci[1, 0])], dtype=torch.int32),
                        torch.tensor([3, 3], dtype=torch.int32))
    assert math.isnan(float(outs[1][0])) and not math.isnan(float(outs[1][1]))
    with pytest.raises(ValueError):
        be.logprobs_finish(part, cv[:, :57], ci[:, :57], 19, torch.zeros(2, dtype=torch.int32),
                           torch.zeros(2, dtype=torch.int32))
    for bad in (0, 65):
        with pytest.raises(ValueError):
            be.lse_partials(x, bad)


# ----------------------------------------------------------------------------- engine vs transformers
def _hf_model(cfg, seed=0):
    transformers = pytest.importorskip("transformers")
    hc = transformers.LlamaConfig(**{k: v for k, v in cfg.to_hf_dict().items() if k not in ("architectures",)})
    torch.manual_seed(seed)
    m = transformers.LlamaForCausalLM(hc).eval()
    with torch.no_grad():
        for p in m.parameters():
            p.normal_(0, 0.05)
        for n, p in m.named_parameters():
            if "norm" in n:
                p.fill_(1.0).add_(torch.randn_like(p) * 0.1)
    return m.to(torch.bfloat16)


@pytest.fixture(scope="module")
def tiny():
    cfg = llama_tiny(vocab=384, layers=2, hidden=256, heads=4, kv_heads=2, inter=512)
    cfg.rope_scaling = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                        "original_max_position_embeddings": 64}
    hf = _hf_model(cfg)
    sd = {k: v.detach() for k, v in hf.state_dict().items()}
    return cfg, hf, sd


def _engine(cfg, sd, **kw):
    w = LlamaWeights.from_state_dict(cfg, sd, "cpu")
    model = LlamaModel(cfg, w, "cpu", max_positions=512)
    args = dict(num_blocks=64, max_batch=4, max_model_len=512, use_graphs=False)
    args.update(kw)
    return LLMEngine(model, **args)


def _hf_scores(hf, prompt, **kw):
    """(tokens, scores [T, V] fp32) of a greedy generate(output_scores=True)."""
    with torch.no_grad():
        out = hf.generate(torch.tensor([prompt]), do_sample=False, pad_token_id=0, output_scores=True,
                          return_dict_in_generate=True,
                          attention_mask=torch.ones(1, len(prompt), dtype=torch.long), **kw)
    return out.sequences[0, len(prompt):].tolist(), torch.stack([s[0].float() for s in out.scores])


N_NEW = 14
PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=6)


def _prompt(hf):
    """The prompt of tests/test_logits_proc_cpu.py (repeated 3-grams) and as eos the second token plain greedy
    decoding produces."""
    torch.manual_seed(21)
    base = torch.randint(3, 384, (19,)).tolist()
    prompt = base + base[:11] + base[3:17] + base[:5]
    plain, _ = _hf_scores(hf, prompt, max_new_tokens=N_NEW)
    return prompt, plain[1]


@pytest.mark.parametrize("proc", [False, True], ids=["plain", "processors"])
def test_engine_greedy_logprobs_equal_transformers_scores(tiny, proc):
    """Greedy engine tokens == HF generate(); chosen-token logprobs vs log_softmax(scores) within twice the
    engine-vs-HF logits tolerance (relative norm); alternatives are x[id] - lse of the same step, sorted, and an id
    the processors banned (score -inf) is never a finite alternative."""
    cfg, hf, sd = tiny
    prompt, eos = _prompt(hf)
    kw = dict(PROC) if proc else {}
    want, scores = _hf_scores(hf, prompt, max_new_tokens=N_NEW, eos_token_id=eos, **kw)
    eng = _engine(cfg, sd, max_prefill_tokens=16, eos_ids=[eos])
    s = eng.add_request(prompt, SamplingParams(max_new_tokens=N_NEW, do_sample=False, logprobs=5, **kw), seed=2)
    other = eng.add_request(prompt[:23], SamplingParams(max_new_tokens=N_NEW, do_sample=False), seed=1)
    eng.run_until_done()
    assert s.out == want, (s.out, want)
    assert len(s.logprobs) == len(s.top_logprobs) == len(s.out) >= 2
    assert other.logprobs is None and other.top_logprobs is None
    ref = torch.log_softmax(scores, 1)
    hf_lp = torch.tensor([float(ref[k, t]) for k, t in enumerate(want)])
    got = torch.tensor(s.logprobs)
    rel = float((got - hf_lp).norm() / hf_lp.norm())
    print("chosen-token logprobs vs HF: rel %.4f, max abs %.4f" % (rel, float((got - hf_lp).abs().max())))
    assert rel < 2 * HF_LOGITS_REL_TOL, rel
    for k, alts in enumerate(s.top_logprobs):
        assert len(alts) == 5
        lps = [lp for _, lp in alts]
        assert lps == sorted(lps, reverse=True) and alts[0][1] <= 0.0
        assert alts[0] == (s.out[k], s.logprobs[k])  # greedy: the chosen token is the best alternative
        banned = set((scores[k] == float("-inf")).nonzero().flatten().tolist())
        assert not any(i in banned for i, lp in alts if lp > float("-inf"))
    if proc:
        assert (scores == float("-inf")).any() and eng.stats["logit_proc_steps"] > 0
    assert eng.stats["logprob_steps"] == len(s.out)


def test_validation_at_admission(tiny):
    cfg, hf, sd = tiny
    eng = _engine(cfg, sd)
    for bad in (True, False, 1.0, -1, LOGPROBS_MAX + 1, "3"):
        with pytest.raises(ValueError):
            eng.add_request([5, 6], SamplingParams(max_new_tokens=4, logprobs=bad))
    for ok in (None, 0, LOGPROBS_MAX):
        eng.check_params(SamplingParams(max_new_tokens=4, logprobs=ok))
    narrow = _engine(cfg, sd, top_k_cap=16)  # candidate lists shorter than LOGPROBS_MAX
    with pytest.raises(ValueError):
        narrow.check_params(SamplingParams(max_new_tokens=4, logprobs=1))
    narrow.check_params(SamplingParams(max_new_tokens=4))


def _run(eng, prompts, params, seeds):
    seqs = [eng.add_request(p, q, seed=sd) for p, q, sd in zip(prompts, params, seeds)]
    while eng.has_work():
        eng.step()
        for s in seqs:
            if s.logprobs is not None:
                assert len(s.logprobs) == len(s.top_logprobs) == len(s.out)
    return seqs


def test_sampled_request_and_mixed_batch(tiny):
    """A sampled logprobs request next to a plain one: sum exp(top) <= 1 (+ fp32 slack), the chosen token's value
    equals its entry among the alternatives, the same seed gives the same values; the plain sequence's tokens are
    those of a run with no logprobs request at all and it carries no values."""
    cfg, hf, sd = tiny
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(3, 384, (n,), generator=g).tolist() for n in (31, 17)]
    lp = SamplingParams(max_new_tokens=12, temperature=0.9, top_p=0.95, top_k=40, ignore_eos=True, logprobs=LOGPROBS_MAX)
    plain = SamplingParams(max_new_tokens=12, temperature=0.9, top_p=0.95, top_k=40, ignore_eos=True)
    runs = [_run(_engine(cfg, sd), prompts, [lp, plain], [7, 8]) for _ in range(2)]
    base = _run(_engine(cfg, sd), prompts, [plain, plain], [7, 8])
    a, b = runs[0]
    assert a.out == base[0].out and b.out == base[1].out  # logprobs change nobody's tokens
    assert b.logprobs is None and b.top_logprobs is None and base[0].logprobs is None
    assert runs[1][0].logprobs == a.logprobs and runs[1][0].top_logprobs == a.top_logprobs
    found = 0
    for t, v, alts in zip(a.out, a.logprobs, a.top_logprobs):
        assert len(alts) == LOGPROBS_MAX and v <= 0.0
        # 20 fp32 exponentials of values with <= 2^-21 absolute error each: far below 1e-5 of slack
        assert sum(math.exp(x) for _, x in alts) <= 1.0 + 1e-5
        ids = [i for i, _ in alts]
        if t in ids:
            assert alts[ids.index(t)][1] == v
            found += 1
    assert found >= 6  # a 384-entry vocabulary: most sampled tokens are among the top 20


def test_discarded_step_values_equal_a_fault_free_run(tiny):
    """A decode step that is discarded and recomputed (engine._kernel_fault, as tests/test_llama_cpu.py drives it):
    values and tokens equal a fault-free run, lengths match s.out after every step."""
    cfg, hf, sd = tiny
    g = torch.Generator().manual_seed(11)
    prompts = [torch.randint(3, 384, (n,), generator=g).tolist() for n in (27, 29)]
    params = [SamplingParams(max_new_tokens=9, temperature=0.8, top_p=0.9, top_k=20, ignore_eos=True, logprobs=4),
              SamplingParams(max_new_tokens=9, do_sample=False, ignore_eos=True, logprobs=0)]
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
        seqs = _run(eng, prompts, params, [5, 6])
        assert eng.stats.get("engine_faults", 0) == (0 if fault_at is None else 1)
        assert all(len(s.out) == 9 for s in seqs) and all(t == [] for t in seqs[1].top_logprobs)
        outs.append([(s.out, s.logprobs, s.top_logprobs) for s in seqs])
    assert outs[1] == outs[0] and outs[2] == outs[0]


def test_full_vocabulary_path_returns_values(tiny):
    """top_k = 0 takes the exact full-vocabulary sampler (on the host) and still returns values: the chosen
    token's logprob is log_softmax of the row, checked through the alternatives of a greedy twin."""
    cfg, hf, sd = tiny
    prompt = torch.randint(3, 384, (21,), generator=torch.Generator().manual_seed(4)).tolist()
    eng = _engine(cfg, sd)
    s, = _run(eng, [prompt], [SamplingParams(max_new_tokens=6, temperature=0.8, top_p=0.9, top_k=0, ignore_eos=True,
                                             logprobs=LOGPROBS_MAX)], [3])
    assert len(s.out) == 6 and eng.stats["logprob_steps"] == 6
    for t, v, alts in zip(s.out, s.logprobs, s.top_logprobs):
        assert len(alts) == LOGPROBS_MAX and v <= 0.0 and math.isfinite(v)
        lps = [x for _, x in alts]
        assert lps == sorted(lps, reverse=True) and sum(math.exp(x) for x in lps) <= 1.0 + 1e-5
        ids = [i for i, _ in alts]
        if t in ids:
            assert alts[ids.index(t)][1] == v
    # first token: the same row through the candidate path (greedy twin, top_k within the lists)
    twin, = _run(_engine(cfg, sd), [prompt], [SamplingParams(max_new_tokens=1, do_sample=False, ignore_eos=True,
                                                             logprobs=LOGPROBS_MAX)], [3])
    assert [i for i, _ in twin.top_logprobs[0]] == [i for i, _ in s.top_logprobs[0]]
    for (_, p), (_, q) in zip(twin.top_logprobs[0], s.top_logprobs[0]):
        assert abs(p - q) <= 2.0 ** -20  # the two paths chunk the lse differently: a few fp32 ulps of ~6


# ----------------------------------------------------------------------------- TP = 2 over gloo
WORLD = 2
CFG = llama_tiny(vocab=320, layers=2, hidden=256, heads=4, kv_heads=2, inter=512)
TP_PARAMS = dict(max_new_tokens=8, do_sample=False, ignore_eos=True, logprobs=7)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _entry(rank, port, d, sd, prompts):
    import torch.distributed as dist

    # a CPU test wherever it runs: no GPU is visible to the ranks (init_distributed would claim one per rank)
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
        # record what the two ops saw and gave: this rank's logits shard of every sampling call, and the lse
        be, shards, lses = m.be, [], []
        part_op, finish_op = be.lse_partials, be.logprobs_finish
        be.lse_partials = lambda lg, chunks, out=None: (shards.append(lg.clone()), part_op(lg, chunks, out=out))[1]
        be.logprobs_finish = lambda *a: (finish_op(*a), lses.append(a[6].clone()))[0]
        seqs = [eng.add_request(p, SamplingParams(**TP_PARAMS), seed=i) for i, p in enumerate(prompts)]
        eng.run_until_done()
        torch.save(([(s.out, s.logprobs, s.top_logprobs) for s in seqs], shards, lses), os.path.join(d, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_tp2_logprobs_equal_tp1():
    """Vocab-parallel TP=2 (partials and candidates gathered rank-major, the same finish on the same bytes):
    identical bits on the two ranks; tokens and alternative ids equal TP=1's. The TP=2 model's logits differ from
    TP=1's in bf16 roundings of the row-parallel sums, so the lse bound is checked where it applies: every lse the
    TP=2 engine produced against the float64 logsumexp of its own row (the two ranks' shards concatenated), and
    every returned list must be the (id, x[id] - lse) list of that row, bit for bit, at the step it was sampled for.
    Against TP=1 a place may hold another id only where TP=1's own sorted logits are closer together than twice
    the logits' TP difference; the places that differ are counted against the places where that holds."""
    import dataclasses

    import torch.multiprocessing as mp

    from rag_llm_k8s_amd.engine.llm_engine import Sequence
    from rag_llm_k8s_amd.parallel.tp import _decode, _encode

    sd = llama_state_dict(CFG, seed=4, std=0.05)
    g = torch.Generator().manual_seed(8)
    prompts = [torch.randint(3, 320, (n,), generator=g).tolist() for n in (35, 40)]
    m = LlamaModel(CFG, LlamaWeights.from_state_dict(CFG, sd, "cpu"), "cpu", max_positions=512)
    eng = LLMEngine(m, num_blocks=32, max_batch=4, max_prefill_tokens=24, max_model_len=512, use_graphs=False)
    rows1, part_op = [], m.be.lse_partials
    m.be.lse_partials = lambda lg, chunks, out=None: (rows1.append(lg.clone()), part_op(lg, chunks, out=out))[1]
    ref = [eng.add_request(p, SamplingParams(**TP_PARAMS), seed=i) for i, p in enumerate(prompts)]
    eng.run_until_done()
    port = _free_port()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_entry, args=(port, d, sd, prompts), nprocs=WORLD, join=True)
        got = [torch.load(os.path.join(d, "r%d.pt" % r), weights_only=False) for r in range(WORLD)]
    assert got[0][0] == got[1][0]  # every rank: the same bits
    assert all(torch.equal(a, b) for a, b in zip(got[0][2], got[1][2])) and len(got[0][2]) >= 8
    # the same schedule on both engines: sampling call k of TP=2 saw the rows of call k of TP=1, up to the bf16
    # roundings of the row-parallel sums. Ids must be equal, except that two ids may trade places where TP=1's own
    # logits hold them closer together than twice that difference of the logits (model.forward's, not this op's).
    assert len(rows1) == len(got[0][1])
    slack = {}
    for k, (x1, sh0, sh1) in enumerate(zip(rows1, got[0][1], got[1][1])):
        d = (torch.cat([sh0, sh1], 1) - x1).abs().max(1).values
        for b in range(x1.shape[0]):
            slack[tuple(torch.sort(x1[b], descending=True, stable=True).indices[:7].tolist())] = (x1[b], 2 * float(d[b]))
    # (If y = x + e with |e| <= d, the p-th largest of y is within d of the p-th largest of x, so the ids the two
    # orders hold at place p are within 2d of each other in x, and then so is a neighbour of place p in x's own
    # order: a place may differ only where TP=1's sorted values are that close. `near` counts those places.)
    swapped = near = total = 0
    for s, (out, lps, tops) in zip(ref, got[0][0]):
        assert out == s.out and len(lps) == len(tops) == len(out) == 8
        for alts, walts in zip(tops, s.top_logprobs):
            ids, wids = [i for i, _ in alts], [i for i, _ in walts]
            assert len(ids) == len(set(ids)) == 7
            x1, tol = slack[tuple(wids)]
            sv = torch.sort(x1, descending=True, stable=True).values[:8].tolist()
            for p, (i, j) in enumerate(zip(ids, wids)):
                assert i == j or abs(float(x1[i] - x1[j])) <= tol, (ids, wids, tol)
                swapped += int(i != j)
                near += int((p > 0 and sv[p - 1] - sv[p] <= tol) or sv[p] - sv[p + 1] <= tol)
                total += 1
    print("places holding another id than TP=1's: %d, places where the logits' TP difference allows it: %d of %d"
          % (swapped, near, total))
    assert swapped <= near < total
    # Exact, for every recorded sampling call and every row of it: the row the TP=2 engine sampled from is the two
    # ranks' shards side by side; its lse is within the bound of float64, and the (id, x[id] - lse) list of its
    # stable sort is, bit for bit, what some sequence got at its next step, with that sequence's token and value.
    # Every call advances the sequences it served, and in the end every step of every sequence is accounted for.
    worst, step = 0.0, [0] * len(prompts)
    for sh0, sh1, lse in zip(got[0][1], got[1][1], got[0][2]):
        x = torch.cat([sh0, sh1], 1)
        assert x.shape[1] == CFG.vocab_size and lse.shape[0] == x.shape[0]
        l64, bound = C.lse_oracle(x)
        err = (lse.double() - l64).abs()
        assert (err <= bound).all(), (err, bound)
        worst = max(worst, float((err / bound).max()))
        order = torch.sort(x, dim=1, descending=True, stable=True).indices
        served = set()
        for b in range(x.shape[0]):
            want = [(int(i), float(x[b, i] - lse[b])) for i in order[b, :7]]
            hits = [k for k, (out, lps, tops) in enumerate(got[0][0]) if k not in served and step[k] < len(out)
                    and tops[step[k]] == want and lps[step[k]] == float(x[b, out[step[k]]] - lse[b])]
            assert hits, (step, b, want)
            served.add(hits[0])
        for k in served:
            step[k] += 1
    print("lse error / bound: %.3f" % worst)
    assert step == [8] * len(prompts)
    # the admission record a follower rank rebuilds its SamplingParams from carries the new field
    s = Sequence(prompts[0], SamplingParams(**TP_PARAMS), 3)
    new, _ = _decode(_encode([s]))
    assert dataclasses.asdict(new[0][2]) == dataclasses.asdict(s.params) and new[0][2].logprobs == 7


# ----------------------------------------------------------------------------- service / Flask
@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    from rag_llm_k8s_amd.models import encoder as E
    from rag_llm_k8s_amd.models import gpt2 as G2
    from rag_llm_k8s_amd.utils import synthetic as S

    root = tmp_path_factory.mktemp("models")
    G2.write_gpt2_checkpoint(str(root), G2.gpt2_tiny(1024), seed=0)
    ecfg = E.EncoderConfig(vocab_size=1024, hidden_size=128, num_hidden_layers=2, num_attention_heads=4,
                           intermediate_size=256, max_seq_length=128)
    S.write_encoder_checkpoint(str(root / "minilm"), ecfg, seed=0)
    pdfs = tmp_path_factory.mktemp("pdfs")
    S.write_pdf_corpus(str(pdfs), 2, pages=1, words_per_page=300)
    return root, pdfs


def _service(assets, idx, threads=True, **kw):
    from rag_llm_k8s_amd.config import RagConfig
    from rag_llm_k8s_amd.server.builder import build_service

    root, pdfs = assets
    cfg = RagConfig(model_path=str(root), index_path=str(idx / "faiss_index"), pdf_dir=str(pdfs),
                    embed_model=str(root / "minilm"), device="cpu", max_new_tokens=6, max_model_len=1024,
                    max_batch=4, use_cuda_graphs=False, kv_cache_blocks=64, seed=1, do_sample=False, **kw)
    svc = build_service(cfg, start_threads=threads)
    svc.store.ensure_exists()
    assert svc.ingest_directory() == 2
    svc.ready = True
    return svc


def _check_object(obj, n_alt):
    assert set(obj) == {"token_ids", "tokens", "token_logprobs", "top_logprobs", "mean_logprob"}
    n = len(obj["token_ids"])
    assert n >= 1 and len(obj["tokens"]) == len(obj["token_logprobs"]) == len(obj["top_logprobs"]) == n
    assert all(isinstance(t, int) for t in obj["token_ids"]) and all(isinstance(t, str) for t in obj["tokens"])
    assert all(isinstance(v, float) and v <= 0.0 for v in obj["token_logprobs"])
    assert obj["mean_logprob"] == pytest.approx(sum(obj["token_logprobs"]) / n)
    for alts in obj["top_logprobs"]:
        assert len(alts) <= n_alt
        assert all(set(a) == {"id", "token", "logprob"} and math.isfinite(a["logprob"]) for a in alts)


def test_flask_field_response_object_and_400s(assets, tmp_path_factory):
    from rag_llm_k8s_amd.server.app import create_app

    svc = _service(assets, tmp_path_factory.mktemp("index"))
    try:
        c = create_app(svc).test_client()
        q = {"prompt": "Pleabra tisho quar?"}

        def post(route="/generate", **kw):
            svc._seed = 1  # the same request seed for every call
            return c.post(route, json=dict(q, **kw))

        r0 = post()
        assert r0.status_code == 200 and set(r0.get_json()) == {"generated_text", "context"}  # exactly today's keys
        assert svc.engine.stats["logprob_steps"] == 0
        for route in ("/generate", "/query"):
            r = post(route, logprobs=3)
            assert r.status_code == 200 and set(r.get_json()) == {"generated_text", "context", "logprobs"}
            assert r.get_json()["generated_text"] == r0.get_json()["generated_text"]
            obj = r.get_json()["logprobs"]
            _check_object(obj, 3)
            assert len(obj["token_ids"]) == svc.params.max_new_tokens or obj["token_ids"][-1] in svc.params.stop_token_ids
            assert all(len(a) == 3 for a in obj["top_logprobs"])
        _check_object(post(logprobs=0).get_json()["logprobs"], 0)
        assert svc.engine.stats["logprob_steps"] > 0 and svc.params.logprobs is None
        steps = svc.engine.stats["logprob_steps"]
        for bad in (True, 2.0, -1, LOGPROBS_MAX + 1):
            r = post(logprobs=bad)
            assert r.status_code == 400 and "error" in r.get_json(), bad
        assert svc.engine.stats["logprob_steps"] == steps  # refused before anything was queued
    finally:
        svc.shutdown()


def test_infinite_alternatives_are_dropped_from_the_object(assets, tmp_path_factory):
    """Fewer than N finite logits: the -inf alternatives stay in Sequence.top_logprobs and leave the JSON object."""
    from rag_llm_k8s_amd.engine.llm_engine import Sequence

    svc = _service(assets, tmp_path_factory.mktemp("index"))
    try:
        s = Sequence([5, 6], SamplingParams(max_new_tokens=2, logprobs=3), 0)
        s.out = [11, 12]
        s.logprobs = [-0.5, 0.0]
        s.top_logprobs = [[(11, -0.5), (40, -1.25), (41, -3.0)], [(12, 0.0), (0, float("-inf")), (1, float("-inf"))]]
        obj = svc.logprobs_object(s)
        _check_object(obj, 3)
        assert [len(a) for a in obj["top_logprobs"]] == [3, 1] and obj["top_logprobs"][1][0]["id"] == 12
        assert obj["mean_logprob"] == -0.25
        assert svc.logprobs_object(Sequence([5], SamplingParams(max_new_tokens=2), 0)) is None
    finally:
        svc.shutdown()


def test_logprobs_env_default(assets, tmp_path_factory, monkeypatch):
    from rag_llm_k8s_amd.config import RagConfig

    assert RagConfig.from_env().logprobs is None
    monkeypatch.setenv("LOGPROBS", "2")
    cfg = RagConfig.from_env()
    assert cfg.logprobs == 2
    svc = _service(assets, tmp_path_factory.mktemp("index"), logprobs=cfg.logprobs)
    try:
        assert svc.params.logprobs == 2
        out = svc.generate("Pleabra tisho quar?")
        _check_object(out["logprobs"], 2)
    finally:
        svc.shutdown()
    with pytest.raises(ValueError):
        _service(assets, tmp_path_factory.mktemp("index"), logprobs=LOGPROBS_MAX + 1)


def test_generate_batch_outputs_carry_the_object(assets, tmp_path_factory):
    import dataclasses

    svc = _service(assets, tmp_path_factory.mktemp("index"), threads=False)
    try:
        qs = ["Pleabra tisho quar?", "Quar tisho?"]
        plain = svc.generate_batch(qs, seeds=[1, 2])
        assert all("logprobs" not in o for o in plain)
        outs = svc.generate_batch(qs, params=dataclasses.replace(svc.params, logprobs=4), seeds=[1, 2])
        for o, p in zip(outs, plain):
            assert o["generated_text"] == p["generated_text"]
            _check_object(o["logprobs"], 4)
            assert len(o["logprobs"]["token_ids"]) == o["_gen_tokens"]
    finally:
        svc.shutdown()
