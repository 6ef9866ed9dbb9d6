"""Per-token logprobs on the GPU: ragk_lse_partials / ragk_logprobs_finish on the shared kernel cases (canary
frames, strided and misaligned views, float64 lse oracle, exact ids and values), behind the real candidate top-k,
the launcher's refusals, and the engine with the two launches inside the decode graph (graph == eager == async,
vs the CPU oracle, the plain path's graphs untouched, an EOS overrun's values dropped)."""
import math

import pytest
import torch

import logprobs_cases as C
from rag_llm_k8s_amd.engine.llm_engine import LOGPROBS_MAX, LLMEngine, SamplingParams
from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights, llama_tiny
from rag_llm_k8s_amd.utils.synthetic import llama_state_dict

pytestmark = pytest.mark.gpu

# GPU-vs-CPU logits tolerance of tests/test_e2e_gpu.py::test_gpu_prefill_logits_vs_cpu (relative norm); logprobs
# (a logit minus an lse) are held to twice it, in the same metric
GPU_LOGITS_REL_TOL = 3e-2


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("name,case", C.kernel_cases(), ids=[n for n, _ in C.kernel_cases()])
def test_kernel_cases(native, name, case):
    worst = C.check_case(native, "cuda", case)
    print("lse error / bound: %.3f" % worst)
    assert worst <= 1.0


def test_two_vocab_shards(native):
    print("lse error / bound: %.3f" % C.check_two_shards(native, "cuda"))


@pytest.mark.parametrize("chunks", [1, 3, 31])
def test_finish_behind_the_candidate_topk(native, chunks):
    """The lists ragk_topk_candidates yields (the radix-select kernel at 1 / 3 chunks, the lane-network kernel at
    31) straight into the finish: ids == a stable sort of the row, values == x[id] - lse."""
    V, K = 4099, 64
    x = C.make_rows(V, chunks, "all_equal", 40 + chunks)
    d = x.cuda()
    cv, ci = native.topk_candidates(d, K, chunks=chunks)
    want_v, want_i = C.chunk_candidates(x, chunks, K)
    assert torch.equal(ci.cpu(), want_i) and torch.equal(cv.cpu(), want_v)
    nlp = torch.tensor([20, 5, 1, 20, 20], dtype=torch.int32)
    tok = ci[:, chunks * K // 2].clone().cpu()
    tok[tok < 0] = ci[:, 0].cpu()[tok < 0]
    part = native.lse_partials(d, chunks)
    outs = C.run_finish(native, "cuda", part.cpu(), cv.cpu(), ci.cpu(), K, tok, nlp)
    C.check_finish(outs, x, tok, nlp, *C.lse_oracle(x))


def test_token_outside_the_lists_is_nan(native):
    x = C.make_rows(1001, 3, "ties", 1)[:2]
    cv, ci = C.chunk_candidates(x, 3, 64)
    part = native.lse_partials(x.cuda(), 3).cpu()
    missing = int(torch.sort(x[0], descending=True, stable=True).indices[-1])
    assert missing not in ci[0].tolist()
    outs = C.run_finish(native, "cuda", part, cv, ci, 64, torch.tensor([missing, int(ci[1, 0])], dtype=torch.int32),
                        torch.tensor([3, 3], dtype=torch.int32))
    assert math.isnan(float(outs[1][0])) and outs[1][1] == x[1, int(ci[1, 0])] - outs[0][1]
    assert not torch.isnan(outs[2][:, :3]).any()


def test_launcher_refusals(native):
    """Wrong dtype, wrong device, non-contiguous buffers, chunks out of range, list_len < LOGPROBS_MAX: refused
    on the host, before any launch (the output buffers keep their canaries)."""
    x = C.make_rows(1001, 3, "ties", 2)[:2].cuda()
    part = torch.full((2, 3, 2), C.CANARY_F, device="cuda")
    for bad in (lambda: native.lse_partials(x.double(), 3), lambda: native.lse_partials(x.cpu(), 3),
                lambda: native.lse_partials(x.t().contiguous().t(), 3), lambda: native.lse_partials(x, 0),
                lambda: native.lse_partials(x, 65), lambda: native.lse_partials(x, 3, out=part.cpu()),
                lambda: native.lse_partials(x, 3, out=part.double()),
                lambda: native.lse_partials(x, 3, out=torch.empty((2, 3, 4), device="cuda")[:, :, :2])):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert (part == C.CANARY_F).all()
    native.lse_partials(x, 3, out=part)
    cv, ci = (t.cuda() for t in C.chunk_candidates(x.cpu(), 3, 64))
    tok, nlp = ci[:, 0].contiguous(), torch.tensor([3, 3], dtype=torch.int32, device="cuda")
    lse = torch.full((2,), C.CANARY_F, device="cuda")
    ok = dict(part=part, cand_v=cv, cand_i=ci, list_len=64, tok=tok, nlp=nlp, out_lse=lse)
    for k, v in (("cand_v", cv.double()), ("cand_v", cv.cpu()), ("cand_v", cv[:, ::2]), ("cand_i", ci.long()),
                 ("cand_i", ci.cpu()), ("part", part.cpu()), ("part", part.double()), ("part", part[:, :, :1]),
                 ("tok", tok.long()), ("tok", tok.cpu()), ("nlp", nlp.float()), ("nlp", nlp[:1]),
                 ("list_len", 50), ("out_lse", lse.cpu()), ("out_lse", lse.double()),
                 ("out_top_id", torch.zeros((2, LOGPROBS_MAX), dtype=torch.int64, device="cuda")),
                 ("out_top_lp", torch.zeros((2, 2 * LOGPROBS_MAX), device="cuda")[:, ::2])):
        with pytest.raises(ValueError):
            native.logprobs_finish(**dict(ok, **{k: v}))
    with pytest.raises(ValueError):  # lists shorter than LOGPROBS_MAX
        native.logprobs_finish(part, cv[:, :57].contiguous(), ci[:, :57].contiguous(), LOGPROBS_MAX - 1, tok, nlp, lse)
    torch.cuda.synchronize()
    assert (lse == C.CANARY_F).all()
    native.logprobs_finish(**ok)
    torch.cuda.synchronize()
    assert (lse != C.CANARY_F).all()


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
    return [torch.randint(3, 1000, (n,), generator=g).tolist() for n in lens]


STOP = tuple(range(3, 1000, 9))  # ~1/9 of the vocabulary ends a sequence (as test_e2e_gpu's async test)


def _run_seqs(eng, prompts, params):
    seqs = [eng.add_request(pr, pa, seed=10 + i) for i, (pr, pa) in enumerate(zip(prompts, params))]
    while eng.has_work():
        eng.step()
        for s in seqs:
            if s.logprobs is not None:
                assert len(s.logprobs) == len(s.top_logprobs) == len(s.out)
    assert eng._inflight is None and not eng.running and eng.bm.free_blocks() == 64 - 1
    return seqs


def _run(eng, prompts, params):
    return [(s.out, s.finish_reason, s.logprobs, s.top_logprobs) for s in _run_seqs(eng, prompts, params)]


def test_graph_eager_async_sync_identical(native, tiny_llama):
    """Sampled requests, logprobs on for five of seven (N = 20 / 5 / 0; more requests than batch slots, early
    stops, a repetition-penalty row): hipGraph decode == eager decode, async pipeline == sync, and a second run on
    the engine whose logprob graphs were captured lazily mid-pipeline: equal tokens, bit-equal values."""
    cfg, sd = tiny_llama
    prompts = _prompts(4, (9, 40, 200, 5, 77, 130, 31))
    params = [SamplingParams(max_new_tokens=m, temperature=0.9, top_p=0.95, top_k=50, stop_token_ids=STOP, logprobs=n,
                             repetition_penalty=rp)
              for m, n, rp in ((12, 20, 1.0), (3, None, 1.0), (20, 5, 1.3), (7, 0, 1.0), (16, None, 1.0), (1, 20, 1.0),
                               (9, 3, 1.0))]
    outs = {}
    for name, graphs, async_ in (("async", True, True), ("sync", True, False), ("eager", False, False)):
        eng = _engine(cfg, sd, "cuda", graphs)
        eng.async_decode = async_ and eng.async_decode
        eng.mixed_steps = False  # as test_e2e_gpu.test_async_decode_equals_sync: isolate the decode pipeline
        outs[name] = _run(eng, prompts, params)
        assert eng.stats["logprob_steps"] > 0
        if name == "async":
            assert any(k.logprobs and not k.penalties for k in eng.graphs)
            assert any(not (k.logprobs or k.penalties) for k in eng.graphs)
            outs["again"] = _run(eng, prompts, params)
    assert outs["async"] == outs["sync"] == outs["eager"] == outs["again"]
    assert any(r == "stop" for _, r, _, _ in outs["async"]) and any(r == "length" for _, r, _, _ in outs["async"])
    for (out, _, lps, tops), pa in zip(outs["async"], params):
        if pa.logprobs is None:
            assert lps is None and tops is None
            continue
        assert all(math.isfinite(v) and v <= 0.0 for v in lps)
        for t, v, alts in zip(out, lps, tops):
            assert len(alts) == pa.logprobs and [x for _, x in alts] == sorted((x for _, x in alts), reverse=True)
            ids = [i for i, _ in alts]
            if t in ids:
                assert alts[ids.index(t)][1] == v


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


def test_gpu_greedy_logprobs_vs_cpu_oracle(native, tiny_llama):
    """The prompts of test_e2e_gpu.test_gpu_engine_matches_cpu_greedy, greedy with logprobs = 5, teacher forced on
    the GPU's own tokens as that test is: the chosen tokens' logprobs, and the alternatives' (by id), against
    log_softmax of the CPU oracle's row within twice the GPU-vs-CPU logits tolerance (relative norm)."""
    cfg, sd = tiny_llama
    torch.manual_seed(0)
    prompts = [torch.randint(3, 1000, (n,)).tolist() for n in (5, 77, 130, 300, 513)]
    p = SamplingParams(max_new_tokens=6, do_sample=False, ignore_eos=True, logprobs=5)
    eng = _engine(cfg, sd, "cuda", True, mb=8)
    seqs = [eng.add_request(pr, p, seed=1) for pr in prompts]
    eng.run_until_done()
    got, want, got_alt, want_alt = [], [], [], []
    for pr, s in zip(prompts, seqs):
        assert len(s.out) == len(s.logprobs) == len(s.top_logprobs) == 6
        ref = torch.log_softmax(_oracle_logits(cfg, sd, pr + s.out[:-1])[len(pr) - 1:], 1)
        for k, (t, v, alts) in enumerate(zip(s.out, s.logprobs, s.top_logprobs)):
            assert alts[0] == (t, v)  # greedy: the chosen token leads the alternatives
            got.append(v), want.append(float(ref[k, t]))
            for i, x in alts:
                got_alt.append(x), want_alt.append(float(ref[k, i]))
    for a, b, what in ((got, want, "chosen"), (got_alt, want_alt, "alternatives")):
        a, b = torch.tensor(a), torch.tensor(b)
        rel = float((a - b).norm() / b.norm())
        print("%s logprobs, GPU engine vs CPU oracle: rel %.5f, max abs %.5f" % (what, rel, float((a - b).abs().max())))
        assert rel < 2 * GPU_LOGITS_REL_TOL, (what, rel)


def test_plain_path_untouched_by_a_logprobs_request(native, tiny_llama):
    """Plain requests before and after a logprobs request on one engine: identical tokens, every (B, False) /
    (B, True) graph entry captured before it the same object, logprob_steps counting only steps with such a row."""
    cfg, sd = tiny_llama
    prompts = _prompts(7, (9, 40, 200))
    p = SamplingParams(max_new_tokens=8, temperature=0.8, top_p=0.9, top_k=40, ignore_eos=True)
    pen = SamplingParams(max_new_tokens=8, temperature=0.8, top_p=0.9, top_k=40, ignore_eos=True, repetition_penalty=1.3)
    eng = _engine(cfg, sd, "cuda", True)
    a = eng.generate(prompts, p, seeds=[1, 2, 3])
    a2 = eng.generate(prompts[:2], pen, seeds=[4, 5])
    assert eng.stats["logprob_steps"] == 0 and eng._lp_pins is None
    assert not any(k.logprobs or k.penalties for k in eng.graphs)
    assert any(k.processors for k in eng.graphs) and any(not k.processors for k in eng.graphs)
    entries = dict(eng.graphs)
    lp = SamplingParams(max_new_tokens=8, temperature=0.8, top_p=0.9, top_k=40, ignore_eos=True, logprobs=2)
    seqs = [eng.add_request(pr, q, seed=sd_) for pr, q, sd_ in zip(prompts[:2], (lp, p), (4, 5))]
    eng.run_until_done()
    n = eng.stats["logprob_steps"]
    assert n == 8 and len(seqs[0].logprobs) == 8 and seqs[1].logprobs is None  # 1 prefill + 7 decode steps
    assert any(k.logprobs and not k.penalties for k in eng.graphs)
    assert eng.generate(prompts, p, seeds=[1, 2, 3]) == a and eng.generate(prompts[:2], pen, seeds=[4, 5]) == a2
    assert eng.stats["logprob_steps"] == n
    assert all(eng.graphs[k] is v for k, v in entries.items())


def test_eos_overrun_values_are_dropped(native, tiny_llama):
    """A request that stops on EOS while the pipeline has its next row in flight: that row's token and values are
    discarded together -- lengths match, and the values are those of the synchronous run, which has no overrun."""
    cfg, sd = tiny_llama
    prompts = _prompts(9, (33, 60))
    free = SamplingParams(max_new_tokens=10, do_sample=False, ignore_eos=True, logprobs=4)
    eng = _engine(cfg, sd, "cuda", True)
    full = _run(eng, prompts, [free, free])
    out0 = full[0][0]
    cut = next(k for k in range(2, 9) if out0[k] not in out0[:k])  # stops at its (cut + 1)-th token
    stop = SamplingParams(max_new_tokens=10, do_sample=False, stop_token_ids=(out0[cut],), logprobs=4)
    res = {}
    for async_ in (True, False):
        e = _engine(cfg, sd, "cuda", True)
        e.async_decode = async_ and e.async_decode
        e.mixed_steps = False
        seqs = _run_seqs(e, prompts, [stop, free])
        res[async_] = [(s.out, s.finish_reason, s.logprobs, s.top_logprobs) for s in seqs]
        out, reason, lps, tops = res[async_][0]
        assert reason == "stop" and out == out0[:cut + 1] and len(lps) == len(tops) == cut + 1
        assert lps == full[0][2][:cut + 1] and tops == full[0][3][:cut + 1]
        # the pipeline had the row after the EOS in flight (its K/V was computed: computed == length); the
        # synchronous path never ran it
        assert e.async_decode == async_ and seqs[0].computed == seqs[0].length - (0 if async_ else 1)
    assert res[True] == res[False]
    assert res[True][1] == full[1]
