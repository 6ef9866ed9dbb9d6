"""History-dependent logit processors on CPU: the torch backend vs transformers' own processors, the engine vs
transformers' generate(), the discard / recompute path, the history-row lifecycle, TP=2 over gloo, and the
service / Flask surface (repetition_penalty, no_repeat_ngram_size, min_new_tokens)."""
import os
import socket
import tempfile

import pytest
import torch

import logits_proc_cases as C
from rag_llm_k8s_amd.engine.llm_engine import LLMEngine, SamplingParams
from rag_llm_k8s_amd.models.llama import LlamaModel, LlamaWeights, llama_tiny
from rag_llm_k8s_amd.utils.synthetic import llama_state_dict

V = 211


# ----------------------------------------------------------------------------- op level
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_torch_backend_equals_transformers(n):
    """TorchBackend.logits_process == the three transformers processors (torch.equal) and == the token-by-token
    Python oracle, over history lengths 1, n-2, n-1, n, 300, penalties 0.5 / 1.0 / 1.3, a history that is one id
    100 times, min_new_tokens 0 / 1 / beyond the generated count with several stop ids; the logits hold
    positive, negative, zero and -inf entries."""
    pytest.importorskip("transformers")
    stop = [5, 9, 200]
    g = torch.Generator().manual_seed(n)
    lens = sorted({L for L in (1, n - 2, n - 1, n, 300) if L >= 1})
    seqs = [torch.randint(2, 12, (L,), generator=g).tolist() for L in lens] + [[4] * 100]
    seqs += [h for L in lens for h in C.ngram_histories(n, L, vocab=12)]
    checked = 0
    for si, seq in enumerate(seqs):
        x = C.make_logits(1, V, 100 * n + si)
        x[0, seq[0]] = (0.0, -2.5, 3.25, float("-inf"))[si % 4]  # a history id on each kind of logit
        for pen in (0.5, 1.0, 1.3):
            for min_new, generated in ((0, 0), (1, 0), (1, 1), (len(seq) + 3, min(len(seq), 2))):
                bans = stop if generated < min_new else []
                case = C.make_case(x, [seq], pen, n, bans=[bans], rows=[2], hist_rows=4)
                got, hist = C.reference(case)
                assert torch.equal(hist, case["hist"])  # no ids: the history is only read
                want = C.hf_row(x[0], seq, pen, n, min_new, generated, stop)
                assert torch.equal(got[0], want), (seq[:10], pen, n, min_new, generated)
                assert torch.equal(got[0], C.python_row(x[0], seq, pen, n, bans))
                checked += 1
    assert checked >= 12 * len(seqs)


def test_torch_backend_rows_shards_and_decode_store():
    """Rows with history row -1 and rows with neutral parameters come back bit-identical; the decode form stores
    exactly hist[row][pos] = id; two vocab shards concatenate to the unsharded result."""
    x = C.make_logits(4, V, 7)
    seqs = [[3, 4, 3, 4, 3], None, [8] * 30, [2, 6, 2, 6, 9, 2, 6]]
    case = C.make_case(x, seqs, [1.3, 1.3, 1.0, 0.5], [2, 2, 0, 3], bans=[[5, 150], [5], [], [210]],
                       rows=[5, 0, 1, 3], hist_rows=7, decode=True)
    got, hist = C.reference(case)
    assert torch.equal(got[1], x[1]) and torch.equal(got[2], x[2])
    want_hist = case["hist"].clone()
    for b, r in ((0, 5), (2, 1), (3, 3)):
        want_hist[r, len(seqs[b]) - 1] = seqs[b][-1]
    assert torch.equal(hist, want_hist)
    for b in (0, 3):
        bans = [[5, 150], None, None, [210]][b]
        assert torch.equal(got[b], C.python_row(x[b], seqs[b], float(case["penalty"][b]), int(case["ngram"][b]), bans))
    parts = []
    for off, w in ((0, 101), (101, V - 101)):
        sh = dict(case, logits=x[:, off:off + w].clone(), vocab_offset=off)
        parts.append(C.reference(sh)[0])
    assert torch.equal(torch.cat(parts, 1), got)


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


def _hf_generate(hf, prompt, **kw):
    with torch.no_grad():
        out = hf.generate(torch.tensor([prompt]), do_sample=False, pad_token_id=0,
                          attention_mask=torch.ones(1, len(prompt), dtype=torch.long), **kw)
    return out[0, len(prompt):].tolist()


K_MIN, N_NEW = 6, 14
PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=K_MIN)


def _prompt_and_eos(hf):
    """A prompt with repeats in it, and as eos the second token plain greedy decoding produces: without the
    processors the model stops after 2 tokens (checked), so a run that ignores them cannot pass."""
    torch.manual_seed(21)
    base = torch.randint(3, 384, (19,)).tolist()
    prompt = base + base[:11] + base[3:17] + base[:5]  # 49 tokens, repeated 3-grams
    plain = _hf_generate(hf, prompt, max_new_tokens=N_NEW)
    eos = plain[1]
    assert eos not in plain[:1]
    return prompt, eos, plain


def test_engine_greedy_equals_transformers_generate(tiny):
    """Engine greedy tokens == HF generate(do_sample=False, repetition_penalty=1.3, no_repeat_ngram_size=3,
    min_new_tokens=6), with the prompt split over four prefill chunks and a plain request in the same batch; the
    plain request's tokens equal its tokens in a batch without processor rows."""
    cfg, hf, sd = tiny
    prompt, eos, plain = _prompt_and_eos(hf)
    stopped = _hf_generate(hf, prompt, max_new_tokens=N_NEW, eos_token_id=eos)
    assert len(stopped) == 2 < K_MIN and stopped[-1] == eos  # without the processors: an early stop
    want = _hf_generate(hf, prompt, max_new_tokens=N_NEW, eos_token_id=eos, **PROC)
    assert want != plain[:len(want)] and len(want) >= K_MIN and eos not in want[:K_MIN]
    other = torch.randint(3, 384, (23,), generator=torch.Generator().manual_seed(2)).tolist()
    p_plain = SamplingParams(max_new_tokens=N_NEW, do_sample=False)
    p_proc = SamplingParams(max_new_tokens=N_NEW, do_sample=False, **PROC)

    eng = _engine(cfg, sd, max_prefill_tokens=16, eos_ids=[eos])
    a = eng.add_request(other, p_plain, seed=1)
    b = eng.add_request(prompt, p_proc, seed=2)
    eng.run_until_done()
    assert b.out == want, (b.out, want)
    assert C.no_ngram_repeats(prompt + b.out, 3, start=len(prompt))
    assert eng.stats["logit_proc_steps"] > 0 and sorted(eng._hist_free) == list(range(4))
    assert eng.bm.free_blocks() == 63

    ref = _engine(cfg, sd, max_prefill_tokens=16, eos_ids=[eos])
    a2 = ref.add_request(other, p_plain, seed=1)
    b2 = ref.add_request(prompt, p_plain, seed=2)
    ref.run_until_done()
    assert a.out == a2.out and a.finish_reason == a2.finish_reason
    assert b2.out == stopped and b2.finish_reason == "stop"  # the engine, too, stops early without them
    assert ref.stats["logit_proc_steps"] == 0 and ref._hist is None


def test_validation_at_admission(tiny):
    cfg, hf, sd = tiny
    eng = _engine(cfg, sd, eos_ids=[7])
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")),
                dict(repetition_penalty=float("nan")), dict(no_repeat_ngram_size=9), dict(no_repeat_ngram_size=-1),
                dict(min_new_tokens=-1), dict(min_new_tokens=11), dict(no_repeat_ngram_size=2.5)):
        with pytest.raises(ValueError):
            eng.add_request([5, 6], SamplingParams(max_new_tokens=10, **bad))
        with pytest.raises(ValueError):
            eng.make_sequence([5, 6], SamplingParams(max_new_tokens=10, **bad), 0)
    eng.add_request([5, 6], SamplingParams(max_new_tokens=10, no_repeat_ngram_size=8, min_new_tokens=10,
                                           repetition_penalty=0.5))
    assert not eng.running and eng._hist is None  # allocated at the first admission, not before


def test_ignore_eos_requests_unaffected_by_min_new_tokens(tiny):
    cfg, hf, sd = tiny
    outs = []
    for m in (0, 5):
        eng = _engine(cfg, sd, eos_ids=[7])
        outs.append(eng.generate([[5, 6, 9, 10]], SamplingParams(max_new_tokens=8, do_sample=False, ignore_eos=True,
                                                                 min_new_tokens=m)))
        assert eng._hist is None and eng.stats["logit_proc_steps"] == 0
    assert outs[0] == outs[1]


# ----------------------------------------------------------------------------- discard / recompute, row lifecycle
def test_discarded_step_recomputed_with_processors(tiny):
    """A decode step that is discarded and recomputed (engine._kernel_fault, as tests/test_llama_cpu.py drives
    it) leaves the processors' outputs unchanged: the history writes are idempotent."""
    cfg, hf, sd = tiny
    torch.manual_seed(11)
    base = torch.randint(3, cfg.vocab_size, (9,)).tolist()
    prompts = [base * 3, torch.randint(3, cfg.vocab_size, (29,)).tolist()]
    params = [SamplingParams(max_new_tokens=9, temperature=0.8, top_p=0.9, top_k=20, stop_token_ids=(7, 11),
                             repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=9),
              SamplingParams(max_new_tokens=9, do_sample=False, ignore_eos=True)]
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
        assert all(len(o) == 9 for o in outs[-1])
        assert eng.stats.get("engine_faults", 0) == (0 if fault_at is None else 1)
        assert C.no_ngram_repeats(prompts[0] + outs[-1][0], 2, start=len(prompts[0]))
        assert sorted(eng._hist_free) == list(range(4))
    assert outs[1] == outs[0] and outs[2] == outs[0]


def test_history_rows_reused_and_returned(tiny):
    """More sequential requests than history rows: rows are reused, none leaks, the free list is full again."""
    cfg, hf, sd = tiny
    eng = _engine(cfg, sd, max_batch=2)
    p = SamplingParams(max_new_tokens=3, do_sample=False, ignore_eos=True, repetition_penalty=1.2)
    plain = SamplingParams(max_new_tokens=3, do_sample=False, ignore_eos=True)
    seqs = [eng.add_request([5 + i, 6, 9, 10 + i], plain if i == 2 else p, seed=i) for i in range(7)]
    used = []
    while eng.has_work():
        eng.step()
        used.append(tuple(sorted(s.hist_row for s in eng.running if s.hist_row >= 0)))
        assert len(eng.running) <= 2 and all(len(set(u)) == len(u) for u in used)
        assert len(eng._hist_free) + len(eng._hist_after) + len(used[-1]) == 2
    assert all(len(s.out) == 3 and s.hist_row == -1 for s in seqs)
    assert eng._hist.shape == (2, 512) and sorted(eng._hist_free) == [0, 1] and not eng._hist_after
    assert {r for u in used for r in u} == {0, 1}  # 6 processor requests shared the 2 rows


# ----------------------------------------------------------------------------- TP = 2 over gloo
WORLD = 2
CFG = llama_tiny(vocab=320, layers=2, hidden=256, heads=4, kv_heads=2, inter=512)
TP_PARAMS = dict(max_new_tokens=8, do_sample=False, stop_token_ids=(17, 300), repetition_penalty=1.3,
                 no_repeat_ngram_size=2, min_new_tokens=8)


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
        outs = eng.generate(prompts, SamplingParams(**TP_PARAMS))
        torch.save((outs, eng.stats["logit_proc_steps"]), os.path.join(d, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_tp2_engine_tokens_equal_tp1():
    """Vocab-parallel TP=2 (each rank processes its logit shard against the replicated history) == TP=1, all
    three processors on, chunked prompts."""
    import dataclasses

    import torch.multiprocessing as mp

    from rag_llm_k8s_amd.parallel.tp import _decode, _encode
    from rag_llm_k8s_amd.engine.llm_engine import Sequence

    sd = llama_state_dict(CFG, seed=4, std=0.05)
    g = torch.Generator().manual_seed(8)
    base = torch.randint(3, 320, (7,), generator=g).tolist()
    prompts = [base * 5, torch.randint(3, 320, (40,), generator=g).tolist()]
    m = LlamaModel(CFG, LlamaWeights.from_state_dict(CFG, sd, "cpu"), "cpu", max_positions=512)
    eng = LLMEngine(m, num_blocks=32, max_batch=4, max_prefill_tokens=24, max_model_len=512, use_graphs=False)
    want = eng.generate(prompts, SamplingParams(**TP_PARAMS))
    assert all(len(o) == 8 for o in want) and all(C.no_ngram_repeats(p + o, 2, start=len(p)) for p, o in zip(prompts, want))
    port = _free_port()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_entry, args=(port, d, sd, prompts), nprocs=WORLD, join=True)
        got = [torch.load(os.path.join(d, "r%d.pt" % r), weights_only=False) for r in range(WORLD)]
    assert got[0][0] == want and got[1][0] == want
    assert got[0][1] == got[1][1] == eng.stats["logit_proc_steps"] > 0
    # the admission record a follower rank rebuilds its SamplingParams from carries the new fields
    s = Sequence(prompts[0], SamplingParams(**TP_PARAMS), 3)
    new, _ = _decode(_encode([s]))
    assert dataclasses.asdict(new[0][2]) == dataclasses.asdict(s.params)


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


def _service(assets, idx, **kw):
    from rag_llm_k8s_amd.config import RagConfig
    from rag_llm_k8s_amd.server.builder import build_service

    root, pdfs = assets
    cfg = RagConfig(model_path=str(root), index_path=str(idx / "faiss_index"), pdf_dir=str(pdfs),
                    embed_model=str(root / "minilm"), device="cpu", max_new_tokens=6, max_model_len=1024,
                    max_batch=4, use_cuda_graphs=False, kv_cache_blocks=64, seed=1, do_sample=False, **kw)
    svc = build_service(cfg, start_threads=True)
    svc.store.ensure_exists()
    assert svc.ingest_directory() == 2
    svc.ready = True
    return svc


def test_flask_per_request_fields(assets, tmp_path_factory):
    from rag_llm_k8s_amd.server.app import create_app

    svc = _service(assets, tmp_path_factory.mktemp("index"))
    try:
        c = create_app(svc).test_client()
        seen = []
        submit = svc.loop.submit
        svc.loop.submit = lambda ids, params, seed=None: (seen.append(params), submit(ids, params, seed=seed))[1]
        q = {"prompt": "Pleabra tisho quar?"}

        def post(**kw):
            svc._seed = 1  # the same request seed for every call
            return c.post("/generate", json=dict(q, **kw))

        r0 = post()
        r1 = post(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)
        assert r0.status_code == r1.status_code == 200 and r0.data == r1.data  # neutral values: the same bytes
        assert seen[0] is svc.params and seen[1] == svc.params and svc.engine.stats["logit_proc_steps"] == 0
        for route in ("/generate", "/query"):
            svc._seed = 1
            r = c.post(route, json=dict(q, repetition_penalty=1.5, no_repeat_ngram_size=2, min_new_tokens=3))
            assert r.status_code == 200 and set(r.get_json()) == {"generated_text", "context"}
            p = seen[-1]
            assert (p.repetition_penalty, p.no_repeat_ngram_size, p.min_new_tokens) == (1.5, 2, 3)
            assert p.max_new_tokens == svc.params.max_new_tokens and p is not svc.params
        assert svc.engine.stats["logit_proc_steps"] > 0
        assert svc.params.repetition_penalty == 1.0  # the defaults are not touched by a request
        n = len(seen)
        for bad in (dict(repetition_penalty=0), dict(repetition_penalty=-2.0), dict(repetition_penalty="1.3"),
                    dict(no_repeat_ngram_size=9), dict(no_repeat_ngram_size=1.5), dict(min_new_tokens=7),
                    dict(min_new_tokens=-1), dict(min_new_tokens=True)):
            r = post(**bad)
            assert r.status_code == 400 and "error" in r.get_json(), bad
        assert len(seen) == n  # refused before anything was queued
        r = c.post("/generate", data="not json", content_type="text/plain")
        assert r.status_code in (400, 415, 500)
    finally:
        svc.shutdown()


def test_env_defaults_feed_the_service(assets, tmp_path_factory, monkeypatch):
    from rag_llm_k8s_amd.config import RagConfig

    base = RagConfig.from_env()
    assert (base.repetition_penalty, base.no_repeat_ngram_size, base.min_new_tokens) == (1.0, 0, 0)
    monkeypatch.setenv("REPETITION_PENALTY", "1.25")
    monkeypatch.setenv("NO_REPEAT_NGRAM_SIZE", "3")
    monkeypatch.setenv("MIN_NEW_TOKENS", "2")
    cfg = RagConfig.from_env()
    assert (cfg.repetition_penalty, cfg.no_repeat_ngram_size, cfg.min_new_tokens) == (1.25, 3, 2)
    svc = _service(assets, tmp_path_factory.mktemp("index"), repetition_penalty=cfg.repetition_penalty,
                   no_repeat_ngram_size=cfg.no_repeat_ngram_size, min_new_tokens=cfg.min_new_tokens)
    try:
        p = svc.params
        assert (p.repetition_penalty, p.no_repeat_ngram_size, p.min_new_tokens) == (1.25, 3, 2)
        out = svc.generate("Pleabra tisho quar?")
        assert isinstance(out["generated_text"], str) and svc.engine.stats["logit_proc_steps"] > 0
    finally:
        svc.shutdown()
    with pytest.raises(ValueError):
        _service(assets, tmp_path_factory.mktemp("index"), no_repeat_ngram_size=12)
