"""Cross-encoder reranking on the CPU: pair building vs HF tokenizers, Reranker.score on the TorchBackend vs
fp32 transformers *ForSequenceClassification, the rerank_select oracle, the document token cache, and the
service with a reranker attached (order of the context, per-request switch, filters, untouched store)."""
import math
import re

import numpy as np
import pytest
import torch

import rerank_cases as C
from rag_llm_k8s_amd.config import RagConfig
from rag_llm_k8s_amd.engine.rerank_engine import PairLayout, Reranker, TokenCache
from rag_llm_k8s_amd.ingest.text import build_context
from rag_llm_k8s_amd.models import encoder as E
from rag_llm_k8s_amd.ops import reference as R
from rag_llm_k8s_amd.ops.backend import TorchBackend
from rag_llm_k8s_amd.utils import synthetic as S

tokenizers = pytest.importorskip("tokenizers")
KINDS = ["bert", "xlm-roberta"]


# ------------------------------------------------------------------------------------------ pair building
def _hf_tok(path, max_len):
    t = tokenizers.Tokenizer.from_file(path + "/tokenizer.json")
    t.enable_truncation(max_length=max_len, strategy="only_second")
    return t


def _one_token_word(rr, kind):
    """A word that is one token, alone and repeated (so a text of n words is n tokens)."""
    for w in C.word_model(kind).words[:300]:
        if len(rr.tok.encode(w, add_special_tokens=False)) == 1 and \
                len(rr.tok.encode(" ".join([w] * 7), add_special_tokens=False)) == 7:
            return w
    raise AssertionError("no single-token word in the synthetic vocabulary")


@pytest.mark.parametrize("kind", KINDS)
def test_pairs_equal_hf_only_second(kind):
    path = C.checkpoint(kind, 128, 2)
    max_len = 32
    rr = C.load_reranker(path, "cpu", max_len=max_len)
    specials = 3 if kind == "bert" else 4
    assert rr.layout.specials == specials and rr.budget == max_len - specials
    ht = _hf_tok(path, max_len)
    w = _one_token_word(rr, kind)
    q = " ".join([w] * 4)
    room = rr.budget - 4
    docs = [" ".join([w] * n) for n in (1, room - 1, room, room + 1, 3 * room)] + [""]
    wm = C.word_model(kind)
    docs += [" ".join(wm.sample(n, np.random.default_rng(n))) for n in (3, 11, 40)]  # natural text, multi-piece words
    got = rr.pairs([q], [docs])
    for d, (ids, types) in zip(docs, got):
        e = ht.encode(q, d)
        assert ids.tolist() == e.ids, d
        assert types.tolist() == e.type_ids, d
        assert ids.dtype == np.int32 and types.dtype == np.int32 and len(ids) <= max_len
    assert [len(p[0]) for p in got[:6]] == [specials + 5, max_len - 1, max_len, max_len, max_len, specials + 4]
    if kind == "bert":  # [CLS] q [SEP] d [SEP] with type ids 0...0 1...1
        ids, types = got[0]
        assert types.tolist() == [0] * 6 + [1] * 2
        assert ids[0] == rr.tok.token_to_id("[CLS]") and ids[5] == ids[-1] == rr.tok.token_to_id("[SEP]")
    else:  # <s> q </s></s> d </s>
        ids, _ = got[0]
        assert ids[0] == 0 and ids[5] == ids[6] == ids[-1] == 2


@pytest.mark.parametrize("kind", KINDS)
def test_long_query_keeps_half_the_budget(kind):
    """A query longer than half the budget keeps budget // 2 tokens and the document the rest (pinned by hand:
    HF only_second would fail on such a pair)."""
    path = C.checkpoint(kind, 128, 2)
    rr = C.load_reranker(path, "cpu", max_len=32)
    w = _one_token_word(rr, kind)
    wid = rr.tok.encode(w, add_special_tokens=False)[0]
    ids, types = rr.pairs([" ".join([w] * 20)], [[" ".join([w] * 30)]])[0]
    half = rr.budget // 2
    rest = rr.budget - half
    if kind == "bert":
        cls_, sep = rr.tok.token_to_id("[CLS]"), rr.tok.token_to_id("[SEP]")
        assert ids.tolist() == [cls_] + [wid] * half + [sep] + [wid] * rest + [sep]
        assert types.tolist() == [0] * (half + 2) + [1] * (rest + 1)
    else:
        assert ids.tolist() == [0] + [wid] * half + [2, 2] + [wid] * rest + [2]
    assert len(ids) == 32
    # a short query leaves the document everything else
    ids, _ = rr.pairs([w], [[" ".join([w] * 60)]])[0]
    assert len(ids) == 32 and (ids == wid).sum() == rr.budget


def test_layout_from_bert_and_roberta_processors():
    bert = PairLayout.from_spec({"post_processor": {"type": "BertProcessing", "sep": ["[SEP]", 102],
                                                    "cls": ["[CLS]", 101]}}, lambda t: None)
    ids, types = bert.build([7, 8], [9])
    assert ids.tolist() == [101, 7, 8, 102, 9, 102] and types.tolist() == [0, 0, 0, 0, 1, 1]
    rob = PairLayout.from_spec({"post_processor": {"type": "Sequence", "processors": [
        {"type": "ByteLevel"}, {"type": "RobertaProcessing", "sep": ["</s>", 2], "cls": ["<s>", 0]}]}}, lambda t: None)
    ids, types = rob.build([7], [9, 9])
    assert ids.tolist() == [0, 7, 2, 2, 9, 9, 2] and not types.any()
    with pytest.raises(ValueError, match="post-processor"):
        PairLayout.from_spec({"post_processor": None}, lambda t: None)


# ------------------------------------------------------------------------------------------ scores vs the oracle
def _text_pairs(kind):
    wm = C.word_model(kind)
    rng = np.random.default_rng(3)
    qs = [" ".join(wm.sample(n, rng)) for n in (1, 3, 5)]
    docs = [[" ".join(wm.sample(n, rng)) for n in row] for row in ((1, 6, 14, 60), (2, 10, 22, 4), (0, 8, 30, 12))]
    return qs, docs


@pytest.mark.parametrize("kind,H,heads", C.MODELS)
def test_scores_match_transformers(kind, H, heads):
    pytest.importorskip("transformers")
    path = C.checkpoint(kind, H, heads)
    rr = C.load_reranker(path, "cpu")
    assert isinstance(rr.be, TorchBackend) and rr.typed == (kind == "bert")
    qs, docs = _text_pairs(kind)
    got = rr.score(qs, docs)
    assert [len(g) for g in got] == [4, 4, 4] and all(g.dtype == np.float32 for g in got)
    ht = _hf_tok(path, C.MAX_LEN)
    enc = [ht.encode(q, d) for q, ds in zip(qs, docs) for d in ds]
    lens = [len(e.ids) for e in enc]
    assert min(lens) < 12 and max(lens) == C.MAX_LEN and len(set(lens)) >= 8  # mixed lengths, one truncated
    ref = C.hf_scores(path, [(e.ids, e.type_ids) for e in enc])
    e_cpu = float(np.abs(np.concatenate(got) - ref).max())
    print("%s H=%d: e_cpu = %.5f, fp32 score std = %.3f" % (kind, H, e_cpu, ref.std()))
    assert ref.std() >= 0.5, "head_scale too small: fp32 score std %.3f" % ref.std()
    assert e_cpu < C.E_BOUND, "e_cpu = %.5f (bound %.3g, score std %.3f)" % (e_cpu, C.E_BOUND, ref.std())
    # one packed batch or one pair per batch: both within the bound of the fp32 scores (bf16 GEMM rounding
    # depends on the batch shape), so within twice the bound of each other
    rr1 = Reranker(rr.model, rr.tok, max_len=C.MAX_LEN, max_batch_tokens=1)
    assert np.allclose(np.concatenate(rr1.score(qs, docs)), np.concatenate(got), atol=2 * C.E_BOUND)


@pytest.mark.parametrize("kind,H,heads", C.MODELS)
def test_token_pairs_meet_the_ordering_condition(kind, H, heads):
    """The inputs of the GPU model test, checked on the CPU: spread >= 0.5 and at least three quarters of the
    adjacent gaps of the fp32 order exceed 4 e_cpu; the TorchBackend keeps the order across those gaps."""
    pytest.importorskip("transformers")
    path = C.checkpoint(kind, H, heads)
    model = C.load_model(path, "cpu")
    pairs, ref = C.token_pairs(path)
    assert [len(p[0]) for p in pairs][-1] == C.MAX_LEN and len(pairs) == 12
    assert np.array_equal(ref, C.hf_scores(path, pairs))
    ids, lens, types = C.pack(pairs, "cpu", kind == "bert")
    got = model.score_packed(ids, lens, types).double().numpy()
    e_cpu = float(np.abs(got - ref).max())
    gaps, n_adj = C.ordering_gaps(ref, e_cpu)
    print("%s H=%d: e_cpu = %.5f, std = %.3f, %d / %d gaps > 4 e_cpu" % (kind, H, e_cpu, ref.std(), len(gaps), n_adj))
    assert ref.std() >= 0.5 and e_cpu < C.E_BOUND
    assert len(gaps) >= 0.75 * n_adj
    assert all(got[a] > got[b] for a, b in gaps)


def test_head_errors():
    cfg = C.encoder_config("bert", 128, 2)
    sd = S.cross_encoder_state_dict(cfg, seed=0)
    sd["classifier.weight"] = torch.zeros(3, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="num_labels"):
        E.EncoderWeights.from_state_dict(cfg, sd, "cpu")
    bare = E.EncoderModel(cfg, E.EncoderWeights.from_state_dict(cfg, S.encoder_state_dict(cfg), "cpu"), "cpu")
    assert bare.w.head is None
    with pytest.raises(ValueError, match="head"):
        bare.score_packed(torch.zeros(3, dtype=torch.int32), [3])
    w = E.EncoderWeights.random(cfg, "cpu", seed=4, head=True)
    w0 = E.EncoderWeights.random(cfg, "cpu", seed=4)
    assert w0.head is None and torch.equal(w.word, w0.word) and torch.equal(w.layers[1]["wo2"], w0.layers[1]["wo2"])
    assert w.type_table.shape == (2, 128) and torch.equal(w.type_table[0], w.type_row)
    assert w.head["w1"].shape == (128, 128) and isinstance(w.head["b2"], float)


def test_forward_packed_unchanged_and_typed_embed_reduces():
    """forward_packed = hidden_packed + pooling (the embedder's path); all-zero type ids give the same hidden states."""
    cfg = C.encoder_config("bert", 128, 2)
    m = E.EncoderModel(cfg, E.EncoderWeights.random(cfg, "cpu", seed=2, head=True, head_scale=4.0), "cpu")
    lens = [5, 1, 9]
    ids = torch.randint(5, 1000, (sum(lens),), generator=torch.Generator().manual_seed(0)).int()
    h, cu = m.hidden_packed(ids, lens)
    assert cu.tolist() == [0, 5, 6, 15]
    assert torch.equal(m.forward_packed(ids, lens), m.be.pool_l2norm(h, cu, mode=cfg.pooling, normalize=cfg.normalize))
    h0, _ = m.hidden_packed(ids, lens, torch.zeros_like(ids))
    assert torch.equal(h0, h)
    h1, _ = m.hidden_packed(ids, lens, torch.ones_like(ids))
    assert not torch.equal(h1, h)


# ------------------------------------------------------------------------------------------ rerank_select oracle
@pytest.mark.parametrize("Q,N,k", C.SELECT_SHAPES)
def test_rerank_select_reference_is_a_stable_sort(Q, N, k):
    s, ids, dist, nv = C.select_case(Q, N)
    got = TorchBackend().rerank_select(s, ids, dist, nv, k)
    want = C.select_oracle(s, ids, dist, nv, k)
    for g, w in zip(got, want):
        assert C.bits_equal(g, w)
    if Q == 3:
        assert nv.tolist()[1] == 0 and (got[0][1] == -1).all() and (got[1][1] == C.FLT_MAX).all() \
            and (got[2][1] == -C.FLT_MAX).all()


def test_rerank_select_hand_case():
    nan, inf = float("nan"), float("inf")
    s = torch.tensor([[1.0, nan, 2.0, -inf, 2.0, nan, 1.0, inf]])
    ids = torch.arange(10, 18)[None]
    dist = torch.arange(8, dtype=torch.float32)[None]
    oi, od, osc = R.rerank_select(s, ids, dist, torch.tensor([8], dtype=torch.int32), 8)
    assert oi.tolist() == [[17, 12, 14, 10, 16, 13, 11, 15]]  # inf, the 2.0 tie in order, the 1.0 tie, -inf, NaNs
    assert od.tolist() == [[7, 2, 4, 0, 6, 3, 1, 5]]
    assert math.isnan(osc[0, 6]) and math.isnan(osc[0, 7]) and osc[0, 5] == -inf
    with pytest.raises(ValueError):
        TorchBackend().rerank_select(torch.zeros(1, 65), torch.zeros(1, 65, dtype=torch.int64), torch.zeros(1, 65),
                                     torch.zeros(1, dtype=torch.int32), 3)


# ------------------------------------------------------------------------------------------ token cache
class _CountingTok:
    def __init__(self, tok):
        self._tok, self.calls = tok, []

    def __getattr__(self, name):
        return getattr(self._tok, name)

    def encode_batch(self, texts, **kw):
        self.calls.append(list(texts))
        return self._tok.encode_batch(texts, **kw)


def test_second_score_call_tokenizes_no_document():
    rr = C.load_reranker(C.checkpoint("bert", 128, 2), "cpu")
    rr.tok = _CountingTok(rr.tok)
    qs, docs = _text_pairs("bert")
    docs[1][0] = docs[0][1]  # a chunk shared by two queries is tokenized once
    first = rr.score(qs, docs)
    flat_docs = {d for row in docs for d in row}
    assert sorted(map(len, rr.tok.calls)) == sorted([len(qs), len(flat_docs)])
    rr.tok.calls.clear()
    second = rr.score(["another question"] + qs[1:], docs)
    assert [len(c) for c in rr.tok.calls] == [len(qs)]  # the queries only
    assert all(np.array_equal(a, b) for a, b in zip(first[1:], second[1:]))
    assert len(rr.cache) == len(flat_docs) and rr.cache.tokens == sum(len(v) for v in rr.cache._d.values())


def test_cache_eviction_respects_the_token_bound():
    c = TokenCache(10)
    for name, n in (("a", 4), ("b", 4)):
        c.put(name, np.zeros(n, dtype=np.int32))
    assert c.get("a") is not None  # "a" is now the most recently used
    c.put("c", np.zeros(4, dtype=np.int32))  # 12 > 10: the least recently used ("b") goes
    assert c.get("b") is None and c.get("a") is not None and c.get("c") is not None and c.tokens == 8
    c.put("huge", np.zeros(11, dtype=np.int32))  # never fits: not cached, nothing evicted for it
    assert c.get("huge") is None and c.tokens == 8
    c.put("a", np.zeros(2, dtype=np.int32))  # replacing an entry keeps the count right
    assert c.tokens == 6
    rr = C.load_reranker(C.checkpoint("bert", 128, 2), "cpu", cache_tokens=70)
    qs, docs = _text_pairs("bert")
    full = C.load_reranker(C.checkpoint("bert", 128, 2), "cpu").score(qs, docs)
    got = rr.score(qs, docs)
    assert 0 < rr.cache.tokens <= 70 and len(rr.cache) < 12
    assert all(np.array_equal(a, b) for a, b in zip(full, got))  # a small cache changes no score


def test_cache_is_thread_safe():
    import threading

    c = TokenCache(500)
    def work(t):
        for i in range(300):
            c.put("k%d" % ((i * 7 + t) % 40), np.zeros(1 + (i + t) % 30, dtype=np.int32))
            c.get("k%d" % (i % 40))
    ts = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert c.tokens == sum(len(v) for v in c._d.values()) <= 500


# ------------------------------------------------------------------------------------------ Reranker.rerank
def test_rerank_copies_metadata_and_keeps_distances():
    rr = C.load_reranker(C.checkpoint("bert", 128, 2), "cpu")
    qs, docs = _text_pairs("bert")
    store = [[{"filename": "f%d" % q, "chunk_id": i, "text": d} for i, d in enumerate(row)] for q, row in enumerate(docs)]
    results = [[(m, 0.25 * i) for i, m in enumerate(row)] for row in store]
    results[2] = results[2][:2]  # ragged
    results.append([])
    out = rr.rerank(qs + ["nothing found"], results, k=3)
    scores = rr.score(qs, [[m["text"] for m, _ in r] for r in results[:3]])
    for q in range(3):
        order = sorted(range(len(results[q])), key=lambda i: -scores[q][i])[:3]
        assert [m["chunk_id"] for m, _ in out[q]] == order
        assert [d for _, d in out[q]] == [0.25 * i for i in order]
        assert [m["rerank_score"] for m, _ in out[q]] == [float(scores[q][i]) for i in order]
    assert len(out[2]) == 2 and out[3] == []
    assert not any("rerank_score" in m for row in store for m in row)
    with pytest.raises(ValueError, match="64"):
        rr.rerank(["q"], [[({"text": "x"}, 0.0)] * 65], k=3)


# ------------------------------------------------------------------------------------------ service
CAND = 8
PROMPT = "Pleabra tisho quar?"


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    from rag_llm_k8s_amd.models import gpt2 as G2

    root = tmp_path_factory.mktemp("models")
    G2.write_gpt2_checkpoint(str(root), G2.gpt2_tiny(1024), seed=0)
    ecfg = E.EncoderConfig(vocab_size=C.VOCAB, hidden_size=128, num_hidden_layers=2, num_attention_heads=4,
                           intermediate_size=256, max_seq_length=128)
    C.train_tokenizer(str(root / "minilm"), "bert")
    S.write_encoder_checkpoint(str(root / "minilm"), ecfg, seed=0)
    pdfs = tmp_path_factory.mktemp("pdfs")
    S.write_pdf_corpus(str(pdfs), 4, pages=2, words_per_page=900)
    return root, pdfs, C.checkpoint("bert", 128, 2)


def _cfg(assets, index_dir, rerank=True, **kw):
    root, pdfs, ce = assets
    return RagConfig(model_path=str(root), index_path=str(index_dir / "faiss_index"), pdf_dir=str(pdfs),
                     embed_model=str(root / "minilm"), device="cpu", max_new_tokens=4, max_model_len=1024,
                     max_batch=4, use_cuda_graphs=False, kv_cache_blocks=64, seed=1,
                     rerank_model=ce if rerank else "", rerank_candidates=CAND, rerank_max_len=C.MAX_LEN, **kw)


def _service(cfg):
    from rag_llm_k8s_amd.server.builder import build_service

    svc = build_service(cfg)
    svc.store.ensure_exists()
    assert svc.ingest_directory() == 4
    svc.ready = True
    return svc


@pytest.fixture(scope="module")
def services(assets, tmp_path_factory):
    from rag_llm_k8s_amd.server.app import create_app

    on = _service(_cfg(assets, tmp_path_factory.mktemp("index_on")))
    off = _service(_cfg(assets, tmp_path_factory.mktemp("index_off"), rerank=False))
    assert on.reranker is not None and off.reranker is None and on.store.index.ntotal > CAND
    yield create_app(on).test_client(), on, create_app(off).test_client(), off
    on.shutdown()
    off.shutdown()


def _post(client, svc, body, seed=500):
    svc._seed = seed  # the next request samples with seed + 1
    r = client.post("/generate", json=body)
    assert r.status_code == 200, r.get_json()
    return r.get_json()


def _expected(svc, prompt, filenames=None):
    """The L2 candidates of a prompt and their order by an independent sort on the reranker's scores."""
    q = svc.embedder.embed([prompt])
    kw = {"filters": [tuple(filenames)]} if filenames else {}
    cands = svc.store.search(q, CAND, **kw)[0]
    scores = svc.reranker.score([prompt], [[m["text"] for m, _ in cands]])[0]
    order = sorted(range(len(cands)), key=lambda i: -float(scores[i]))
    return cands, order, scores


def _chunks(context):
    return re.findall(r"Document '([^']+)' \(chunk (\d+), score: ([0-9.]+)\)", context)


def test_context_is_in_reranked_order_with_l2_scores(services):
    c_on, on, _, _ = services
    cands, order, scores = _expected(on, PROMPT)
    assert len(cands) == CAND and len(set(np.round(scores, 4))) == CAND
    top = order[:on.cfg.context_k]
    assert top != list(range(on.cfg.context_k)), "pick a prompt whose reranked order differs from the L2 order"
    j = _post(c_on, on, {"prompt": PROMPT})
    assert set(j) == {"generated_text", "context"}
    assert j["context"] == build_context([cands[i] for i in order[:on.cfg.retrieve_k]], on.cfg.context_k)
    got = _chunks(j["context"])
    assert [(f, int(ch)) for f, ch, _ in got] == [(cands[i][0]["filename"], cands[i][0]["chunk_id"]) for i in top]
    assert [s for _, _, s in got] == ["%.4f" % cands[i][1] for i in top]  # score: stays the L2 distance


def test_rerank_false_is_the_unreranked_response(services):
    c_on, on, c_off, off = services
    plain = _post(c_off, off, {"prompt": PROMPT})
    assert _post(c_on, on, {"prompt": PROMPT, "rerank": False}) == plain
    assert _post(c_on, on, {"prompt": PROMPT}) != plain
    # RERANK_MODEL unset: the bi-encoder order, the reference's response keys, no second-stage fields
    q = off.embedder.embed([PROMPT])
    assert plain["context"] == build_context(off.store.search(q, off.cfg.retrieve_k)[0], off.cfg.context_k)
    dbg = _post(c_off, off, {"prompt": PROMPT, "debug": True})
    assert "retrieved" not in dbg and "rerank" not in dbg["timings_ms"]
    assert {k: dbg[k] for k in ("generated_text", "context")} == plain
    assert _post(c_off, off, {"prompt": PROMPT, "rerank": False}) == plain
    r = c_off.post("/generate", json={"prompt": PROMPT, "rerank": True})
    assert r.status_code == 500 and "RERANK_MODEL" in r.get_json()["error"]


def test_mixed_micro_batch_gives_each_request_its_own_result(services):
    _, on, _, off = services
    prompts = [PROMPT, "Grea stou bich?", PROMPT, "Thraiz plo?"]
    flags = [None, False, False, True]
    batch = on._retrieve_batch([(p, None, f) for p, f in zip(prompts, flags)])
    for p, f, (res, spans) in zip(prompts, flags, batch):
        alone = on._retrieve_batch([(p, None, f)])[0][0]
        # (the fp32 distances of a batched and a single search differ in the last bits on the CPU)
        assert [(m["filename"], m["chunk_id"]) for m, _ in res] == [(m["filename"], m["chunk_id"]) for m, _ in alone]
        assert [d for _, d in res] == pytest.approx([d for _, d in alone], rel=1e-5)
        assert len(res) == on.cfg.retrieve_k and "rerank" in spans
        if f is False:
            plain = off._retrieve_batch([(p, None)])[0][0]
            assert [m for m, _ in res] == [m for m, _ in plain] and "rerank_score" not in res[0][0]
        else:
            cands, order, _ = _expected(on, p)
            assert [m["chunk_id"] for m, _ in res] == [cands[i][0]["chunk_id"] for i in order[:on.cfg.retrieve_k]]
            assert all("rerank_score" in m for m, _ in res)
    assert "rerank" not in on._retrieve_batch([(PROMPT, None, False)])[0][1]  # nobody asked: no second stage


def test_filtered_request_is_reranked_within_its_files(services):
    c_on, on, _, _ = services
    name = on.documents()[1]["filename"]
    cands, order, _ = _expected(on, PROMPT, [name])
    assert 1 < len(cands) <= CAND and all(m["filename"] == name for m, _ in cands)
    j = _post(c_on, on, {"prompt": PROMPT, "filenames": [name], "debug": True})
    assert j["context"] == build_context([cands[i] for i in order[:on.cfg.retrieve_k]], on.cfg.context_k)
    assert all(r["filename"] == name for r in j["retrieved"])


def test_debug_fields_and_metrics(services):
    c_on, on, _, _ = services
    j = _post(c_on, on, {"prompt": PROMPT, "debug": True})
    assert j["timings_ms"]["rerank"] > 0 and {"embed", "search"} <= set(j["timings_ms"])
    cands, order, scores = _expected(on, PROMPT)
    assert len(j["retrieved"]) == on.cfg.retrieve_k
    for r, i in zip(j["retrieved"], order):
        assert set(r) == {"filename", "chunk_id", "distance", "rerank_score"}
        assert (r["filename"], r["chunk_id"]) == (cands[i][0]["filename"], cands[i][0]["chunk_id"])
        assert r["distance"] == pytest.approx(cands[i][1]) and r["rerank_score"] == pytest.approx(float(scores[i]))
    j = _post(c_on, on, {"prompt": PROMPT, "debug": True, "rerank": False})
    assert all(r["rerank_score"] is None for r in j["retrieved"])
    assert b'stage="rerank"' in c_on.get("/metrics").data


def test_store_metadata_is_never_mutated(services):
    c_on, on, _, _ = services
    _post(c_on, on, {"prompt": PROMPT})
    assert on.store.metadata and all(set(m) == {"filename", "chunk_id", "text"} for m in on.store.metadata)


def test_generate_batch_reranks_and_reports_chunks(assets, tmp_path):
    from rag_llm_k8s_amd.server.builder import build_service

    svc = build_service(_cfg(assets, tmp_path), start_threads=False)
    try:
        svc.store.ensure_exists()
        svc.ingest_directory()
        prompts = [PROMPT, "Grea stou bich?"]
        outs = svc.generate_batch(prompts, seeds=[7, 8], rerank=[None, False])
        cands, order, _ = _expected(svc, PROMPT)
        assert outs[0]["_retrieved"] == [(cands[i][0]["filename"], cands[i][0]["chunk_id"])
                                         for i in order[:svc.cfg.retrieve_k]]
        q = svc.embedder.embed([prompts[1]])
        assert outs[1]["_retrieved"] == [(m["filename"], m["chunk_id"])
                                         for m, _ in svc.store.search(q, svc.cfg.retrieve_k)[0]]
        assert outs[0]["context"] == build_context([cands[i] for i in order], svc.cfg.context_k)
    finally:
        svc.shutdown()


@pytest.mark.parametrize("n", [4, 65, 0])
def test_candidates_outside_the_range_are_refused_at_start_up(assets, tmp_path, monkeypatch, n):
    from rag_llm_k8s_amd.server.builder import build_reranker

    monkeypatch.setenv("RERANK_MODEL", assets[2])
    monkeypatch.setenv("RERANK_CANDIDATES", str(n))
    with pytest.raises(ValueError, match="RERANK_CANDIDATES"):
        RagConfig.from_env()
    cfg = _cfg(assets, tmp_path)
    cfg.rerank_candidates = n  # a config built in code is checked when the reranker is built
    with pytest.raises(ValueError, match="RERANK_CANDIDATES"):
        build_reranker(cfg, "cpu")
    monkeypatch.setenv("RERANK_MODEL", "")
    assert RagConfig.from_env().rerank_model == ""  # off: the candidate count is not looked at


def test_config_defaults_and_bounds(assets, monkeypatch):
    c = RagConfig()
    assert (c.rerank_model, c.rerank_candidates, c.rerank_max_len, c.rerank_batch_tokens) == ("", 32, 512, 65536)
    monkeypatch.setenv("RERANK_MODEL", assets[2])
    for n in (5, 32, 64):
        monkeypatch.setenv("RERANK_CANDIDATES", str(n))
        assert RagConfig.from_env().rerank_candidates == n
    from rag_llm_k8s_amd.server.builder import build_reranker

    with pytest.raises(FileNotFoundError, match="RERANK_MODEL"):
        build_reranker(RagConfig(rerank_model="/nonexistent/reranker"), "cpu")
    rr = build_reranker(RagConfig(rerank_model=assets[2], rerank_max_len=512), "cpu")
    assert rr.max_len == C.MAX_LEN  # capped by the model's positions
