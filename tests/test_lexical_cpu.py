"""Hybrid retrieval on the CPU: the analyzer (C++ runtime == pure-Python twin), the fp32 BM25 replica of
ops/reference.py against an independent float64 oracle, reciprocal rank fusion against a hand-computed table, the
LexicalIndex, the store (tombstones, compaction, reload, texts=None), the configuration, and the service with
tiny synthetic models (a chunk only the lexical list can find reaches the context with "hybrid": true)."""
import os
import re

import numpy as np
import pytest
import torch

import lexical_cases as C
from rag_llm_k8s_amd.config import RagConfig
from rag_llm_k8s_amd.index import lexical as LX
from rag_llm_k8s_amd.index.store import DocumentStore
from rag_llm_k8s_amd.ingest.text import build_context
from rag_llm_k8s_amd.ops import reference as R

GOLDEN_PDF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                          "tr_technology_radar_vol_29_en.text_only.pdf")


# ------------------------------------------------------------------------------------------ analyzer
def _golden_text():
    from rag_llm_k8s_amd.ingest.pdf import extract_text

    with open(GOLDEN_PDF, "rb") as f:
        return extract_text(f.read())


ANALYZER_TEXTS = {
    "ascii": "the quick brown fox jumps over the lazy dog the end",
    "mixed_case": "Hello hELLO HELLO World wOrLd",
    "digits_joined": "error E1234x code 42 v2 2v x86_64 id0007x",
    "punctuation_only": "... ,;: !? -- (){}[] \t\n",
    "empty": "",
    "multibyte": "café CAFÉ naïve 日本語 日本語abc \U0001f600 École école",
    "saturating_tf": "word " * 70000 + "once",
}


def _equal_csr(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(ANALYZER_TEXTS) + ["golden_pdf", "batch"])
def test_native_analyzer_equals_the_python_twin(name):
    from rag_llm_k8s_amd.runtime import native_rt

    rt = native_rt()
    assert rt is not None and hasattr(rt, "lex_analyze_batch"), "the C++ runtime with the analyzer must be built"
    if name == "batch":
        texts = list(ANALYZER_TEXTS.values())
    else:
        texts = [_golden_text() if name == "golden_pdf" else ANALYZER_TEXTS[name]]
    got, want = LX.analyze_batch(texts, use_native=True), LX.py_analyze_batch(texts)
    assert _equal_csr(got, want)
    rp, terms, tf, dl = want
    assert rp.dtype == np.int64 and terms.dtype == np.uint32 and tf.dtype == np.uint16 and dl.dtype == np.int32
    for i in range(len(texts)):
        row = terms[rp[i]:rp[i + 1]]
        assert (np.diff(row.astype(np.int64)) > 0).all()  # distinct, ascending as unsigned
        assert np.array_equal(np.asarray(rt.lex_tokens(LX._utf8(texts[i])), dtype=np.uint32),
                              np.asarray(LX.py_tokens(texts[i]), dtype=np.uint32))
    if name == "golden_pdf":
        assert dl[0] > 1000 and len(terms) > 500
    if name == "empty" or name == "punctuation_only":
        assert dl.tolist() == [0] and len(terms) == 0 and rp.tolist() == [0, 0]


def test_analyzer_rules():
    h = LX.fnv1a32
    assert (h(b"a"), h(b"hello")) == (0xE40C292C, 0x4F9F2CAB)  # published FNV-1a 32 vectors
    rp, terms, tf, dl = LX.py_analyze_batch([ANALYZER_TEXTS["mixed_case"]])
    assert sorted(terms.tolist()) == sorted({h(b"hello"), h(b"world")}) and dl.tolist() == [5]
    assert dict(zip(terms.tolist(), tf.tolist())) == {h(b"hello"): 3, h(b"world"): 2}
    # digits join letters; '_' and '-' split
    toks = LX.py_tokens("E1234x x86_64 a-b")
    assert toks == [h(b"e1234x"), h(b"x86"), h(b"64"), h(b"a"), h(b"b")]
    # non-ASCII bytes are kept and not lowered: "É" (c3 89) and "é" (c3 a9) are different terms, "CAFÉ" lowers only
    # its ASCII letters
    e_up, e_lo = "É".encode(), "é".encode()
    assert LX.py_tokens("École école") == [h(e_up + b"cole"), h(e_lo + b"cole")]
    assert LX.py_tokens("CAFÉ") == [h(b"caf" + e_up)]
    assert LX.py_tokens("日本語abc") == [h("日本語".encode() + b"abc")]
    # tf saturates, the length does not
    rp, terms, tf, dl = LX.py_analyze_batch([ANALYZER_TEXTS["saturating_tf"]])
    assert dict(zip(terms.tolist(), tf.tolist())) == {h(b"word"): 65535, h(b"once"): 1} and dl.tolist() == [70001]
    # a query keeps its first 64 distinct terms in order of appearance
    q = " ".join("t%d" % (i % 70) for i in range(200))
    assert LX.query_terms(q) == [h(b"t%d" % i) for i in range(64)]
    assert LX.doc_text({"text": "x"}) == "x" and LX.doc_text({"filename": "f"}) == "" and LX.doc_text("str") == ""


def test_padding_id_is_remapped():
    from rag_llm_k8s_amd.runtime import native_rt

    rt = native_rt()
    assert rt is not None
    for fn in (LX.lex_remap, rt.lex_remap):
        assert fn(0xFFFFFFFF) == 0xFFFFFFFE and fn(0xFFFFFFFE) == 0xFFFFFFFE and fn(0) == 0 and fn(12345) == 12345


# ------------------------------------------------------------------------------------------ replica vs float64
def _replica(case):
    t = case.tensors()
    df = R.lex_df(t["row_ptr"], t["terms"], case.n, t["qterms"], live=t["live"])
    idf, avgdl = case.host_numbers(df.numpy())
    k1p1 = float(np.float32(C.K1) + np.float32(1))
    S, I = R.lex_search(t["row_ptr"], t["terms"], t["tf"], t["doc_len"], case.n, t["qterms"], idf, t["member"],
                        len(case.queries), C.K1, k1p1, C.B, avgdl, case.k, masks=t["masks"], qmask=t["qmask"])
    return t, df, S, I


@pytest.mark.parametrize("case", C.replica_cases(), ids=repr)
def test_replica_against_float64_oracle(case):
    t, df, S, I = _replica(case)
    oracle, odf = case.oracle()
    T = t["qterms"].numel()
    bound = C.rel_bound(T)
    assert df.tolist() == [odf.get(int(x) & 0xFFFFFFFF, 0) for x in t["qterms"].tolist()]
    for qi, res in enumerate(oracle):
        top = res[:case.k + 1]
        for (s0, _), (s1, _) in zip(top, top[1:]):
            # the case data: neighbouring float64 scores are exactly tied (equal tf and lengths: the fp32 values tie
            # too) or farther apart than both fp32 errors together
            assert s0 == s1 or (s0 - s1) > 2 * bound * s0, (case, qi, s0, s1)
        want_ids = [d for _, d in res[:case.k]]
        assert I[qi].tolist() == want_ids + [-1] * (case.k - len(want_ids))
        for j, (s, _) in enumerate(res[:case.k]):
            assert abs(float(S[qi, j]) - s) <= bound * s
        assert S[qi, len(want_ids):].tolist() == [0.0] * (case.k - len(want_ids))


def test_replica_exact_ties_come_out_lowest_id_first():
    case = [c for c in C.edge_cases() if c.name == "identical_docs"][0]
    _, _, S, I = _replica(case)
    assert I[0].tolist() == list(range(64)) and I[1].tolist() == list(range(64))
    assert len(set(S[0].tolist())) == 1
    case = [c for c in C.edge_cases() if c.name == "ties_across_tiles"][0]
    _, _, S, I = _replica(case)
    for qi in range(2):
        tied = [i for i in I[qi].tolist() if i in (10, 63, 64, 70, 199)]
        assert tied == [10, 63, 64, 70, 199]


def test_replica_refusals():
    t = C.n_sweep()[1].tensors()
    big = torch.arange(4097, dtype=torch.int32)
    with pytest.raises(ValueError, match="4096"):
        R.lex_df(t["row_ptr"], t["terms"], 63, big)
    with pytest.raises(ValueError, match="ascending"):
        R.lex_df(t["row_ptr"], t["terms"], 63, torch.tensor([5, 4], dtype=torch.int32))
    one = torch.ones(2)
    with pytest.raises(ValueError, match="k <= 64"):
        R.lex_search(t["row_ptr"], t["terms"], t["tf"], t["doc_len"], 63, torch.tensor([4, 5], dtype=torch.int32), one,
                     one.long(), 1, 1.2, 2.2, 0.75, 3.0, 65)


# ------------------------------------------------------------------------------------------ RRF
def test_rrf_hand_table():
    dense = [7, 3, 9, 4]     # ranks 1..4
    lexical = [3, 5, -1, -1]  # shorter than the depth: padded
    got = LX.rrf_fuse([dense, lexical], 60, 10)
    want = {3: 1 / 62 + 1 / 61,  # in both lists
            5: 1 / 62, 7: 1 / 61, 9: 1 / 63, 4: 1 / 64}
    assert [i for i, _ in got] == [3, 7, 5, 9, 4]
    for i, f in got:
        assert f == want[i]
    # the 1/61 tie (rank 1 of either list) is broken by id
    assert [i for i, _ in LX.rrf_fuse([[8, 1], [2, 1]], 60, 3)] == [1, 2, 8]
    assert LX.rrf_fuse([[8, 1], [2, 1]], 60, 3)[0][1] == 1 / 62 + 1 / 62
    assert [i for i, _ in LX.rrf_fuse([[8], [2]], 60, 1)] == [2]  # cut to k after the tie-break
    assert LX.rrf_fuse([[], [-1, -1]], 60, 5) == []
    assert LX.rrf_fuse([[4, 6], []], 1.5, 5) == [(4, 1 / 2.5), (6, 1 / 3.5)]


# ------------------------------------------------------------------------------------------ LexicalIndex
TEXTS = ["alpha beta gamma id%04dx %s" % (i, " ".join("w%d" % ((i * 7 + j) % 23) for j in range(i % 11)))
         for i in range(90)]


def _state_equal(a, b):
    sa, sb = a.state(), b.state()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


def test_index_add_in_pieces_and_compact():
    once = LX.LexicalIndex("cpu")
    once.add(TEXTS)
    pieces = LX.LexicalIndex("cpu", capacity=2, entry_capacity=4)  # every add grows it
    for a, b in ((0, 1), (1, 2), (2, 40), (40, 40), (40, 90)):
        pieces.add(TEXTS[a:b])
    twin = LX.LexicalIndex("cpu")
    twin.add(TEXTS, use_native=False)
    assert once.ntotal == pieces.ntotal == 90 and _state_equal(once, pieces) and _state_equal(once, twin)
    keep = np.asarray([i for i in range(90) if i % 4 != 2])
    pieces.compact(keep)
    fresh = LX.LexicalIndex("cpu")
    fresh.add([TEXTS[i] for i in keep])
    assert pieces.ntotal == len(keep) and _state_equal(pieces, fresh)
    s0, i0 = pieces.search(["id0005x beta", "w3 w4"], 6)
    s1, i1 = fresh.search(["id0005x beta", "w3 w4"], 6)
    assert torch.equal(s0, s1) and torch.equal(i0, i1) and int(i0[0, 0]) == list(keep).index(5)
    pieces.compact(np.zeros(0, np.int64))
    assert pieces.ntotal == 0 and pieces.nnz == 0 and pieces.search(["beta"], 3)[1].tolist() == [[-1, -1, -1]]
    with pytest.raises(ValueError):
        fresh.compact([3, 2])


def test_index_search_splits_more_than_64_queries():
    idx = LX.LexicalIndex("cpu")
    idx.add(TEXTS)
    qs = ["id%04dx gamma" % i for i in range(70)]
    S, I = idx.search(qs, 3)
    assert I[:, 0].tolist() == list(range(70))
    for j in (0, 63, 64, 69):
        s, i = idx.search([qs[j]], 3)
        assert torch.equal(i[0], I[j]) and torch.equal(s[0], S[j])


# ------------------------------------------------------------------------------------------ store
def _store(path, index_type="flat", **kw):
    rng = np.random.default_rng(5)
    vecs = rng.standard_normal((90, 16)).astype(np.float32)
    st = DocumentStore(str(path), 16, device="cpu", index_type=index_type, ivf_nlist=4, ivf_nprobe=4, lexical=True,
                       hybrid_candidates=8, **kw)
    meta = [{"filename": "f%d.pdf" % (i % 5), "chunk_id": i // 5, "text": t} for i, t in enumerate(TEXTS)]
    st.add(vecs, meta, persist=False)
    return st, vecs, meta


def _ids(res):
    return [[(m["filename"], m["chunk_id"]) for m, _ in r] for r in res]


@pytest.mark.parametrize("index_type", ["flat", "ivf"])
def test_store_hybrid_search_tombstones_compaction_reload(tmp_path, index_type):
    st, vecs, meta = _store(tmp_path / "idx", index_type)
    assert st.lexical.ntotal == st.index.ntotal == 90
    q = vecs[[1, 2]] + 0.01
    texts = ["id0040x zzz", "id0077x beta"]  # chunks 40 (f0.pdf) and 77 (f2.pdf)
    res = st.search(q, 5, texts=texts)
    for j, want in enumerate((40, 77)):
        hit = [(m, d) for m, d in res[j] if m["text"] == TEXTS[want]]
        assert hit and hit[0][0]["lexical_rank"] == 1 and hit[0][0]["dense_rank"] is None
        ref = float(((vecs[want].astype(np.float64) - q[j]) ** 2).sum())
        assert abs(hit[0][1] - ref) <= 18 * 2.0 ** -24 * ref  # index.distances: (d + 2) * 2^-24 with d = 16
    # query 0's lexical list is chunk 40 alone: it ties with the dense winner (chunk 1) at 1/61, the lower id leads
    assert [(m["text"], m["dense_rank"], m["lexical_rank"]) for m, _ in res[0][:2]] == [(TEXTS[1], 1, None),
                                                                                         (TEXTS[40], None, 1)]
    assert all(set(m) == {"filename", "chunk_id", "text"} for m in st.metadata)  # copies carry the ranks
    # texts=None (and all-None texts) is the old call
    plain = st.search(q, 5)
    assert st.search(q, 5, texts=None) == plain and st.search(q, 5, texts=[None, None]) == plain
    D0, I0 = st.index.search(q, 5)
    assert [[d for _, d in r] for r in plain] == D0.tolist()
    mixed = st.search(q, 5, texts=[texts[0], None])
    assert _ids(mixed)[0] == _ids(res)[0] and mixed[1] == st.search(q[1:], 5)[0]
    # df and avgdl follow the live set: "beta" is in every chunk, so its df is the live count
    n_live, avgdl = st.lexical.live_stats(None)
    assert n_live == 90
    s_before = [m["lexical_score"] for m, _ in res[1] if m["text"] == TEXTS[77]][0]
    assert st.delete("f0.pdf", persist=False) == 18
    res2 = st.search(q, 5, texts=texts)  # the tombstones take effect in the very next search
    assert all(m["filename"] != "f0.pdf" for r in res2 for m, _ in r)
    assert not any(m["text"] == TEXTS[40] for m, _ in res2[0])
    live = np.asarray([i % 5 != 0 for i in range(90)])
    n_live2, avgdl2 = st.lexical.live_stats(live)
    assert n_live2 == 72 and avgdl2 != avgdl
    s_after = [m["lexical_score"] for m, _ in res2[1] if m["text"] == TEXTS[77]][0]
    assert s_after != s_before
    # ... and equal a store that never held the deleted document
    never = DocumentStore(str(tmp_path / "never"), 16, device="cpu", index_type=index_type, ivf_nlist=4, ivf_nprobe=4,
                          lexical=True, hybrid_candidates=8)
    if index_type == "ivf":
        never.index.train(vecs)  # the same centroids as the store that saw every vector
    never.add(vecs[live], [m for m, lv in zip(meta, live) if lv], persist=False)
    want = never.search(q, 5, texts=texts)
    assert _ids(res2) == _ids(want)
    assert [[m["lexical_score"] for m, _ in r] for r in res2] == [[m["lexical_score"] for m, _ in r] for r in want]
    # compaction at the snapshot keeps the results
    st.persist()
    assert st.lexical.ntotal == st.index.ntotal == 72 and st._live is None
    res3 = st.search(q, 5, texts=texts)
    assert _ids(res3) == _ids(res2)
    assert [[m["lexical_score"] for m, _ in r] for r in res3] == [[m["lexical_score"] for m, _ in r] for r in res2]
    # a reload rebuilds the index from the metadata texts
    again = DocumentStore(str(tmp_path / "idx"), 16, device="cpu", index_type=index_type, ivf_nlist=4, ivf_nprobe=4,
                          lexical=True, hybrid_candidates=8).ensure_exists()
    assert again.lexical.ntotal == 72 and _state_equal(again.lexical, st.lexical)
    assert _ids(again.search(q, 5, texts=texts)) == _ids(res3)
    # filters: the same masks for both lists
    flt = st.search(q, 5, filters=[("f2.pdf",), ("f1.pdf",)], texts=texts)
    assert all(m["filename"] == "f2.pdf" for m, _ in flt[0]) and all(m["filename"] == "f1.pdf" for m, _ in flt[1])
    assert not any(m["text"] == TEXTS[77] for m, _ in flt[1])


def test_store_without_a_lexical_index_refuses_texts(tmp_path):
    st = DocumentStore(str(tmp_path / "i"), 4, device="cpu")
    st.add(np.eye(4, dtype=np.float32), [{"filename": "a", "chunk_id": i, "text": "t%d" % i} for i in range(4)],
           persist=False)
    assert st.lexical is None
    with pytest.raises(ValueError, match="lexical"):
        st.search(np.eye(4, dtype=np.float32)[:1], 2, texts=["t1"])
    with pytest.raises(ValueError, match="sharded|INDEX_SHARDED"):
        DocumentStore(str(tmp_path / "s"), 4, device="cpu", shard=(None, 0, 2), lexical=True)
    for kw in ({"hybrid_candidates": 0}, {"hybrid_candidates": 65}, {"bm25_b": 1.5}, {"bm25_k1": -1}, {"rrf_k": 0}):
        with pytest.raises(ValueError):
            DocumentStore(str(tmp_path / "r"), 4, device="cpu", lexical=True, **kw)


def test_quarantine_resets_the_lexical_index(tmp_path):
    st, _, _ = _store(tmp_path / "idx")
    st.persist()
    with open(st.index_file, "wb") as f:
        f.write(b"not an index")
    st2 = DocumentStore(str(tmp_path / "idx"), 16, device="cpu", lexical=True).ensure_exists()
    assert st2.recovered and st2.lexical.ntotal == 0 and st2.index.ntotal == 0


# ------------------------------------------------------------------------------------------ configuration
def test_config_defaults_and_refusals(monkeypatch):
    c = RagConfig()
    assert (c.hybrid_search, c.hybrid_candidates, c.bm25_k1, c.bm25_b, c.rrf_k, c.hybrid) == ("off", 32, 1.2, 0.75, 60.0,
                                                                                            False)
    assert not RagConfig.from_env().hybrid
    monkeypatch.setenv("HYBRID_SEARCH", "rrf")
    c = RagConfig.from_env()
    assert c.hybrid and c.hybrid_candidates == 32
    for env, bad, good in (("HYBRID_SEARCH", "bm25", "rrf"), ("HYBRID_CANDIDATES", "31", "64"),
                           ("HYBRID_CANDIDATES", "65", "32"), ("BM25_K1", "-0.1", "0"), ("BM25_B", "1.01", "1"),
                           ("BM25_B", "-0.5", "0"), ("RRF_K", "0", "0.5")):
        monkeypatch.setenv(env, bad)
        with pytest.raises(ValueError, match=env):
            RagConfig.from_env()
        monkeypatch.setenv(env, good)
        RagConfig.from_env()
    monkeypatch.setenv("RETRIEVE_K", "40")  # the depth must cover retrieve_k
    monkeypatch.setenv("HYBRID_CANDIDATES", "32")
    with pytest.raises(ValueError, match="HYBRID_CANDIDATES"):
        RagConfig.from_env()
    monkeypatch.setenv("RETRIEVE_K", "5")
    monkeypatch.setenv("INDEX_SHARDED", "1")
    with pytest.raises(ValueError, match="INDEX_SHARDED"):
        RagConfig.from_env()
    monkeypatch.setenv("HYBRID_SEARCH", "off")
    assert RagConfig.from_env().index_sharded  # off: nothing of it is looked at
    monkeypatch.setenv("HYBRID_SEARCH", "")
    monkeypatch.setenv("HYBRID_CANDIDATES", "3")
    assert not RagConfig.from_env().hybrid


# ------------------------------------------------------------------------------------------ service
tokenizers = pytest.importorskip("tokenizers")
N_CHUNKS, HC, CAND = 80, 32, 8
ABSENT = "zzqxa zzqxb zzqxc"  # words no chunk holds


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    import rerank_cases as RC
    from rag_llm_k8s_amd.models import encoder as E
    from rag_llm_k8s_amd.models import gpt2 as G2
    from rag_llm_k8s_amd.utils import synthetic as S

    root = tmp_path_factory.mktemp("models")
    G2.write_gpt2_checkpoint(str(root), G2.gpt2_tiny(1024), seed=0)
    ecfg = E.EncoderConfig(vocab_size=RC.VOCAB, hidden_size=128, num_hidden_layers=2, num_attention_heads=4,
                           intermediate_size=256, max_seq_length=128)
    RC.train_tokenizer(str(root / "minilm"), "bert")
    S.write_encoder_checkpoint(str(root / "minilm"), ecfg, seed=0)
    wm = S.WordModel(n_words=3000, seed=3)
    rng = np.random.default_rng(11)
    chunks = ["id%04dx %s" % (i, " ".join(wm.sample(40, rng))) for i in range(N_CHUNKS)]
    assert not any(w in c.split() for c in chunks for w in ABSENT.split())
    return root, tmp_path_factory.mktemp("pdfs"), RC.checkpoint("bert", 128, 2), chunks


def _cfg(assets, index_dir, hybrid, rerank=False):
    import rerank_cases as RC

    root, pdfs, ce, _ = assets
    return RagConfig(model_path=str(root), index_path=str(index_dir / "faiss_index"), pdf_dir=str(pdfs),
                     embed_model=str(root / "minilm"), device="cpu", max_new_tokens=2, max_model_len=1024,
                     max_batch=4, use_cuda_graphs=False, kv_cache_blocks=64, seed=1,
                     hybrid_search="rrf" if hybrid else "off", hybrid_candidates=HC,
                     rerank_model=ce if rerank else "", rerank_candidates=CAND, rerank_max_len=RC.MAX_LEN)


def _service(assets, cfg):
    from rag_llm_k8s_amd.server.builder import build_service

    svc = build_service(cfg)
    svc.store.ensure_exists()
    chunks = assets[3]
    for f in range(4):  # four documents of 20 chunks
        svc._job_ingest(("doc%d.pdf" % f, chunks[20 * f:20 * f + 20], True, False))
    svc.ready = True
    return svc


@pytest.fixture(scope="module")
def services(assets, tmp_path_factory):
    from rag_llm_k8s_amd.server.app import create_app

    on = _service(assets, _cfg(assets, tmp_path_factory.mktemp("on"), True))
    off = _service(assets, _cfg(assets, tmp_path_factory.mktemp("off"), False))
    rr = _service(assets, _cfg(assets, tmp_path_factory.mktemp("rr"), True, rerank=True))
    assert on.store.lexical is not None and off.store.lexical is None and rr.reranker is not None
    assert on.store.index.ntotal == on.store.lexical.ntotal == N_CHUNKS
    yield {"on": (create_app(on).test_client(), on), "off": (create_app(off).test_client(), off),
           "rr": (create_app(rr).test_client(), rr)}
    for s in (on, off, rr):
        s.shutdown()


def _prompt(i):
    return "id%04dx %s" % (i, ABSENT)


@pytest.fixture(scope="module")
def hidden(services):
    """The chunks i that the dense search does not return within HYBRID_CANDIDATES for their own query (80 chunks,
    32 candidates: most of them) -- only the lexical list can bring them in. The first three."""
    _, on = services["on"]
    q = on.embedder.embed([_prompt(i) for i in range(N_CHUNKS)])
    _, I = on.store.index.search(q, HC)
    out = [i for i in range(N_CHUNKS) if i not in I[i].tolist()]
    assert out, "80 chunks > 64 candidates: some chunk must be outside the dense list"
    return out[:3]


def _post(client, svc, body, seed=500, status=200):
    svc._seed = seed
    r = client.post("/generate", json=body)
    assert r.status_code == status, r.get_json()
    return r.get_json()


def _chunks(context):
    return [(f, int(c), s) for f, c, s in re.findall(r"Document '([^']+)' \(chunk (\d+), score: ([0-9.]+)\)", context)]


def test_hybrid_brings_the_lexical_only_chunk_into_the_context(services, hidden):
    c_on, on = services["on"]
    c_off, off = services["off"]
    for i in hidden:
        name = ("doc%d.pdf" % (i // 20), i % 20)
        p = _prompt(i)
        q = on.embedder.embed([p])
        parent = build_context(off.store.search(q, off.cfg.retrieve_k)[0], off.cfg.context_k)
        assert name not in [(f, c) for f, c, _ in _chunks(parent)]
        for body in ({"prompt": p, "hybrid": True}, {"prompt": p}):  # HYBRID_SEARCH=rrf: on by default
            j = _post(c_on, on, dict(body, debug=True))
            got = _chunks(j["context"])
            assert name in [(f, c) for f, c, _ in got]
            row = [r for r in j["retrieved"] if (r["filename"], r["chunk_id"]) == name][0]
            assert row["dense_rank"] is None and row["lexical_rank"] == 1 and row["lexical_score"] > 0
            x = on.store.index.reconstruct_all()[i].astype(np.float64)
            ref = float(((x - q[0].double().numpy()) ** 2).sum())
            assert abs(row["distance"] - ref) <= (128 + 2) * 2.0 ** -24 * ref  # its real L2 distance
            assert [s for f, c, s in got if (f, c) == name] == ["%.4f" % row["distance"]]
            others = [r for r in j["retrieved"] if (r["filename"], r["chunk_id"]) != name]
            assert [r["dense_rank"] for r in others] == list(range(1, len(others) + 1))
            assert all(r["lexical_rank"] is None and r["lexical_score"] is None for r in others)
            assert "lexical" in j["timings_ms"] and "fuse" in j["timings_ms"]
        # "hybrid": false on the hybrid server, and the server without it, give the parent's bytes
        plain = _post(c_off, off, {"prompt": p})
        assert plain["context"] == parent and set(plain) == {"generated_text", "context"}
        assert _post(c_on, on, {"prompt": p, "hybrid": False}) == plain
        assert _post(c_off, off, {"prompt": p, "hybrid": False}) == plain
        dbg = _post(c_off, off, {"prompt": p, "debug": True})
        assert "retrieved" not in dbg and "lexical" not in dbg["timings_ms"]


def test_refused_requests_are_400(services):
    c_off, off = services["off"]
    c_on, on = services["on"]
    j = _post(c_off, off, {"prompt": _prompt(1), "hybrid": True}, status=400)
    assert "HYBRID_SEARCH" in j["error"]
    r = c_off.post("/query", json={"prompt": _prompt(1), "hybrid": True})
    assert r.status_code == 400
    for bad in ("yes", 1, [True]):
        assert "hybrid" in _post(c_on, on, {"prompt": _prompt(1), "hybrid": bad}, status=400)["error"]
    with pytest.raises(ValueError, match="HYBRID_SEARCH"):
        off.retrieve(_prompt(1), hybrid=True)


def test_mixed_micro_batch(services, hidden):
    _, on = services["on"]
    _, off = services["off"]
    i, j = hidden[0], hidden[1]
    items = [(_prompt(i), None, None, True), (_prompt(i), None, None, False), (_prompt(j), None, None, None),
             ("plain words only", None, None, False), (_prompt(j), ("doc%d.pdf" % (j // 20),), None, True)]
    batch = on._retrieve_batch(items)
    for it, (res, spans) in zip(items, batch):
        alone = on._retrieve_batch([it])[0][0]
        assert _ids(res and [res])[0] == _ids([alone])[0]
        assert [d for _, d in res] == pytest.approx([d for _, d in alone], rel=1e-5)
        if it[3] is False:  # exactly the dense result, in the same batch as queries that want hybrid
            dense = off._retrieve_batch([(it[0], it[1])])[0][0]
            assert [m for m, _ in res] == [m for m, _ in dense]
            assert [d for _, d in res] == pytest.approx([d for _, d in dense], rel=1e-5)
            assert "dense_rank" not in res[0][0]
        else:
            want = i if it[0] == _prompt(i) else j
            assert any(m["text"].startswith("id%04dx " % want) and m["lexical_rank"] == 1 for m, _ in res)
    assert "lexical" in batch[0][1] and "lexical" not in on._retrieve_batch([items[1]])[0][1]


def test_hybrid_with_a_filenames_filter(services, hidden):
    c_on, on = services["on"]
    i = hidden[0]
    own, other = "doc%d.pdf" % (i // 20), "doc%d.pdf" % ((i // 20 + 1) % 4)
    j = _post(c_on, on, {"prompt": _prompt(i), "hybrid": True, "filenames": [own], "debug": True})
    assert all(r["filename"] == own for r in j["retrieved"])
    assert (own, i % 20) in [(r["filename"], r["chunk_id"]) for r in j["retrieved"]]
    j = _post(c_on, on, {"prompt": _prompt(i), "hybrid": True, "filenames": [other], "debug": True})
    assert all(r["filename"] == other for r in j["retrieved"]) and len(j["retrieved"]) == on.cfg.retrieve_k
    assert all(r["lexical_rank"] is None for r in j["retrieved"])  # the masked lexical search cannot see chunk i


def test_hybrid_with_the_reranker_sees_the_fused_list(services, hidden):
    c_rr, rr = services["rr"]
    i = hidden[0]
    seen = []
    orig = rr.reranker.rerank

    def spy(queries, results, k):
        seen.append([[m["text"] for m, _ in r] for r in results])
        return orig(queries, results, k)

    rr.reranker.rerank = spy
    try:
        j = _post(c_rr, rr, {"prompt": _prompt(i), "debug": True})
        assert len(seen) == 1 and len(seen[0][0]) == CAND  # the search ran rerank_candidates deep
        assert any(t.startswith("id%04dx " % i) for t in seen[0][0]), "the cross-encoder did not see the fused list"
        fused = rr.store.search(rr.embedder.embed([_prompt(i)]), CAND, texts=[_prompt(i)])[0]
        assert seen[0][0] == [m["text"] for m, _ in fused]
        scores = rr.reranker.score([_prompt(i)], [[m["text"] for m, _ in fused]])[0]
        order = sorted(range(CAND), key=lambda c: -float(scores[c]))[:rr.cfg.retrieve_k]
        assert [(r["filename"], r["chunk_id"]) for r in j["retrieved"]] == \
               [(fused[c][0]["filename"], fused[c][0]["chunk_id"]) for c in order]
        assert all(set(r) >= {"rerank_score", "dense_rank", "lexical_rank", "lexical_score"} for r in j["retrieved"])
        seen.clear()
        k = _post(c_rr, rr, {"prompt": _prompt(i), "debug": True, "hybrid": False})
        assert not any(t.startswith("id%04dx " % i) for t in seen[0][0])
        assert all("dense_rank" not in r for r in k["retrieved"])
    finally:
        rr.reranker.rerank = orig


def test_generate_batch_hybrid_flags(assets, tmp_path, hidden):
    from rag_llm_k8s_amd.server.builder import build_service

    svc = build_service(_cfg(assets, tmp_path, True), start_threads=False)
    try:
        svc.store.ensure_exists()
        for f in range(4):
            svc._job_ingest(("doc%d.pdf" % f, assets[3][20 * f:20 * f + 20], True, False))
        i = hidden[0]
        outs = svc.generate_batch([_prompt(i), _prompt(i)], seeds=[7, 8], hybrid=[True, False])
        name = ("doc%d.pdf" % (i // 20), i % 20)
        assert name in [(f, c) for f, c, _ in _chunks(outs[0]["context"])]
        q = svc.embedder.embed([_prompt(i)])
        assert outs[1]["context"] == build_context(svc.store.search(q, svc.cfg.retrieve_k)[0], svc.cfg.context_k)
    finally:
        svc.shutdown()
