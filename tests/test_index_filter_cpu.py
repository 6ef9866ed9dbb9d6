"""Document delete / replace and filtered retrieval, CPU tier: the masked search of both index classes,
compact(keep), the DocumentStore scenario (tombstones, compaction at the snapshot, plain files on disk), the
service and Flask routes, and the oracle-side condition of the GPU random-mask cases."""
import io
import threading

import numpy as np
import pytest
import torch

import filter_cases as C
from rag_llm_k8s_amd.index.flat import FlatL2Index, mask_allowed, pack_masks
from rag_llm_k8s_amd.index.ivf import IVFFlatIndex
from test_service_cpu import assets, make_cfg, make_service  # noqa: F401  (assets: the tiny-model fixture)

FLT_MAX = C.FLT_MAX


# ------------------------------------------------------------------------------------------ bitmaps
def test_pack_masks_and_bit_lookup():
    al = np.zeros((2, 70), dtype=bool)
    al[0, [0, 31, 32, 63, 64, 69]] = True
    al[1, 33] = True
    m = pack_masks(al)
    assert m.dtype == np.uint32 and m.shape == (2, 3)
    assert m[0].tolist() == [(1 << 31) | 1, (1 << 31) | 1, 1 | (1 << 5)] and m[1].tolist() == [0, 2, 0]
    ids = np.array([0, 31, 32, 33, 63, 64, 69, 70, 95, 96, 10 ** 6, -1])
    got = mask_allowed(m, [0, 1, -1], ids)
    assert got[0].tolist() == [True, True, True, False, True, True, True] + [False] * 5  # >= 32 * words: not allowed
    assert got[1].tolist() == [False, False, False, True] + [False] * 8
    assert got[2].all()  # unfiltered
    with pytest.raises(ValueError):
        mask_allowed(m, [2], ids)


# ------------------------------------------------------------------------------------------ index classes
def _flat(xb):
    idx = FlatL2Index(xb.shape[1])
    idx.add(xb)
    return idx


def _ivf(xb, nlist, nprobe, centroids=None):
    idx = IVFFlatIndex(xb.shape[1], nlist=nlist, nprobe=nprobe)
    if centroids is None:
        idx.train(xb)
    else:
        idx._set_centroids(centroids)
    idx.add(xb)
    return idx


def test_flat_cpu_masked_search_matches_oracle_and_unmasked():
    xb, q = C.data(777, 96, 5)
    idx = _flat(xb)
    D0, I0 = idx.search(q, 10)
    ones = pack_masks(np.ones((1, 777), dtype=bool))
    D1, I1 = idx.search(q, 10, masks=ones, qmask=[0] * 5)
    assert torch.equal(D0, D1) and torch.equal(I0, I1)
    D2, I2 = idx.search(q, 10, masks=ones, qmask=[-1] * 5)
    assert torch.equal(D0, D2) and torch.equal(I0, I2)
    allowed, masks, qmask = C.random_masks(777, 5, 0.5)
    D, I = idx.search(q, 10, masks=masks, qmask=qmask)
    C.assert_within_two_swaps(D, I, *C.random_mask_oracle(777, 96, 5, 10, 0.5))
    assert all(allowed[j, i] for j in range(5) for i in I[j].tolist())


def test_flat_cpu_ties_go_to_the_lower_allowed_id():
    base = torch.randn(50, 32, generator=torch.Generator().manual_seed(3))
    idx = _flat(base.repeat(4, 1))  # row i == i + 50 == i + 100 == i + 150
    al = np.ones((1, 200), dtype=bool)
    al[0, :7] = False  # the lowest-id duplicate of the queried vectors
    D, I = idx._cpu_search(base[:7], 3, pack_masks(al), [0] * 7)
    for j in range(7):
        assert I[j].tolist() == [j + 50, j + 100, j + 150]


@pytest.mark.parametrize("kind", ["flat", "ivf"])
def test_padding_is_exact_with_fewer_allowed_rows_than_k(kind):
    """k > allowed rows: the tail is exactly (-1, FLT_MAX) -- through FlatL2Index._cpu_search and the IVF
    host search; different queries of one call carry different masks (3, 0, 1 and all rows allowed)."""
    xb, q = C.data(300, 64, 4, seed=2)
    al = np.zeros((3, 300), dtype=bool)
    al[0, [5, 64, 299]] = True
    al[2, [31]] = True
    masks, qmask, counts = pack_masks(al), [0, 1, 2, -1], [3, 0, 1, 300]
    if kind == "flat":
        D, I = _flat(xb)._cpu_search(q, 6, masks, qmask)
    else:
        idx = _ivf(xb, 8, 8)
        from rag_llm_k8s_amd.index.ivf import probes

        D, I = idx._search_host(q, probes(q, idx.centroids, idx._cnorm, 8), 6, masks, qmask)
    C.assert_padding(D, I, counts)
    assert sorted(I[0, :3].tolist()) == [5, 64, 299] and I[2, 0].item() == 31
    Dr, Ir = C.masked_oracle(xb, q, 6, mask_allowed(masks, qmask, np.arange(300)))
    assert torch.equal(I, Ir) and torch.allclose(D, Dr, rtol=1e-4, atol=1e-3)


def test_ivf_cpu_masked_search_full_probe_matches_flat():
    N, d, nlist = C.IVF_CASE
    xb, q = C.data(N, d, 6)
    idx = _ivf(xb, nlist, nlist)
    allowed, masks, qmask = C.random_masks(N, 6, 0.5)
    D, I = idx.search(q, 5, masks=masks, qmask=qmask)
    Dr, Ir = C.masked_oracle(xb, q, 5, allowed)
    assert torch.equal(I, Ir) and torch.allclose(D, Dr, rtol=1e-4, atol=1e-3)


def test_flat_compact_equals_fresh_index():
    xb, q = C.data(500, 48, 7, seed=4)
    keep = np.sort(np.random.default_rng(0).choice(500, 211, replace=False))
    idx = _flat(xb)
    idx.compact(keep)
    fresh = _flat(xb[torch.from_numpy(keep)])
    assert idx.ntotal == fresh.ntotal == 211
    D, I = idx.search(q, 9)
    Df, If = fresh.search(q, 9)
    assert torch.equal(D, Df) and torch.equal(I, If)
    assert np.array_equal(idx.reconstruct_all(), fresh.reconstruct_all())
    idx.add(xb[:3])  # appends land after the compacted rows
    assert idx.ntotal == 214 and np.array_equal(idx.reconstruct_all()[211:], xb[:3].numpy())
    idx.compact(np.zeros(0, dtype=np.int64))
    assert idx.ntotal == 0 and idx.search(q, 2)[1].eq(-1).all()
    for bad in ([3, 2], [0, 0], [-1], [500]):
        with pytest.raises(ValueError):
            _flat(xb).compact(np.asarray(bad))


def test_ivf_compact_equals_fresh_index_with_the_same_centroids():
    N, d, nlist = C.IVF_CASE
    xb, q = C.data(N, d, 6)
    keep = np.sort(np.random.default_rng(1).choice(N, 1300, replace=False))
    idx = _ivf(xb, nlist, nlist)
    cents = idx.centroids.clone()
    idx.compact(keep)
    fresh = _ivf(xb[torch.from_numpy(keep)], nlist, nlist, centroids=cents)
    assert idx.ntotal == fresh.ntotal == 1300 and torch.equal(idx.centroids, cents)
    for a, b in zip(idx.ids, fresh.ids):
        assert np.array_equal(a, b)
    for a, b in zip(idx.lists, fresh.lists):
        assert np.array_equal(a, b)
    D, I = idx.search(q, 8)
    Df, If = fresh.search(q, 8)
    assert torch.equal(I, If) and torch.equal(D, Df)
    idx.add(xb[:2])
    assert idx.ntotal == 1302 and sorted(np.concatenate(idx.ids).tolist()) == list(range(1302))


# ------------------------------------------------------------------------------------------ document store
@pytest.mark.parametrize("index_type", ["flat", "ivf"])
def test_store_delete_filter_compact_cpu(tmp_path, index_type):
    C.store_scenario(tmp_path, "cpu", index_type)


def test_sharded_store_refuses_delete_and_filters(tmp_path):
    from rag_llm_k8s_amd.index.store import DocumentStore

    store = DocumentStore(str(tmp_path / "faiss_index"), 16, shard=(None, 0, 1))
    v = np.random.default_rng(0).standard_normal((4, 16)).astype(np.float32)
    store.add(v, [{"filename": "a.pdf", "chunk_id": i, "text": "t"} for i in range(4)], persist=False)
    with pytest.raises(ValueError, match="INDEX_SHARDED"):
        store.delete("a.pdf")
    with pytest.raises(ValueError, match="INDEX_SHARDED"):
        store.search(v[:1], 2, filters=[["a.pdf"]])
    with pytest.raises(ValueError, match="INDEX_SHARDED"):
        store.add(v, [{"filename": "a.pdf", "chunk_id": i, "text": "t"} for i in range(4)], replace=True)
    assert len(store.search(v[:1], 2, filters=[None])[0]) == 2  # an empty filter list entry is no filter
    assert store.documents() == [{"filename": "a.pdf", "chunks": 4}]


# ------------------------------------------------------------------------------------------ service / Flask
def _pdf(tag, n_words):
    from rag_llm_k8s_amd.ingest.pdf import write_pdf

    return write_pdf([[" ".join("%s%d" % (tag, i) for i in range(n_words))]])


def _upload(c, name, data, replace=False):
    return c.post("/upload_pdf" + ("?replace=1" if replace else ""), data={"file": (io.BytesIO(data), name)},
                  content_type="multipart/form-data")


@pytest.fixture(scope="module")
def client(assets, tmp_path_factory):  # noqa: F811
    from rag_llm_k8s_amd.server.app import create_app

    root, pdfs = assets
    idx = tmp_path_factory.mktemp("index_filter")
    svc = make_service(make_cfg(root, pdfs, idx))
    assert svc.ingest_directory() == 3
    svc.ready = True
    yield create_app(svc).test_client(), svc
    svc.shutdown()


def _doc_chunks(svc):
    return {d["filename"]: d["chunks"] for d in svc.store.documents()}


def test_documents_route_lists_documents(client):
    c, svc = client
    r = c.get("/documents")
    assert r.status_code == 200
    docs = r.get_json()["documents"]
    assert [d["filename"] for d in docs] == ["doc_00000.pdf", "doc_00001.pdf", "doc_00002.pdf"]
    assert all(set(d) == {"filename", "chunks"} and d["chunks"] >= 1 for d in docs)
    assert sum(d["chunks"] for d in docs) == c.get("/index_info").get_json()["total_chunks"]


def test_generate_with_filenames_takes_context_from_those_files_only(client):
    c, svc = client
    for route in ("/generate", "/query"):
        r = c.post(route, json={"prompt": "Pleabra tisho quar?", "filenames": ["doc_00002.pdf"]})
        assert r.status_code == 200, r.get_json()
        j = r.get_json()
        assert set(j) == {"generated_text", "context"}
        assert j["context"].count("Document 'doc_00002.pdf'") == j["context"].count("(chunk ") == 3
    r = c.post("/generate", json={"prompt": "Pleabra tisho quar?", "filenames": ["unknown.pdf"]})
    assert r.status_code == 200
    from rag_llm_k8s_amd.ingest.text import NO_RESULTS

    assert r.get_json() == {"generated_text": NO_RESULTS}


def test_generate_without_filenames_is_unchanged(client):
    """No "filenames": the unfiltered search and the same response bytes -- equal to the same request with a
    filter naming every document (which allows every row) under the same sampling seed."""
    c, svc = client
    seen = []
    search = svc.store.search
    svc.store.search = lambda *a, **kw: (seen.append((len(a), sorted(kw))), search(*a, **kw))[1]
    try:
        svc._seed = 100
        plain = c.post("/generate", json={"prompt": "Pleabra tisho quar?"})
        assert seen == [(2, [])]  # store.search(q, k): today's call, no filter argument
        svc._seed = 100
        again = c.post("/generate", json={"prompt": "Pleabra tisho quar?"})
        svc._seed = 100
        empty = c.post("/generate", json={"prompt": "Pleabra tisho quar?", "filenames": []})
        svc._seed = 100
        every = c.post("/generate", json={"prompt": "Pleabra tisho quar?",
                                          "filenames": [d["filename"] for d in svc.store.documents()]})
        assert seen[-1] == (2, ["filters"])
    finally:
        svc.store.search = search
    assert plain.status_code == 200 and set(plain.get_json()) == {"generated_text", "context"}
    assert plain.data == again.data == empty.data == every.data


def _metric(c, name):
    for ln in c.get("/metrics").data.decode().splitlines():
        if ln.startswith(name + " "):
            return float(ln.split()[1])
    raise AssertionError("no metric " + name)


def test_delete_route_then_404(client):
    c, svc = client
    deleted0, compact0 = _metric(c, "rag_index_chunks_deleted_total"), _metric(c, "rag_index_compactions_total")
    assert _upload(c, "x.pdf", _pdf("x", 1700)).status_code == 200
    assert _doc_chunks(svc)["x.pdf"] == 3
    r = c.delete("/documents/x.pdf")
    assert r.status_code == 200 and r.get_json() == {"message": "Document deleted. 3 chunks removed.",
                                                     "chunks_removed": 3}
    assert "x.pdf" not in _doc_chunks(svc)
    r = c.delete("/documents/x.pdf")
    assert r.status_code == 404 and set(r.get_json()) == {"error"}
    assert _metric(c, "rag_index_chunks_deleted_total") == deleted0 + 3
    svc.store.flush()
    assert _metric(c, "rag_index_compactions_total") == compact0 + 1
    assert _metric(c, "rag_index_tombstoned_chunks") == 0
    assert c.get("/index_info").get_json()["total_chunks"] == sum(_doc_chunks(svc).values())


def test_upload_replace_and_dedupe(client):
    c, svc = client
    r = _upload(c, "rev.pdf", _pdf("old", 1700))
    assert r.get_json() == {"message": "PDF processed and indexed successfully. 3 chunks created."}
    assert _doc_chunks(svc)["rev.pdf"] == 3
    # without replace: today's dedupe -- chunk ids 0..2 exist, only the new id 3 is added, old text stays
    r = _upload(c, "rev.pdf", _pdf("new", 2600))
    assert r.status_code == 200 and _doc_chunks(svc)["rev.pdf"] == 4
    texts = [m["text"] for m in svc.store.metadata if m["filename"] == "rev.pdf"]
    assert sum(t.startswith("old") for t in texts) == 3
    # with replace: exactly the new chunks
    r = _upload(c, "rev.pdf", _pdf("new", 2600), replace=True)
    assert r.get_json() == {"message": "PDF processed and indexed successfully. 4 chunks created."}
    res = svc.store.search(np.zeros((1, svc.store.dim), np.float32), 64, filters=[["rev.pdf"]])[0]
    assert len(res) == 4 and all(m["text"].startswith("new") for m, _ in res)
    assert sorted(m["chunk_id"] for m, _ in res) == sorted(
        m["chunk_id"] for m in svc.store.metadata[-4:]) and _doc_chunks(svc)["rev.pdf"] == 4
    r = c.post("/upload_pdf", data={"file": (io.BytesIO(_pdf("third", 600)), "rev.pdf"), "replace": "1"},
               content_type="multipart/form-data")  # the form-field spelling
    assert r.status_code == 200 and _doc_chunks(svc)["rev.pdf"] == 1


def test_concurrent_search_during_replace_sees_exactly_one_version(client):
    c, svc = client
    assert _upload(c, "live.pdf", _pdf("va", 1700), replace=True).status_code == 200
    stop, bad, seen = threading.Event(), [], set()
    q = np.zeros((1, svc.store.dim), np.float32)

    def reader():
        while not stop.is_set():
            tags = {m["text"][:2] for m, _ in svc.store.search(q, 64, filters=[["live.pdf"]])[0]}
            seen.update(tags)
            if len(tags) != 1:
                bad.append(tags)

    t = threading.Thread(target=reader)
    t.start()
    try:
        for i in range(6):
            assert _upload(c, "live.pdf", _pdf("vb" if i % 2 == 0 else "va", 1700), replace=True).status_code == 200
    finally:
        stop.set()
        t.join()
    assert not bad, bad  # never zero chunks of the document, never old and new together
    assert seen <= {"va", "vb"} and _doc_chunks(svc)["live.pdf"] == 3


def test_sharded_service_refuses_delete_and_filters(client):
    c, svc = client
    svc.store.sharded = True
    try:
        r = c.delete("/documents/doc_00000.pdf")
        assert r.status_code == 501 and "INDEX_SHARDED" in r.get_json()["error"]
        r = c.post("/generate", json={"prompt": "x", "filenames": ["doc_00000.pdf"]})
        assert r.status_code == 500 and "INDEX_SHARDED" in r.get_json()["error"]
        r = _upload(c, "doc_00000.pdf", _pdf("s", 100), replace=True)
        assert r.status_code == 501 and "INDEX_SHARDED" in r.get_json()["error"]
    finally:
        svc.store.sharded = False
    assert "doc_00000.pdf" in _doc_chunks(svc)


# ------------------------------------------------------------------------------------------ oracle-side condition
@pytest.mark.parametrize("density", C.DENSITIES)
@pytest.mark.parametrize("N,d,nq,k", C.FLAT_CASES)
def test_random_mask_cases_fp32_is_within_two_swaps_of_fp64(N, d, nq, k, density):
    """The GPU random-mask cases allow at most 2 rank swaps of near-equal distances against the fp64 masked
    oracle (the rule of test_l2_search). Same seeds and shapes: an fp32 torch masked search already stays
    within that rule, so the allowance cannot hide a kernel fault."""
    xb, q = C.data(N, d, nq)
    allowed, masks, qmask = C.random_masks(N, nq, density)
    assert np.array_equal(mask_allowed(masks, qmask, np.arange(N)), allowed)
    D = torch.full((nq, k), FLT_MAX)
    I = torch.full((nq, k), -1, dtype=torch.int64)
    for j in range(nq):  # fp32 direct form, one query at a time
        dist = ((xb - q[j][None]) ** 2).sum(1)
        dist[~torch.from_numpy(allowed[j])] = float("inf")
        dv, di = torch.sort(dist, stable=True)
        n = min(k, int(allowed[j].sum()))
        D[j, :n], I[j, :n] = dv[:n], di[:n]
    C.assert_within_two_swaps(D, I, *C.random_mask_oracle(N, d, nq, k, density))
    C.assert_padding(D, I, allowed.sum(1))
