"""Shared cases of the filtered-search tests (tests/test_index_filter_cpu.py, tests/test_index_filter_gpu.py):
the shapes that reach every masked kernel path, the seeded random masks, the fp64 masked oracle and the
document-store scenario that runs on the CPU and on the GPU."""
import functools

import numpy as np
import torch

from rag_llm_k8s_amd.index.flat import pack_masks
from rag_llm_k8s_amd.ops import reference as R

FLT_MAX = torch.finfo(torch.float32).max

# (N, d, nq, k): one per kernel path of the flat search
FLAT_CASES = [
    (777, 96, 5, 10),       # l2_scan S=4
    (70000, 128, 9, 8),     # l2_scan S=2
    (300000, 32, 3, 64),    # l2_scan S=1
    (129, 384, 1, 5),       # l2_scan, single query
    (777, 96, 70, 3),       # l2_mfma RT=1, QT=2, partial query group
    (5000, 1024, 16, 7),    # l2_mfma RT=1, QT=1
    (300000, 64, 33, 5),    # l2_mfma RT=4
]
DENSITIES = [0.5, 0.01]
IVF_CASE = (3000, 64, 16)   # N, d, nlist; nprobe 16 and 4


@functools.lru_cache(maxsize=None)
def data(N, d, nq, seed=15):
    torch.manual_seed(seed)
    return torch.randn(N, d), torch.randn(nq, d)


@functools.lru_cache(maxsize=None)
def random_masks(N, nq, density, seed=77):
    """(allowed bool [nq, N] -- what each query may return --, masks uint32 [nq, words], qmask int32 [nq]):
    one bitmap row per query, every third query unfiltered (qmask -1: its row is ignored)."""
    g = np.random.default_rng(seed + int(density * 1000) + N)
    rows = g.random((nq, N)) < density
    qmask = np.arange(nq, dtype=np.int32)
    qmask[2::3] = -1
    allowed = rows.copy()
    allowed[qmask < 0] = True
    return allowed, pack_masks(rows), qmask


def masked_oracle(xb, q, k, allowed, ids=None):
    """fp64 exact top-k (ops/reference.l2_knn) of every query over the rows it may return, mapped back to
    ids; (-1, FLT_MAX) padding."""
    D = torch.full((q.shape[0], k), FLT_MAX)
    I = torch.full((q.shape[0], k), -1, dtype=torch.int64)
    for j in range(q.shape[0]):
        rows = torch.from_numpy(np.nonzero(allowed[j])[0])
        if not len(rows):
            continue
        dj, ij = R.l2_knn(xb[rows], q[j:j + 1], k)
        D[j] = dj[0]
        m = ij[0] >= 0
        I[j, m] = rows[ij[0][m]] if ids is None else ids[rows[ij[0][m]]]
    return D, I


@functools.lru_cache(maxsize=None)
def random_mask_oracle(N, d, nq, k, density):
    xb, q = data(N, d, nq)
    return masked_oracle(xb, q, k, random_masks(N, nq, density)[0])


def assert_within_two_swaps(D, I, Dr, Ir):
    """The rule of test_l2_search: distances within rtol 1e-4 / atol 1e-3 of the fp64 reference, at most 2 id
    mismatches, each a swap of distances closer than 1e-3."""
    D, I = D.cpu(), I.cpu()
    bad = I != Ir
    print("id mismatches: %d, max |D - Dref| over finite: %.3g" % (
        int(bad.sum()), float((D - Dr)[Dr < FLT_MAX].abs().max()) if bool((Dr < FLT_MAX).any()) else 0.0))
    assert bad.sum() <= 2
    if bad.any():
        assert (Dr[bad] - D[bad]).abs().max().item() < 1e-3
    assert torch.allclose(D, Dr, rtol=1e-4, atol=1e-3)


def assert_padding(D, I, n_allowed):
    """Rows past the allowed count are exactly (-1, FLT_MAX); no id >= 0 is paired with FLT_MAX."""
    D, I = D.cpu(), I.cpu()
    k = D.shape[1]
    for j, n in enumerate(n_allowed):
        n = min(int(n), k)
        assert bool((I[j, :n] >= 0).all()) and bool((D[j, :n] < FLT_MAX).all())
        assert bool((I[j, n:] == -1).all()) and bool((D[j, n:] == FLT_MAX).all())
    assert not bool(((I >= 0) & (D == FLT_MAX)).any())


# ---------------------------------------------------------------------------------------------
# document store scenario (flat and IVF, cpu and cuda)
DOCS = [("a.pdf", 7), ("b.pdf", 12), ("c.pdf", 5)]
DIM = 64


def doc_vectors(seed=5):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for fn, n in DOCS:
        out[fn] = (torch.randn(n, DIM, generator=g).numpy(),
                   [{"filename": fn, "chunk_id": i, "text": "%s chunk %d" % (fn, i)} for i in range(n)])
    return out


def _keys(res):
    return [(m["filename"], m["chunk_id"]) for m, _ in res]


def _brute(vecs, metas, q, k, allowed_files):
    rows = [i for i, m in enumerate(metas) if allowed_files is None or m["filename"] in allowed_files]
    if not rows:
        return []
    d = ((vecs[rows].astype(np.float64) - q.astype(np.float64)[None]) ** 2).sum(1)
    order = np.argsort(d, kind="stable")[:k]
    return [(metas[rows[i]]["filename"], metas[rows[i]]["chunk_id"]) for i in order]


def _same(a, b):
    assert _keys(a) == _keys(b)
    assert np.allclose([d for _, d in a], [d for _, d in b], rtol=1e-5, atol=1e-5)


def store_scenario(tmp_path, device, index_type):
    from rag_llm_k8s_amd.index.faiss_io import load_metadata, read_index
    from rag_llm_k8s_amd.index.store import DocumentStore

    def new_store():
        return DocumentStore(str(tmp_path / "faiss_index"), DIM, device=device, index_type=index_type, ivf_nlist=4,
                             ivf_nprobe=4)

    docs = doc_vectors()
    store = new_store().ensure_exists()
    for fn, _ in DOCS:
        assert store.add(*docs[fn]) == len(docs[fn][1])
    vecs = np.concatenate([docs[fn][0] for fn, _ in DOCS])
    metas = [m for fn, _ in DOCS for m in docs[fn][1]]
    assert store.documents() == [{"filename": fn, "chunks": n} for fn, n in DOCS]
    g = np.random.default_rng(3)
    q = (vecs[[0, 8, 20, 3, 15, 23]] + 0.3 * g.standard_normal((6, DIM))).astype(np.float32)
    k = 5

    # one filter for every query: only the allowed document's chunks, and the right ones
    res = store.search(q, k, filters=[["b.pdf"]] * 6)
    for j, r in enumerate(res):
        assert _keys(r) == _brute(vecs, metas, q[j], k, {"b.pdf"})
    # mixed filters in one call (None included) == each query on its own
    filters = [None, ["a.pdf"], ["b.pdf", "c.pdf"], None, ("c.pdf",), ["nope.pdf"]]
    res = store.search(q, k, filters=filters)
    for j, f in enumerate(filters):
        _same(res[j], store.search(q[j:j + 1], k, filters=[f])[0])
        assert _keys(res[j]) == _brute(vecs, metas, q[j], k, None if f is None else set(f))
    assert res[5] == []  # a filter naming no known document: no results, not an error
    assert len(store.search(q[:1], 10, filters=[["a.pdf"]])[0]) == 7  # fewer allowed rows than k
    _same(store.search(q, k)[0], store.search(q, k, filters=[None] * 6)[0])

    # delete: gone for the very next search, before any snapshot (the snapshot thread needs the lock)
    with store._wlock:
        assert store.delete("b.pdf") == 12
        assert store._dead == 12 and store.index.ntotal == 24  # tombstoned, not yet compacted
        res = store.search(q, k)
        assert all(fn != "b.pdf" for r in res for fn, _ in _keys(r))
        for j in range(6):
            assert _keys(res[j]) == _brute(vecs, metas, q[j], k, {"a.pdf", "c.pdf"})
        assert store.search(q[:1], k, filters=[["b.pdf"]])[0] == []
        assert store.documents() == [{"filename": "a.pdf", "chunks": 7}, {"filename": "c.pdf", "chunks": 5}]
        info = store.info()
        assert info["total_chunks"] == info["total_vectors"] == 12
        assert all(m["filename"] != "b.pdf" for m in info["sample_chunks"]) and len(info["sample_chunks"]) == 5
    assert store.delete("b.pdf") == 0 and store.delete("nope.pdf") == 0
    before = store.search(q, k)
    store.flush()
    assert store._dead == 0 and store.index.ntotal == 12 and len(store.metadata) == 12
    for a, b in zip(before, store.search(q, k)):  # compaction renumbers ids, results stay
        _same(a, b)

    # the files hold exactly the live vectors and metadata, in original order, in the plain formats
    live = [i for i, m in enumerate(metas) if m["filename"] != "b.pdf"]
    r = read_index(store.index_file)
    assert r["ntotal"] == 12
    if r["type"] == "flat":
        assert np.array_equal(r["xb"], vecs[live])
    else:
        ids = np.concatenate([np.asarray(i) for i in r["ids"]])
        xs = np.concatenate([np.asarray(x, np.float32).reshape(-1, DIM) for x in r["lists"]])
        assert sorted(ids.tolist()) == list(range(12))
        assert np.array_equal(xs[np.argsort(ids)], vecs[live])
    assert load_metadata(store.meta_path) == [metas[i] for i in live]
    fresh = new_store()
    fresh.load()
    for f in (None, [["c.pdf"]] * 6):
        for a, b in zip(store.search(q, k, filters=f), fresh.search(q, k, filters=f)):
            _same(a, b)

    # the deleted document's keys were dropped: it can be uploaded again
    assert store.add(*docs["b.pdf"]) == 12
    assert store.add(*docs["b.pdf"]) == 0  # and dedupes as before
    assert store.documents() == [{"filename": "a.pdf", "chunks": 7}, {"filename": "c.pdf", "chunks": 5},
                                 {"filename": "b.pdf", "chunks": 12}]
    assert _keys(store.search(q[1:2], k, filters=[["b.pdf"]])[0]) == _brute(vecs, metas, q[1], k, {"b.pdf"})
    # replace: old chunks out and new ones in under one lock
    nv = torch.randn(3, DIM, generator=torch.Generator().manual_seed(9)).numpy()
    nm = [{"filename": "a.pdf", "chunk_id": i, "text": "revised %d" % i} for i in range(3)]
    assert store.add(nv, nm, replace=True) == 3
    assert {d["filename"]: d["chunks"] for d in store.documents()} == {"a.pdf": 3, "c.pdf": 5, "b.pdf": 12}
    got = store.search(nv[:1], 10, filters=[["a.pdf"]])[0]
    assert [m["text"] for m, _ in got] == ["revised 0"] + [m["text"] for m, _ in got[1:]] and len(got) == 3
    assert all(m["text"].startswith("revised") for m, _ in got)
    store.flush()
    assert store.info()["total_chunks"] == 20 and len(load_metadata(store.meta_path)) == 20
