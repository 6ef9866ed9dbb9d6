"""BM25 lexical search on the GPU: ragk_lex_df / ragk_lex_search against the fp32 replica of ops/reference.py
(torch.equal for df, ids and scores, inputs and outputs inside sentinel frames, poisoned CSR tails), the
launcher's refusals, the LexicalIndex on the device against the CPU one, and the hybrid store / service
scenarios on the GPU backend against the CPU backend."""
import numpy as np
import pytest
import torch

import lexical_cases as C
from rag_llm_k8s_amd.ops import reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
KCASES = C.kernel_cases()


def _framed(x, poison):
    """x inside a buffer with PAD poisoned elements on both sides -> (buffer, view) on the device."""
    buf = torch.full((x.numel() + 2 * PAD,), poison, dtype=x.dtype)
    buf[PAD:PAD + x.numel()] = x.reshape(-1)
    buf = buf.to(DEV)
    return buf, buf[PAD:PAD + x.numel()].view(x.shape)


def _intact(buf, poison):
    return bool((buf[:PAD] == poison).all()) and bool((buf[-PAD:] == poison).all())


def _device_case(case):
    """The case's CSR on the device in buffers LARGER than the index: poisoned tail rows after row n (row
    pointers far outside the entry arrays) and poisoned entries after the last one (a table term with a huge tf),
    so a kernel that reads past n or past row_ptr[n] changes its result or faults a sentinel check."""
    t = case.tensors()
    n, nnz = case.n, int(t["row_ptr"][case.n])
    rp = torch.full((n + 1 + 8,), 1 << 40, dtype=torch.int64)
    rp[:n + 1] = t["row_ptr"]
    first = int(t["qterms"][0]) if t["qterms"].numel() else 7
    te = torch.full((nnz + 16,), first, dtype=torch.int32)
    te[:nnz] = t["terms"]
    tf = torch.full((nnz + 16,), -1, dtype=torch.int16)  # 65535
    tf[:nnz] = t["tf"]
    dl = torch.full((n + 8,), 1, dtype=torch.int32)
    dl[:n] = t["doc_len"]
    d = dict(t)
    d.update(row_ptr=rp.to(DEV), terms=te.to(DEV), tf=tf.to(DEV), doc_len=dl.to(DEV))
    for k in ("live", "masks"):
        if t[k] is not None:
            d[k] = t[k].to(DEV)
    return t, d


def _run(case):
    from rag_llm_k8s_amd.ops import native

    t, d = _device_case(case)
    T, nq, k, n = t["qterms"].numel(), len(case.queries), case.k, case.n
    want_df = R.lex_df(t["row_ptr"], t["terms"], n, t["qterms"], live=t["live"])
    dbuf, dview = _framed(torch.full((T,), -5, dtype=torch.int32), -777)
    got_df = native.lex_df(d["row_ptr"], d["terms"], n, t["qterms"], live=d["live"], out=dview)
    assert _intact(dbuf, -777)
    idf, avgdl = case.host_numbers(want_df.numpy())
    args = (n, t["qterms"], idf, t["member"], nq, C.K1, float(np.float32(C.K1) + np.float32(1)), C.B, avgdl, k)
    want = R.lex_search(t["row_ptr"], t["terms"], t["tf"], t["doc_len"], *args, masks=t["masks"], qmask=t["qmask"])
    sbuf, sview = _framed(torch.full((nq, k), float("nan")), -7.5)
    ibuf, iview = _framed(torch.full((nq, k), -99, dtype=torch.int64), -777)
    got = native.lex_search(d["row_ptr"], d["terms"], d["tf"], d["doc_len"], *args, masks=d["masks"],
                            qmask=t["qmask"], out=(sview, iview))
    torch.cuda.synchronize()
    assert _intact(sbuf, -7.5) and _intact(ibuf, -777)
    return want_df, got_df.cpu(), want, (got[0].cpu(), got[1].cpu()), (d, t, args)


@pytest.mark.parametrize("case", KCASES, ids=repr)
def test_kernels_equal_the_replica(case):
    want_df, got_df, want, got, _ = _run(case)
    assert torch.equal(got_df, want_df)
    assert torch.equal(got[1], want[1]), "ids"
    assert torch.equal(got[0], want[0]), "scores"
    assert (want[1] >= 0).any() or all(len(q) == 0 for q in case.queries)


def test_two_launches_are_bit_identical():
    from rag_llm_k8s_amd.ops import native

    case = C.t_sweep()[-1]
    _, _, _, got, (d, t, args) = _run(case)
    again = native.lex_search(d["row_ptr"], d["terms"], d["tf"], d["doc_len"], *args)
    assert torch.equal(again[0].cpu(), got[0]) and torch.equal(again[1].cpu(), got[1])


def test_launcher_refusals():
    from rag_llm_k8s_amd.ops import native

    case = C.n_sweep()[2]
    t, d = _device_case(case)
    csr = (d["row_ptr"], d["terms"], d["tf"], d["doc_len"], case.n)
    ok = torch.arange(5, dtype=torch.int32)

    def search(qt, nq=1, k=5):
        T = qt.numel()
        return native.lex_search(*csr, qt, torch.ones(T), torch.ones(T, dtype=torch.int64), nq, 1.2, 2.2, 0.75, 3.0, k)

    search(ok)
    with pytest.raises(ValueError, match="4096"):
        search(torch.arange(4097, dtype=torch.int32))
    with pytest.raises(ValueError, match="4096"):
        native.lex_df(d["row_ptr"], d["terms"], case.n, torch.arange(4097, dtype=torch.int32))
    with pytest.raises(ValueError, match="k <= 64"):
        search(ok, k=65)
    with pytest.raises(ValueError, match="k <= 64"):
        search(ok, k=0)
    with pytest.raises(ValueError, match="ascending"):
        search(torch.tensor([3, 2, 9], dtype=torch.int32))
    with pytest.raises(ValueError, match="ascending"):
        search(torch.tensor([3, 3], dtype=torch.int32))
    with pytest.raises(ValueError, match="ascending"):  # unsigned order: 0x80000000 sorts after 5
        search(torch.tensor([-2 ** 31, 5], dtype=torch.int32))
    with pytest.raises(ValueError, match="ascending"):
        native.lex_df(d["row_ptr"], d["terms"], case.n, torch.tensor([9, 2], dtype=torch.int32).to(DEV))
    with pytest.raises(ValueError, match="64 queries"):
        search(ok, nq=65)


KEYS = ("dense_rank", "lexical_rank", "lexical_score")
TEXTS = ["alpha beta gamma id%04dx %s" % (i, " ".join("w%d" % ((i * 7 + j) % 23) for j in range(i % 11)))
         for i in range(150)]


def _same_state(a, b):
    sa, sb = a.state(), b.state()
    return all(torch.equal(sa[k], sb[k]) for k in sa)


def test_index_on_the_device_equals_the_cpu_index():
    from rag_llm_k8s_amd.index.lexical import LexicalIndex

    cpu, gpu = LexicalIndex("cpu", capacity=4, entry_capacity=8), LexicalIndex(DEV, capacity=4, entry_capacity=8)
    for idx in (cpu, gpu):
        idx.add(TEXTS[:3])
        idx.add(TEXTS[3:90])
        idx.add(TEXTS[90:])
    assert _same_state(cpu, gpu) and gpu._terms.is_cuda
    keep = np.asarray([i for i in range(150) if i % 3 != 1])
    for idx in (cpu, gpu):
        idx.compact(keep)
    assert _same_state(cpu, gpu)
    fresh = LexicalIndex(DEV)
    fresh.add([TEXTS[i] for i in keep])
    assert _same_state(fresh, gpu)
    # 65 queries: the wrapper cuts them into two launches; the same numbers on both backends
    queries = ["id%04dx beta w%d" % (keep[i], i % 23) for i in range(65)]
    sc, ic = cpu.search(queries, 5)
    sg, ig = gpu.search(queries, 5)
    assert torch.equal(ic, ig) and torch.equal(sc, sg)
    assert ic[:, 0].tolist() == list(range(65))  # the chunk that holds the query's unique token wins


def _store(device, tmp_path, name, index_type="flat"):
    from rag_llm_k8s_amd.index.store import DocumentStore

    rng = np.random.default_rng(5)
    vecs = rng.standard_normal((150, 32)).astype(np.float32)
    st = DocumentStore(str(tmp_path / name), 32, device=device, index_type=index_type, ivf_nlist=4, ivf_nprobe=4,
                       lexical=True, hybrid_candidates=16)
    st.add(vecs, [{"filename": "f%d.pdf" % (i % 5), "chunk_id": i // 5, "text": t} for i, t in enumerate(TEXTS)],
           persist=False)
    return st, vecs


@pytest.mark.parametrize("index_type", ["flat", "ivf"])
def test_store_scenario_gpu_equals_cpu(tmp_path, index_type):
    cpu, vecs = _store("cpu", tmp_path, "cpu", index_type)
    gpu, _ = _store(DEV, tmp_path, "gpu", index_type)
    q = vecs[[3, 40, 77, 120]] + 0.01
    texts = ["id0140x gamma", None, "id0003x w5 w6", "nothing matches this"]
    filters = [None, None, ("f0.pdf", "f3.pdf"), None]

    def check():
        for flt in (None, filters):
            rc = cpu.search(q, 8, filters=flt, texts=texts)
            rg = gpu.search(q, 8, filters=flt, texts=texts)
            for j, (a, b) in enumerate(zip(rc, rg)):
                assert [(m["filename"], m["chunk_id"]) for m, _ in a] == [(m["filename"], m["chunk_id"]) for m, _ in b]
                assert [[m.get(k) for k in KEYS] for m, _ in a] == [[m.get(k) for k in KEYS] for m, _ in b]
                for (m, da), (_, db) in zip(a, b):
                    if texts[j] is not None and m["dense_rank"] is None:
                        # a lexical-only chunk: index.distances(), an fp32 sum of 32 squares of the stored row
                        ref = float(((vecs[TEXTS.index(m["text"])].astype(np.float64) - q[j]) ** 2).sum())
                        assert abs(da - ref) <= 34 * 2.0 ** -24 * ref and abs(db - ref) <= 34 * 2.0 ** -24 * ref
                    else:  # the searches' own distances (their forms differ between the backends)
                        assert da == pytest.approx(db, rel=1e-3, abs=1e-3)
        return rc

    rc = check()
    assert any(m["text"].startswith("alpha beta gamma id0140x") and m["dense_rank"] is None for m, _ in rc[0])
    for st in (cpu, gpu):
        st.delete("f0.pdf", persist=False)  # tombstones: masked in the very next search, df / avgdl follow
    rc = check()
    assert all(m["filename"] != "f0.pdf" for r in rc for m, _ in r)
    for st in (cpu, gpu):
        st.persist()  # compaction at the snapshot
    assert gpu.lexical.ntotal == gpu.index.ntotal == 120
    check()


def test_tiny_rag_workload_hybrid_chunk_order_gpu_equals_cpu(tmp_path):
    """The tiny workload with hybrid="rrf": the GPU store's fused chunk order is the order of a CPU store holding
    the same vectors and texts, for the same query vectors (the embedders differ between the devices: bf16
    kernels against fp32 torch; what is compared is the retrieval)."""
    import re

    from rag_llm_k8s_amd.engine.llm_engine import SamplingParams
    from rag_llm_k8s_amd.index.store import DocumentStore
    from rag_llm_k8s_amd.utils.workload import build_workload, make_queries

    DEPTH = 4
    wl = build_workload(model="tiny", embedder="tiny", n_chunks=64, chunk_words=120, retrieve_k=3, context_k=3,
                        max_new_tokens=2, max_batch=4, max_model_len=2048, max_prefill_tokens=4096, device=DEV,
                        word_vocab=20000, hybrid="rrf", hybrid_candidates=DEPTH, rerank_candidates=DEPTH)
    svc = wl.svc
    assert svc.store.lexical is not None and svc.store.lexical.ntotal == 64 and svc.cfg.hybrid
    meta = list(svc.store.metadata)
    twin = DocumentStore(str(tmp_path / "cpu_index"), svc.store.dim, device="cpu", lexical=True,
                         hybrid_candidates=DEPTH)
    twin.add(svc.store.index.reconstruct_all(), meta, dedupe=False, persist=False)
    # Queries: a pool of random ones, each with two words of one chunk appended (so the lexical list has a clear
    # winner), and of those the 3 whose DEPTH + 1 nearest dense distances lie farthest apart on the CPU: both
    # backends sum d = 128 fp32 products of unit vectors, |error| <= 4 (d + 2) 2^-24 in the ||x||^2 + ||q||^2 -
    # 2 x.q form, so ranks across gaps wider than twice that cannot depend on the device.
    pool = make_queries(wl.wm, 48, seed=3, words=6)
    pool = [p + " " + " ".join(meta[(7 * i) % 64]["text"].split()[5:7]) for i, p in enumerate(pool)]
    qv = svc.embedder.embed(pool).cpu()
    D, _ = twin.index.search(qv, DEPTH + 1)
    margin = (D[:, 1:] - D[:, :-1]).min(1).values
    best = torch.argsort(margin, descending=True)[:3].tolist()
    assert float(margin[best[-1]]) > 2 * 4 * 130 * 2.0 ** -24, margin.sort().values[-3:]
    qs, q = [pool[i] for i in best], qv[best]
    ids = lambda res: [[(m["filename"], m["chunk_id"], m["dense_rank"], m["lexical_rank"]) for m, _ in r] for r in res]  # noqa: E731
    want = ids(twin.search(q, 3, texts=qs))
    assert ids(svc.store.search(q, 3, texts=qs)) == want
    assert any(r[2] is None for w in want for r in w), "no lexical-only chunk: the comparison would be vacuous"
    outs = svc.generate_batch(qs, params=SamplingParams(max_new_tokens=2, ignore_eos=True), seeds=[1, 2, 3])
    for o, w in zip(outs, want):
        got = re.findall(r"Document '([^']+)' \(chunk (\d+), score:", o["context"])
        assert [(f, int(c)) for f, c in got] == [(f, c) for f, c, _, _ in w]
    plain = svc.generate_batch(qs, params=SamplingParams(max_new_tokens=2, ignore_eos=True), seeds=[1, 2, 3],
                               hybrid=False)
    dense = svc.store.search(q, 3)
    for o, r in zip(plain, dense):
        got = re.findall(r"Document '([^']+)' \(chunk (\d+), score:", o["context"])
        assert [(f, int(c)) for f, c in got] == [(m["filename"], m["chunk_id"]) for m, _ in r]
