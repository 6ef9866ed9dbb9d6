"""Cross-encoder reranking on the GPU: the typed embed_ln, cls_head (tile tails, scattered CLS rows, NaN-poisoned
neighbours, column indexing, canaries, shape refusal) and rerank_select kernels against their oracles, the
packed cross-encoder against fp32 transformers, and the tiny RAG workload with a reranker attached."""
import functools

import numpy as np
import pytest
import torch

import rerank_cases as C
from rag_llm_k8s_amd.ops import reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ------------------------------------------------------------------------------------------ typed embed_ln
@pytest.mark.parametrize("H", [64, 384, 1024])
def test_embed_ln_typed(native, H):
    torch.manual_seed(7)
    V, P, T = 50, 16, 5
    word, pos, table = (torch.randn(n, H, device=DEV).bfloat16() for n in (V, P, 2))
    g, b = torch.randn(H, device=DEV).bfloat16(), torch.randn(H, device=DEV).bfloat16()
    ids = torch.randint(0, V, (T,), device=DEV, dtype=torch.int32)
    pids = torch.randint(0, P, (T,), device=DEV, dtype=torch.int32)
    types = torch.tensor([0, 1, 1, 0, 1], device=DEV, dtype=torch.int32)
    y = native.embed_ln_tt(ids, pids, types, word, pos, table, g, b, 1e-12)
    h = word[ids.long()].float() + pos[pids.long()].float() + table[types.long()].float()
    ref = torch.nn.functional.layer_norm(h, (H,), g.float(), b.float(), 1e-12)
    assert y.shape == (T, H) and y.dtype == torch.bfloat16
    assert rel_err(y, ref) < 1e-2  # the tolerance of test_embed_ln
    oracle = R.embed_ln_tt(ids.cpu(), pids.cpu(), types.cpu(), word.cpu(), pos.cpu(), table.cpu(), g.cpu(), b.cpu(), 1e-12)
    assert rel_err(y.cpu(), oracle) < 1e-2
    # all-zero type ids: bit-identical to the existing kernel with type_row = table[0]
    y0 = native.embed_ln_tt(ids, pids, torch.zeros_like(types), word, pos, table, g, b, 1e-12)
    assert torch.equal(y0, native.embed_ln(ids, pids, word, pos, table[0].contiguous(), g, b, 1e-12))
    assert not torch.equal(y0, y)


# ------------------------------------------------------------------------------------------ cls_head
HEAD_B = (1, 15, 16, 17, 33)
HEAD_H = (384, 1024)


@functools.lru_cache(maxsize=None)
def _head_case(B, H):
    """Host tensors of one case: ragged cu (CLS rows scattered), every other row of h NaN, and the float64
    scores of the bf16-rounded operands. Computed once and shared."""
    g = torch.Generator().manual_seed(100 * B + H)
    lens = torch.randint(1, 8, (B,), generator=g)
    cu = torch.zeros(B + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    T = int(cu[-1])
    h = torch.full((T, H), float("nan")).bfloat16()
    x = torch.randn(B, H, generator=g).bfloat16()
    h[cu[:-1].long()] = x
    w1 = (torch.randn(H, H, generator=g) / H ** 0.5).bfloat16()
    b1 = (0.5 * torch.randn(H, generator=g)).bfloat16()
    w2 = (torch.randn(H, generator=g) / H ** 0.5).bfloat16()
    b2 = 0.375
    ref = R.cls_head(h, cu, w1, b1, w2, b2, dtype=torch.float64)
    e32 = float((R.cls_head(h, cu, w1, b1, w2, b2, dtype=torch.float32).double() - ref).abs().max())
    assert torch.isfinite(ref).all()
    return h, cu, x, w1, b1, w2, b2, ref, e32


def _head_bound():
    """8x the largest error of the same head in fp32 torch on the CPU vs float64 over these shapes (room for the
    other accumulation order and the device tanh)."""
    return 8 * max(_head_case(B, H)[8] for B in HEAD_B for H in HEAD_H)


@pytest.mark.parametrize("H", HEAD_H)
@pytest.mark.parametrize("B", HEAD_B)
def test_cls_head(native, B, H):
    h, cu, x, w1, b1, w2, b2, ref, e32 = _head_case(B, H)
    CAN = 7
    out = torch.full((B + CAN,), -777.0, device=DEV)  # sentinel slots past B
    got = native.cls_head(h.to(DEV), cu.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert (out[B:] == -777.0).all(), "cls_head wrote past B"
    s = out[:B].cpu().double()
    assert torch.isfinite(s).all(), "a score read a row that is not its sequence's first"
    bound = _head_bound()
    err = float((s - ref).abs().max())
    assert err <= bound, "cls_head B=%d H=%d: max error %.3e vs float64; fp32 torch on the CPU: %.3e (this case), " \
                         "bound 8 x max over the shapes = %.3e" % (B, H, err, e32, bound)
    fresh = native.cls_head(h.to(DEV), cu.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2)
    assert fresh.shape == (B,) and fresh.dtype == torch.float32 and torch.equal(fresh, out[:B])


@pytest.mark.parametrize("H", HEAD_H)
def test_cls_head_column_indexing(native, H):
    """w2 one-hot at column j: score[b] = tanh(W1[j] . x_b + b1[j]) + b2, element by element against float64."""
    B = 17
    h, cu, x, w1, b1, _, b2, _, _ = _head_case(B, H)
    hd, cud, w1d, b1d = h.to(DEV), cu.to(DEV), w1.to(DEV), b1.to(DEV)
    bound = _head_bound()
    for j in (0, 15, 16, 63, 64, H - 1):
        w2 = torch.zeros(H).bfloat16()
        w2[j] = 1.0
        got = native.cls_head(hd, cud, w1d, b1d, w2.to(DEV), b2).cpu().double()
        ref = torch.tanh(x.double() @ w1[j].double() + b1[j].double()) + b2
        err = float((got - ref).abs().max())
        assert err <= bound, "column %d: max error %.3e, bound %.3e" % (j, err, bound)


def test_cls_head_refuses_other_shapes(native):
    def run(H, T=4, **kw):
        a = dict(h=torch.zeros(T, H, device=DEV).bfloat16(), cu=torch.tensor([0, 2, 4], dtype=torch.int32, device=DEV),
                 w1=torch.zeros(H, H, device=DEV).bfloat16(), b1=torch.zeros(H, device=DEV).bfloat16(),
                 w2=torch.zeros(H, device=DEV).bfloat16(), b2=0.0)
        a.update(kw)
        return native.cls_head(**a)

    with pytest.raises(ValueError, match="multiple of 64"):
        run(96)
    with pytest.raises(ValueError, match="multiple of 64"):
        run(1088)
    with pytest.raises(ValueError):
        run(128, cu=torch.tensor([0, 2, 4], device=DEV))  # int64 cu
    with pytest.raises(ValueError):
        run(128, w1=torch.zeros(128, 64, device=DEV).bfloat16())
    with pytest.raises(ValueError):
        run(128, h=torch.zeros(4, 256, device=DEV).bfloat16()[:, 4:132])  # a view whose rows start 8 bytes off
    assert run(128).tolist() == [0.0, 0.0]  # the smallest served shape still runs


# ------------------------------------------------------------------------------------------ rerank_select
@pytest.mark.parametrize("Q,N,k", C.SELECT_SHAPES)
def test_rerank_select(native, Q, N, k):
    s, ids, dist, nv = C.select_case(Q, N)
    want = R.rerank_select(s, ids, dist, nv, k)
    CAN = 5
    out = (torch.full((Q * k + CAN,), -7, dtype=torch.int64, device=DEV),
           torch.full((Q * k + CAN,), -7.0, device=DEV), torch.full((Q * k + CAN,), -7.0, device=DEV))
    native.rerank_select(s.to(DEV), ids.to(DEV), dist.to(DEV), nv.to(DEV), k, out=out)
    torch.cuda.synchronize()
    for o, w in zip(out, want):
        assert (o[Q * k:] == -7).all(), "rerank_select wrote past [Q, k]"
        assert C.bits_equal(o[:Q * k].cpu().view(Q, k), w)
    fresh = native.rerank_select(s.to(DEV), ids.to(DEV), dist.to(DEV), nv.to(DEV), k)
    for o, w in zip(fresh, want):
        assert o.shape == (Q, k) and C.bits_equal(o.cpu(), w)


def test_rerank_select_many_queries_and_refusals(native):
    """More queries than one workgroup holds (4 waves), and the shape checks before launch."""
    Q, N, k = 11, 32, 5
    g = torch.Generator().manual_seed(2)
    s = torch.randint(-4, 5, (Q, N), generator=g).float()
    ids = torch.randint(0, 2 ** 40, (Q, N), generator=g)
    dist = torch.rand(Q, N, generator=g)
    nv = torch.randint(0, N + 1, (Q,), generator=g).int()
    got = native.rerank_select(s.to(DEV), ids.to(DEV), dist.to(DEV), nv.to(DEV), k)
    for o, w in zip(got, C.select_oracle(s, ids, dist, nv, k)):
        assert C.bits_equal(o.cpu(), w)
    z = torch.zeros(1, 65, device=DEV)
    with pytest.raises(ValueError, match="N must be"):
        native.rerank_select(z, z.long(), z, torch.zeros(1, dtype=torch.int32, device=DEV), 3)
    with pytest.raises(ValueError, match="k must be"):
        native.rerank_select(z[:, :8].contiguous(), z[:, :8].long().contiguous(), z[:, :8].contiguous(),
                             torch.zeros(1, dtype=torch.int32, device=DEV), 9)


# ------------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize("kind,H,heads", C.MODELS)
def test_scores_vs_transformers(native, kind, H, heads):
    """12 pairs of lengths 3 ... max_len in one packed batch: GPU scores within 2 e_cpu of fp32 transformers
    (e_cpu: the CPU backend's own error on the same pairs, recomputed here), and the GPU order agrees with the
    fp32 order across every adjacent gap wider than 4 e_cpu."""
    pytest.importorskip("transformers")
    path = C.checkpoint(kind, H, heads)
    pairs, ref = C.token_pairs(path)
    typed = kind == "bert"
    cpu = C.load_model(path, "cpu").score_packed(*C.pack(pairs, "cpu", typed)).double().numpy()
    e_cpu = float(np.abs(cpu - ref).max())
    gaps, n_adj = C.ordering_gaps(ref, e_cpu)
    assert ref.std() >= 0.5 and len(gaps) >= 0.75 * n_adj  # conditions on the inputs (fp32 scores alone)
    assert e_cpu < C.E_BOUND
    gpu = C.load_model(path, DEV).score_packed(*C.pack(pairs, DEV, typed))
    assert gpu.dtype == torch.float32 and gpu.shape == (12,)
    gpu = gpu.cpu().double().numpy()
    e_gpu = float(np.abs(gpu - ref).max())
    print("%s H=%d: e_cpu = %.5f, e_gpu = %.5f, std = %.3f, %d / %d gaps" % (kind, H, e_cpu, e_gpu, ref.std(),
                                                                            len(gaps), n_adj))
    assert e_gpu <= 2 * e_cpu, "e_gpu = %.5f, e_cpu = %.5f" % (e_gpu, e_cpu)
    assert all(gpu[a] > gpu[b] for a, b in gaps)


# ------------------------------------------------------------------------------------------ end to end
def test_tiny_rag_workload_with_reranker(native, tmp_path):
    """The tiny workload of test_e2e_gpu.py with a reranker attached: the GPU service returns the chunk order of a
    CPU service holding the same weights, the same store and the same queries (compared on chunk ids)."""
    from rag_llm_k8s_amd.engine.encoder_engine import EmbeddingEngine
    from rag_llm_k8s_amd.engine.llm_engine import SamplingParams
    from rag_llm_k8s_amd.engine.rerank_engine import Reranker
    from rag_llm_k8s_amd.index.store import DocumentStore
    from rag_llm_k8s_amd.models.encoder import EncoderModel
    from rag_llm_k8s_amd.server.rag_service import RagService
    from rag_llm_k8s_amd.utils.workload import build_workload, make_queries

    wl = build_workload(model="tiny", embedder="tiny", n_chunks=32, chunk_words=120, retrieve_k=3, context_k=3,
                        max_new_tokens=8, max_batch=4, max_model_len=2048, max_prefill_tokens=4096, device="cuda:0",
                        word_vocab=20000, reranker="tiny", rerank_candidates=32, rerank_max_len=128)
    svc = wl.svc
    assert svc.reranker is not None and svc.cfg.rerank_candidates == 32
    # the CPU twin: same embedder and reranker weights, the same vectors and metadata
    emb, rr = svc.embedder, svc.reranker
    emb_c = EmbeddingEngine(EncoderModel(emb.model.cfg, emb.model.w.to("cpu"), "cpu"), emb.tok)
    rr_c = Reranker(EncoderModel(rr.model.cfg, rr.model.w.to("cpu"), "cpu"), rr.tok, max_len=128)
    store_c = DocumentStore(str(tmp_path / "cpu_index"), emb.dim, device="cpu")
    chunks = [m["text"] for m in svc.store.metadata]
    store_c.add(svc.embedder.embed(chunks).cpu(), list(svc.store.metadata), dedupe=False, persist=False)
    twin = RagService(svc.cfg.replace(device="cpu"), svc.engine, svc.tok, emb_c, store_c, start_threads=False,
                      reranker=rr_c)
    # Queries (chosen on the CPU scores alone): the 3 of a pool of 64 whose best 4 candidate scores -- the 3 kept
    # and the first one dropped -- lie farthest apart. Each backend stays within E_BOUND of the fp32 scores on
    # this model family (the model tests), so an order across gaps wider than 2 E_BOUND cannot depend on the
    # device; two of 32 random candidates a hair apart would make the comparison a coin toss.
    pool = make_queries(wl.wm, 64, seed=1)
    every = twin.store.search(emb_c.embed(pool), 32)
    assert all(len(r) == 32 for r in every)  # the candidates are the whole corpus on either device
    margin = []
    for s in rr_c.score(pool, [[m["text"] for m, _ in r] for r in every]):
        top = np.sort(s)[::-1][:4]
        margin.append(float((top[:-1] - top[1:]).min()))
    best = np.argsort(margin)[::-1][:3]
    assert min(margin[i] for i in best) > 2 * C.E_BOUND, sorted(margin)[-3:]
    qs = [pool[i] for i in best]
    want = [[(m["filename"], m["chunk_id"]) for m, _ in res] for res, _ in twin._retrieve_batch([(q, None) for q in qs])]

    outs = svc.generate_batch(qs, params=SamplingParams(max_new_tokens=8, temperature=0.7, top_p=0.9, top_k=50,
                                                        ignore_eos=True), seeds=[1, 2, 3])
    torch.cuda.synchronize()
    plain = svc.generate_batch(qs, params=SamplingParams(max_new_tokens=2, ignore_eos=True), seeds=[1, 2, 3],
                               rerank=False)
    for o, p, w in zip(outs, plain, want):
        assert o["_gen_tokens"] == 8 and o["context"].startswith("Document 'synthetic_")
        assert o["context"].count("(chunk ") == 3 and len(p["_retrieved"]) == 3
        assert o["_retrieved"] == w
    assert want != [p["_retrieved"] for p in plain], "the reranker changed no order: the comparison would be vacuous"
    assert not any("rerank_score" in m for m in svc.store.metadata)
