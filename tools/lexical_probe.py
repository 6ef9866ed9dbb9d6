"""Cost of the BM25 lexical search next to the dense search, on one GPU, same session and box: device time of
one (lex_df, lex_search) pair for a micro-batch of 32 queries of about 12 terms at depth k = 32 over N = 10,000 and
100,000 analysed 1000-word synthetic chunks (utils/workload.make_chunks, the bench corpus' word model), and next
to it l2_search for 32 queries at the same N and k over 384-dim vectors (the MiniLM shape of the bench). Also the
host-inclusive time of LexicalIndex.search (query analysis, the df read-back, idf, uploads, both launches, the
result copy), the analyse-and-build time of the index at start-up and its bytes. Each device figure is the median
of 5 x 10 launches. Prints one JSON line per N.

Not measured here: a served request, the IVF index at 1M chunks, tensor parallelism."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rag_llm_k8s_amd.index.flat import FlatL2Index  # noqa: E402
from rag_llm_k8s_amd.index.lexical import LexicalIndex, bm25_idf, launch_table, query_terms  # noqa: E402
from rag_llm_k8s_amd.ops import native as N  # noqa: E402
from rag_llm_k8s_amd.utils.synthetic import WordModel  # noqa: E402
from rag_llm_k8s_amd.utils.workload import make_chunks, make_queries  # noqa: E402

NQ, K, DIM, PIECE = 32, 32, 384, 10000


def timed(fn, iters=10, reps=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return sorted(out)[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--chunk-words", type=int, default=1000)
    args = ap.parse_args()
    dev = "cuda:0"
    wm = WordModel(n_words=400000, seed=0)
    queries = make_queries(wm, NQ, seed=1, words=12)
    qts = [query_terms(q) for q in queries]
    terms, member = launch_table(qts)
    qt = torch.from_numpy(terms.view(np.int32)).to(dev)
    mem = torch.from_numpy(member.view(np.int64)).to(dev)
    for n in [int(s) for s in args.sizes.split(",")]:
        idx = LexicalIndex(dev)
        t_build = 0.0
        for p0 in range(0, n, PIECE):  # the corpus in pieces of 10,000 chunks (bounded host memory)
            chunks = make_chunks(wm, min(PIECE, n - p0), args.chunk_words, seed=p0 // PIECE)
            t0 = time.perf_counter()
            idx.add(chunks)
            torch.cuda.synchronize()
            t_build += time.perf_counter() - t0
        n_live, avgdl = idx.live_stats(None)
        df = N.lex_df(idx._row_ptr, idx._terms, n, qt)
        idf = torch.from_numpy(bm25_idf(df.cpu().numpy(), n_live)).to(dev)
        csr = (idx._row_ptr, idx._terms, idx._tf, idx._doc_len, n)

        def lex():
            N.lex_df(idx._row_ptr, idx._terms, n, qt)
            N.lex_search(*csr, qt, idf, mem, NQ, 1.2, 2.2, 0.75, avgdl, K)

        t_df = timed(lambda: N.lex_df(idx._row_ptr, idx._terms, n, qt))
        t_lex = timed(lex)
        t0 = time.perf_counter()
        for _ in range(5):
            S, I = idx.search(queries, K)
        t_host = (time.perf_counter() - t0) / 5
        g = torch.Generator().manual_seed(n)
        flat = FlatL2Index(DIM, device=dev, capacity=n)
        for p0 in range(0, n, PIECE):
            flat.add(torch.nn.functional.normalize(torch.randn(min(PIECE, n - p0), DIM, generator=g), dim=1))
        q = torch.nn.functional.normalize(torch.randn(NQ, DIM, generator=g), dim=1).to(dev)
        t_l2 = timed(lambda: flat.search_device(q, K))
        t_l2_k5 = timed(lambda: flat.search_device(q, 5))
        print(json.dumps({
            "n_chunks": n, "chunk_words": args.chunk_words, "queries": NQ, "terms": int(len(terms)), "k": K,
            "lex_df_us": round(t_df, 1), "lex_df_plus_search_us": round(t_lex, 1),
            "l2_search_k32_us": round(t_l2, 1), "l2_search_k5_us": round(t_l2_k5, 1),
            "ratio_lex_to_l2_k32": round(t_lex / t_l2, 2),
            "index_search_host_ms": round(t_host * 1e3, 3), "analyse_and_build_s": round(t_build, 2),
            "entries": int(idx.nnz), "index_bytes": int((n + 1) * 8 + idx.nnz * 6 + n * 4),
            "allocated_bytes": int(idx.memory_bytes()), "avgdl": avgdl,
            "matched_lists": int((I >= 0).all(1).sum())}), flush=True)
        del idx, flat
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
