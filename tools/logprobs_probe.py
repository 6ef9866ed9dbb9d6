"""Cost of the two logprob launches next to the decode sampler, on one GPU: device time of one (top-k, sample)
pair with and without ragk_lse_partials / ragk_logprobs_finish around it, at B = 1 and B = 32 over a Llama-3
vocabulary (128256 fp32 logits per row), every row asking for the 20 alternatives. Chunking as the engine picks
it (llm_engine.SMALL_BATCH_TOPK_*, reference.lse_chunks). Each figure is the median of 5 x 5 replays of a
hipGraph that holds 20 copies of the sequence, all measured in the same run. Prints one JSON line per batch
size; profiles/logprobs_probe.log is that output, redirected
(`python tools/logprobs_probe.py > profiles/logprobs_probe.log`)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rag_llm_k8s_amd.ops import native as N  # noqa: E402

V, K = 128256, 64


def timed(fn, iters=5, reps=5):
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


def graph_of(fn, copies=20):
    fn()  # first launch outside the capture (one-time kernel attributes)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st), torch.cuda.graph(g, stream=st):
        for _ in range(copies):
            fn()
    torch.cuda.current_stream().wait_stream(st)
    return g


def main():
    dev = "cuda"
    for B in (1, 32):
        g = torch.Generator(device=dev).manual_seed(B)
        logits = torch.randn(B, V, device=dev, generator=g) * 3
        temps = torch.full((B,), 0.7, device=dev)
        ks = torch.full((B,), 50, dtype=torch.int32, device=dev)
        ps = torch.full((B,), 0.9, device=dev)
        seeds = torch.arange(B, dtype=torch.int64, device=dev)
        steps = torch.zeros(B, dtype=torch.int32, device=dev)
        chunks = max(1, min(V // 4096, 2048 // K, 64))
        lchunks = N.lse_chunks(V, B)
        cv, ci = N.topk_candidates(logits, K, chunks=chunks)
        tok = torch.empty(B, dtype=torch.int32, device=dev)
        part = torch.empty((B, lchunks, 2), device=dev)
        nlp = torch.full((B,), N.LOGPROBS_MAX, dtype=torch.int32, device=dev)
        outs = [torch.zeros(B, device=dev), torch.zeros(B, device=dev), torch.zeros((B, N.LOGPROBS_MAX), device=dev),
                torch.zeros((B, N.LOGPROBS_MAX), dtype=torch.int32, device=dev)]

        def sample():
            N.topk_candidates(logits, K, chunks=chunks, cand_v=cv, cand_i=ci)
            N.sample_candidates(cv, ci, temps, ks, ps, seeds, steps, out_tok=tok, list_len=K)

        def lse():
            N.lse_partials(logits, lchunks, out=part)

        def finish():
            N.logprobs_finish(part, cv, ci, K, tok, nlp, *outs)

        def both():  # the engine's order: partials next to the top-k, the finish after the sampler
            N.topk_candidates(logits, K, chunks=chunks, cand_v=cv, cand_i=ci)
            lse()
            N.sample_candidates(cv, ci, temps, ks, ps, seeds, steps, out_tok=tok, list_len=K)
            finish()

        t_s = timed(graph_of(sample).replay) / 20
        t_b = timed(graph_of(both).replay) / 20
        t_l = timed(graph_of(lse).replay) / 20
        t_f = timed(graph_of(finish).replay) / 20
        print(json.dumps({"B": B, "V": V, "topk_chunks": chunks, "lse_chunks": lchunks,
                          "topk_sample_dev_us": round(t_s, 2), "with_logprobs_dev_us": round(t_b, 2),
                          "lse_partials_alone_dev_us": round(t_l, 2), "logprobs_finish_alone_dev_us": round(t_f, 2),
                          "added_us": round(t_b - t_s, 2)}), flush=True)


if __name__ == "__main__":
    main()
