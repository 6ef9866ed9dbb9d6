"""Cost of the logit-processor launch next to the decode sampler, on one GPU: device time of one
(top-k, sample) pair with and without ragk_logits_process in front of it, at B = 1 and B = 32 over a Llama-3
vocabulary (128256 fp32 logits per row), every row with a 5200-token history in a max_model_len = 16384 buffer
and all three processors on (repetition penalty 1.3, 3-gram ban, 3 banned stop ids), the decode form (the
kernel stores the step's id first). Chunking as the engine picks it (llm_engine.SMALL_BATCH_TOPK_*). Each figure
is the median of 5 x 5 replays of a hipGraph that holds 20 copies of the sequence. The processor runs in place,
so the penalised logits shrink from replay to replay; its work does not depend on their values. Prints one JSON
line per batch size.

--penalties: the penalty form of the launch (ragk_logits_process_pen: logit_bias, frequency and presence penalties
on top of the three processors above, all six on) alone in a graph, against the old launch alone on the same
history, at B = 1 and B = 32: 5200-token prompts followed by a generated span of 150 or 8192 tokens (ids drawn
from the whole vocabulary, so nearly all distinct: the counting table at its fullest), with 0 and with 300 bias
entries. One JSON line per (batch, span, bias entries)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rag_llm_k8s_amd.ops import native as N  # noqa: E402

V, K, HIST, MAX_LEN, BAN_W = 128256, 64, 5200, 16384, 16
BIAS_W = 300


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


def penalties():
    dev = "cuda"
    for B in (1, 32):
        g = torch.Generator(device=dev).manual_seed(B)
        logits = torch.randn(B, V, device=dev, generator=g) * 3
        hist = torch.randint(0, V, (B, MAX_LEN), device=dev, generator=g, dtype=torch.int32)
        rows = torch.arange(B, dtype=torch.int32, device=dev)
        ids = torch.randint(0, V, (B,), device=dev, generator=g, dtype=torch.int32)
        pen = torch.full((B,), 1.3, device=dev)
        ng = torch.full((B,), 3, dtype=torch.int32, device=dev)
        ban_ids = torch.zeros((B, BAN_W), dtype=torch.int32, device=dev)
        ban_ids[:, :3] = torch.tensor([128001, 128008, 128009], dtype=torch.int32, device=dev)
        ban_count = torch.full((B,), 3, dtype=torch.int32, device=dev)
        gen_start = torch.full((B,), HIST, dtype=torch.int32, device=dev)
        pres = torch.full((B,), 0.5, device=dev)
        freq = torch.full((B,), 0.25, device=dev)
        bias_ids = torch.stack([torch.randperm(V, device=dev, generator=g)[:BIAS_W] for _ in range(B)]).int()
        bias_vals = torch.rand(B, BIAS_W, device=dev, generator=g) * 2 - 1
        for span in (150, 8192):
            pos = torch.full((B,), HIST + span - 1, dtype=torch.int32, device=dev)

            def old():
                N.logits_process(logits, 0, ids, rows, pos, hist, pen, ng, ban_ids, ban_count)

            t_old = timed(graph_of(old).replay) / 20
            for nbias in (0, BIAS_W):
                bias_count = torch.full((B,), nbias, dtype=torch.int32, device=dev)

                def new():
                    N.logits_process(logits, 0, ids, rows, pos, hist, pen, ng, ban_ids, ban_count,
                                     gen_start=gen_start, presence=pres, frequency=freq, bias_ids=bias_ids,
                                     bias_vals=bias_vals, bias_count=bias_count, gen_bound=span)

                t_new = timed(graph_of(new).replay) / 20
                print(json.dumps({"B": B, "V": V, "prompt": HIST, "span": span, "bias": nbias,
                                  "old_alone_dev_us": round(t_old, 2), "pen_alone_dev_us": round(t_new, 2),
                                  "added_us": round(t_new - t_old, 2)}), flush=True)


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
        hist = torch.randint(0, V, (B, MAX_LEN), device=dev, generator=g, dtype=torch.int32)
        rows = torch.arange(B, dtype=torch.int32, device=dev)
        pos = torch.full((B,), HIST - 1, dtype=torch.int32, device=dev)
        ids = torch.randint(0, V, (B,), device=dev, generator=g, dtype=torch.int32)
        pen = torch.full((B,), 1.3, device=dev)
        ng = torch.full((B,), 3, dtype=torch.int32, device=dev)
        ban_ids = torch.zeros((B, BAN_W), dtype=torch.int32, device=dev)
        ban_ids[:, :3] = torch.tensor([128001, 128008, 128009], dtype=torch.int32, device=dev)
        ban_count = torch.full((B,), 3, dtype=torch.int32, device=dev)
        chunks = max(1, min(V // 4096, 2048 // K, 64))
        cv, ci = N.topk_candidates(logits, K, chunks=chunks)
        tok = torch.empty(B, dtype=torch.int32, device=dev)

        def sample():
            N.topk_candidates(logits, K, chunks=chunks, cand_v=cv, cand_i=ci)
            N.sample_candidates(cv, ci, temps, ks, ps, seeds, steps, out_tok=tok, list_len=K)

        def proc():
            N.logits_process(logits, 0, ids, rows, pos, hist, pen, ng, ban_ids, ban_count)

        def both():
            proc()
            sample()

        t_s = timed(graph_of(sample).replay) / 20
        t_b = timed(graph_of(both).replay) / 20
        t_p = timed(graph_of(proc).replay) / 20
        print(json.dumps({"B": B, "V": V, "hist": HIST, "chunks": chunks, "topk_sample_dev_us": round(t_s, 2),
                          "proc_topk_sample_dev_us": round(t_b, 2), "proc_alone_dev_us": round(t_p, 2),
                          "added_us": round(t_b - t_s, 2)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--penalties", action="store_true", help="measure the penalty form of the launch instead")
    penalties() if ap.parse_args().penalties else main()
