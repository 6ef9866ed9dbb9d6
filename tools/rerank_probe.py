"""Cost of the cross-encoder reranking stage on one MI355X, with random weights.

python tools/rerank_probe.py [--quick] [--out profiles/rerank_probe.log]

One micro-batch = 32 queries x 32 candidates = 1024 (query, chunk) pairs: ~20-token queries, chunks truncated so
that a pair fills the 512-token limit (1000-word chunks always do). For a MiniLM-L6 shaped (H = 384, 6 layers)
and a bge-large shaped (H = 1024, 24 layers) BERT cross-encoder the probe times, with device events around whole
passes (one warm-up pass, then `--rounds` timed ones; median and min..max are printed):
  * score: all pairs through EncoderModel.score_packed in packed batches of <= 65536 tokens (what
    Reranker.score runs after tokenisation), with the achieved TFLOP/s from the FLOPs of the shapes;
  * cls_head alone at B = 1024, and rerank_select alone at Q = 32, N = 32, k = 5 (many launches per pass).
The numbers go into docs/PERF_NOTES.md. A run without a GPU fails: a CPU timing says nothing here.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rag_llm_k8s_amd.engine.encoder_engine import pack_batches  # noqa: E402
from rag_llm_k8s_amd.models import encoder as E  # noqa: E402
from rag_llm_k8s_amd.ops import native as N  # noqa: E402

SHAPES = {"minilm-l6": E.minilm_l6, "bge-large": E.bge_large_en}


def timed(fn, rounds, iters=1):
    """ms per call of fn: `rounds` windows of `iters` calls between device events, after one warm-up window."""
    out = []
    for r in range(rounds + 1):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        if r:
            out.append(s.elapsed_time(e) / iters)
    return statistics.median(out), min(out), max(out)


def flops(cfg, lens):
    """Multiply-adds x 2 of the encoder layers (GEMMs + attention) and the head for packed sequences `lens`."""
    H, I, T = cfg.hidden_size, cfg.intermediate_size, int(np.sum(lens))
    gemm = 2 * T * (4 * H * H + 2 * H * I)
    attn = 4 * H * int(np.sum(np.asarray(lens, dtype=np.int64) ** 2))
    return cfg.num_hidden_layers * (gemm + attn) + 2 * len(lens) * H * H


def micro_batch(cfg, queries, cands, max_len, rng):
    """Packed (ids, lens, type_ids) batches of queries x cands pairs: [CLS] q [SEP] d [SEP], d filling max_len."""
    pairs = []
    for _ in range(queries):
        nq = int(rng.integers(16, 25))
        for _ in range(cands):
            nd = max_len - 3 - nq
            ids = rng.integers(1000, cfg.vocab_size, max_len).astype(np.int32)
            types = np.concatenate([np.zeros(nq + 2, dtype=np.int32), np.ones(nd + 1, dtype=np.int32)])
            pairs.append((ids, types))
    lens = np.array([len(p[0]) for p in pairs], dtype=np.int32)
    out = []
    for rows, row_lens in pack_batches(lens, 65536):
        out.append((torch.from_numpy(np.concatenate([pairs[r][0] for r in rows])).cuda(), [int(x) for x in row_lens],
                    torch.from_numpy(np.concatenate([pairs[r][1] for r in rows])).cuda()))
    return out, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="4 x 8 pairs of 128 tokens (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rerank_probe needs a GPU: nothing is measured on a CPU")
    lines = []

    def say(msg):
        print(msg, flush=True)
        lines.append(msg)

    Q, C, L = (4, 8, 128) if a.quick else (32, 32, 512)
    say("rerank_probe: %d queries x %d candidates, pairs of %d tokens, %s, torch %s" % (
        Q, C, L, torch.cuda.get_device_name(0), torch.__version__))
    rng = np.random.default_rng(0)
    with torch.no_grad():
        for name, mk in SHAPES.items():
            cfg = mk()
            model = E.EncoderModel(cfg, E.EncoderWeights.random(cfg, "cuda", seed=1, head=True, head_scale=2.0), "cuda")
            batches, lens = micro_batch(cfg, Q, C, L, rng)

            def score():
                return [model.score_packed(i, ln, t) for i, ln, t in batches]

            med, lo, hi = timed(score, a.rounds)
            fl = flops(cfg, lens)
            say("%-10s score   %4d pairs %7d tokens %2d batches: %9.2f ms (min %.2f max %.2f)  %6.1f TFLOP/s  "
                "%.3f PFLOP" % (name, len(lens), int(lens.sum()), len(batches), med, lo, hi, fl / med / 1e9, fl / 1e15))
            H, B = cfg.hidden_size, Q * C
            h = torch.randn(B * 4, H, device="cuda").bfloat16()
            cu = (torch.arange(B + 1, dtype=torch.int32) * 4).cuda()
            hd = model.w.head
            out = torch.empty(B, dtype=torch.float32, device="cuda")
            med, lo, hi = timed(lambda: N.cls_head(h, cu, hd["w1"], hd["b1"], hd["w2"], hd["b2"], out=out), a.rounds, 200)
            say("%-10s cls_head B = %d H = %d: %8.1f us (min %.1f max %.1f)" % (name, B, H, med * 1e3, lo * 1e3, hi * 1e3))
        s = torch.randn(Q, C, device="cuda")
        ids = torch.arange(Q * C, device="cuda").view(Q, C)
        dist = torch.rand(Q, C, device="cuda")
        nv = torch.full((Q,), C, dtype=torch.int32, device="cuda")
        k = min(5, C)
        out = N.rerank_select(s, ids, dist, nv, k)
        med, lo, hi = timed(lambda: N.rerank_select(s, ids, dist, nv, k, out=out), a.rounds, 200)
        say("rerank_select Q = %d N = %d k = %d: %8.1f us (min %.1f max %.1f)" % (Q, C, k, med * 1e3, lo * 1e3, hi * 1e3))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
