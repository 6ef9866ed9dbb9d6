"""Kernel timing probe for the int4 (AWQ / GPTQ) weight kernels against this tree's MXFP4 and bf16 routes, same
process, same box.

Decode (M = 1, 32): the four Llama-3.1-8B projections -- qkv (6144,4096), o (4096,4096), gate/up (2*14336,4096)
with the SiLU*up epilogue, down (4096,14336) -- through gemm_int4 (fused W4A16), gemm_mxfp4 (the same 4.25 bits
per weight: the yardstick) and the bf16 decode route, reported as time and weight GB/s. Method as
tools/mxfp4_probe.py: each variant is captured into a hipGraph whose launches rotate through enough weight copies
to exceed the 256 MB infinity cache, variants are interleaved round by round, and the median round is reported
with the minimum and maximum beside it (the run-to-run spread).

Prefill (M = 128, 2048, 32768): dequant_int4 + the bf16 GEMM (the M > 64 route of an int4 weight) against the
bf16 GEMM alone on the same dequantized weight, and the dequant kernel alone in GB/s written.

  python tools/int4_probe.py [--m 1,32,128,2048,32768] [--rounds 5] > profiles/gemm_int4_probe.log
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rag_llm_k8s_amd.ops import int4 as I4  # noqa: E402
from rag_llm_k8s_amd.ops import mxfp4 as F4  # noqa: E402
from rag_llm_k8s_amd.ops import native as N  # noqa: E402

SHAPES = [("qkv", 6144, 4096, "none"), ("o", 4096, 4096, "none"), ("gate_up", 14336, 4096, "silu_mul"),
          ("down", 4096, 14336, "none")]
ROTATE_BYTES = 640 << 20  # weight bytes a rotation must cover (> 2x the 256 MB infinity cache)
DEC_MAX_M = 64


def weight_bytes(w):
    return w.numel() * w.element_size() if isinstance(w, torch.Tensor) else w.nbytes()


def clone_weight(w):
    if isinstance(w, I4.Int4Weight):
        return I4.Int4Weight(w.packed.clone(), w.meta.clone())
    if isinstance(w, F4.Mxfp4Weight):
        return F4.Mxfp4Weight(w.packed.clone(), w.scale.clone())
    return w.clone()


def timed(fn, reps):
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3 / reps


def med(ts):
    return sorted(ts)[len(ts) // 2]


def probe_decode(M, name, n, k, epi, rounds):
    rows = 2 * n if epi == "silu_mul" else n
    w = (torch.randn(rows, k, device="cuda") / math.sqrt(k)).bfloat16()
    base = {"int4": I4.quantize_weight(w), "mxfp4": F4.quantize_weight(w), "bf16": w}
    calls = {"int4": N.gemm_int4, "mxfp4": N.gemm_mxfp4, "bf16": N.gemm}
    x = torch.randn(M, k, device="cuda").bfloat16()
    out = torch.empty(M, n, device="cuda").bfloat16()
    graphs, per = {}, {}
    for v, b in base.items():
        cnt = max(2, -(-ROTATE_BYTES // weight_bytes(b)))
        ws = [b] + [clone_weight(b) for _ in range(cnt - 1)]
        for i in range(min(cnt, 3)):  # warm up: code objects, workspaces
            calls[v](x, ws[i], epi=epi, out=out)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for wi in ws:
                calls[v](x, wi, epi=epi, out=out)
        g.replay()
        graphs[v], per[v] = g, (cnt, weight_bytes(b), ws)
    times = {v: [] for v in graphs}
    for _ in range(rounds):
        for v, g in graphs.items():
            reps = max(1, int(0.05 / (per[v][0] * 20e-6)))  # ~50 ms or more of device work per window
            times[v].append(timed(g.replay, reps) / per[v][0])
    for v in graphs:
        t = med(times[v])
        print("M=%-5d %-8s N=%-5d K=%-5d %-6s %8.2f us  %7.1f weight GB/s  (min %.2f max %.2f us, %d copies)  "
              "vs mxfp4 %.2fx" % (M, name, rows, k, v, t * 1e6, per[v][1] / t / 1e9, min(times[v]) * 1e6,
                                  max(times[v]) * 1e6, per[v][0], med(times["mxfp4"]) / t), flush=True)


def probe_prefill(M, name, n, k, epi, rounds):
    rows = 2 * n if epi == "silu_mul" else n
    w4 = I4.quantize_weight((torch.randn(rows, k, device="cuda") / math.sqrt(k)).bfloat16())
    wb = N.dequant_int4(w4)  # the bf16 GEMM alone runs on the very weight the int4 route multiplies by
    x = torch.randn(M, k, device="cuda").bfloat16()
    out = torch.empty(M, n, device="cuda").bfloat16()
    fns = {"int4": lambda: N.gemm_int4_prefill(x, w4, epi=epi, out=out), "bf16": lambda: N.gemm(x, wb, epi=epi, out=out),
           "dequant": lambda: N.dequant_int4(w4, wb)}
    for fn in fns.values():
        fn()
        fn()
    times = {v: [] for v in fns}
    for _ in range(rounds):
        for v, fn in fns.items():
            times[v].append(timed(fn, max(5, int(0.05 / (2.0 * M * rows * k / 1e15 + 20e-6)))))
    flops = 2.0 * M * rows * k
    for v in ("int4", "bf16"):
        t = med(times[v])
        print("M=%-5d %-8s N=%-5d K=%-5d %-7s %9.1f us  %7.1f TFLOP/s  (min %.1f max %.1f us)  vs bf16 %.3fx"
              % (M, name, rows, k, v, t * 1e6, flops / t / 1e12, min(times[v]) * 1e6, max(times[v]) * 1e6,
                 med(times["bf16"]) / t), flush=True)
    t = med(times["dequant"])
    print("M=%-5d %-8s N=%-5d K=%-5d %-7s %9.1f us  %7.1f GB/s written  (min %.1f max %.1f us)"
          % (M, name, rows, k, "dequant", t * 1e6, 2.0 * rows * k / t / 1e9, min(times["dequant"]) * 1e6,
             max(times["dequant"]) * 1e6), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", default="1,32,128,2048,32768")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("int4_probe needs a GPU: timings are not measured without one")
    torch.manual_seed(0)
    print("device: %s" % torch.cuda.get_device_name(0))
    for M in (int(v) for v in a.m.split(",")):
        for name, n, k, epi in SHAPES:
            (probe_decode if M <= DEC_MAX_M else probe_prefill)(M, name, n, k, epi, a.rounds)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
