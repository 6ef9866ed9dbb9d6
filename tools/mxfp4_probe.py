"""Kernel timing probe for the MXFP4 weight GEMMs against this tree's fp8 and bf16 kernels, same process, same box.

Shapes: the four Llama-3.1-8B projections -- qkv (6144,4096), o (4096,4096), gate/up (2*14336,4096) with the
SiLU*up epilogue, down (4096,14336) -- at M = 1 and 32 (decode: weight-stream bound, reported as weight GB/s)
and M = 32768 (prefill: MFMA bound, reported as TFLOP/s; activations pre-quantized, so the fp8 / mxfp4 rows time
the GEMM kernel alone).

Method: decode launches are a few microseconds, less than the host side of a call, so each variant is captured
into a hipGraph of `copies` launches that rotate through enough weight copies to exceed the 256 MB infinity cache
(every launch streams its weights from HBM, as a decode step does); the graph is replayed between device events.
Variants are interleaved round by round and the median round is reported, with the minimum beside it.

  python tools/mxfp4_probe.py [--m 1,32,32768] [--rounds 5] > profiles/gemm_mxfp4_probe.log
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rag_llm_k8s_amd.ops import fp8 as F8  # noqa: E402
from rag_llm_k8s_amd.ops import mxfp4 as F4  # noqa: E402
from rag_llm_k8s_amd.ops import native as N  # noqa: E402

SHAPES = [("qkv", 6144, 4096, "none"), ("o", 4096, 4096, "none"), ("gate_up", 14336, 4096, "silu_mul"),
          ("down", 4096, 14336, "none")]
ROTATE_BYTES = 640 << 20  # weight bytes a rotation must cover (> 2x the 256 MB infinity cache)


def weight_bytes(w):
    return w.nbytes() if hasattr(w, "nbytes") and not isinstance(w, torch.Tensor) else w.numel() * w.element_size()


def clone_weight(w):
    if isinstance(w, F4.Mxfp4Weight):
        return F4.Mxfp4Weight(w.packed.clone(), w.scale.clone())
    if isinstance(w, F8.Fp8Weight):
        return F8.Fp8Weight(w.w8.clone(), w.scale.clone())
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


def decode_variants(x, ws, epi, out):
    """name -> callable(i) launching the kernel on weight copy i."""
    def fp8_dec(i):  # the gemm_fp8_dec kernel itself (the served fp8 route picks the stream kernel per shape)
        N.FP8_DEC_STREAM = False
        try:
            N.gemm_fp8(x, ws["fp8"][i], epi=epi, out=out)
        finally:
            N.FP8_DEC_STREAM = True

    return {"mxfp4": lambda i: N.gemm_mxfp4(x, ws["mxfp4"][i], epi=epi, out=out), "fp8_dec": fp8_dec,
            "fp8_served": lambda i: N.gemm_fp8(x, ws["fp8"][i], epi=epi, out=out),
            "bf16": lambda i: N.gemm(x, ws["bf16"][i], epi=epi, out=out)}


def probe_decode(M, name, n, k, epi, rounds):
    rows = 2 * n if epi == "silu_mul" else n
    w = (torch.randn(rows, k, device="cuda") / math.sqrt(k)).bfloat16()
    base = {"bf16": w, "fp8": F8.quantize_weight(w), "mxfp4": F4.quantize_weight(w)}
    ws = {}
    for key, b in base.items():
        copies = max(2, -(-ROTATE_BYTES // weight_bytes(b)))
        ws[key] = [b] + [clone_weight(b) for _ in range(copies - 1)]
    x = torch.randn(M, k, device="cuda").bfloat16()
    out = torch.empty(M, n, device="cuda").bfloat16()
    graphs, per = {}, {}
    for v, fn in decode_variants(x, ws, epi, out).items():
        key = "fp8" if v.startswith("fp8") else v
        cnt = len(ws[key])
        for i in range(min(cnt, 3)):  # warm up: code objects, workspaces
            fn(i)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(cnt):
                fn(i)
        g.replay()
        graphs[v], per[v] = g, (cnt, weight_bytes(base[key]))
    times = {v: [] for v in graphs}
    for _ in range(rounds):
        for v, g in graphs.items():
            reps = max(1, int(0.05 / (per[v][0] * 20e-6)))  # ~50 ms or more of device work per window
            times[v].append(timed(g.replay, reps) / per[v][0])
    for v in graphs:
        t = sorted(times[v])[len(times[v]) // 2]
        print("M=%-5d %-8s N=%-5d K=%-5d %-10s %8.2f us  %7.1f weight GB/s  (min %.2f us, %d copies)  vs fp8_dec %.2fx"
              % (M, name, rows, k, v, t * 1e6, per[v][1] / t / 1e9, min(times[v]) * 1e6, per[v][0],
                 sorted(times["fp8_dec"])[len(times["fp8_dec"]) // 2] / t), flush=True)


def probe_prefill(M, name, n, k, epi, rounds):
    rows = 2 * n if epi == "silu_mul" else n
    w = (torch.randn(rows, k, device="cuda") / math.sqrt(k)).bfloat16()
    w8, w4 = F8.quantize_weight(w), F4.quantize_weight(w)
    x = torch.randn(M, k, device="cuda").bfloat16()
    q, sa = N.quant_fp8_rows(x)
    out = torch.empty(M, n, device="cuda").bfloat16()
    e = N.EPI[epi]

    def fp8_tile():  # ragk_gemm_fp8 on the pre-quantized activations: gemm_fp8_tile alone
        N.check(N._lib.lib().ragk_gemm_fp8(None, 0, q.data_ptr(), q.stride(0), sa.data_ptr(), w8.w8.data_ptr(),
                                           w8.w8.stride(0), w8.scale.data_ptr(), out.data_ptr(), out.stride(0), None,
                                           None, 0, M, n, k, e, 0, N.stream_ptr()), "ragk_gemm_fp8")

    fns = {"mxfp4": lambda: N.gemm_mxfp4(None, w4, epi=epi, out=out, act=(q, sa)), "fp8_tile": fp8_tile,
           "bf16": lambda: N.gemm(x, w, epi=epi, out=out)}
    for fn in fns.values():
        fn()
        fn()
    times = {v: [] for v in fns}
    for _ in range(rounds):
        for v, fn in fns.items():
            times[v].append(timed(fn, 5))
    ref = sorted(times["fp8_tile"])[len(times["fp8_tile"]) // 2]
    for v in fns:
        t = sorted(times[v])[len(times[v]) // 2]
        print("M=%-5d %-8s N=%-5d K=%-5d %-10s %8.1f us  %7.1f TFLOP/s  (min %.1f us)  vs fp8_tile %.2fx"
              % (M, name, rows, k, v, t * 1e6, 2.0 * M * rows * k / t / 1e12, min(times[v]) * 1e6, ref / t), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", default="1,32,32768")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mxfp4_probe needs a GPU: timings are not measured without one")
    torch.manual_seed(0)
    print("device: %s" % torch.cuda.get_device_name(0))
    for M in (int(v) for v in a.m.split(",")):
        for name, n, k, epi in SHAPES:
            (probe_decode if M <= F8.DEC_MAX_M else probe_prefill)(M, name, n, k, epi, a.rounds)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
