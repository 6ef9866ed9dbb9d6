"""Filtered (masked) vs unfiltered L2 search on one MI355X.

python tools/bench_filtered_search.py [--quick] [--baseline-lib PATH] [--out bench_out/filtered_search.json]

For every shape (N x d, nq, k) these are timed in alternation, `--rounds` times each, with device events around
`--iters` back-to-back searches: the unmasked search; the masked search with an all-ones bitmap (100 %: the
cost of the mask lookup alone), with a random 50 % bitmap, and with every query unfiltered (qmask -1: the masked
kernels without any bitmap load) -- all four through the C entry points on preallocated buffers, so the numbers
are the two kernels plus two ctypes calls; and "*_call", the same search through ops/native (argument checks,
output allocation, upload of a host qmask), which is what a caller pays. The table shows the median and the
min..max spread of the rounds, which is the run-to-run noise a difference has to exceed. --baseline-lib names a
libragk_hip.so built from another commit: its ragk_l2_search joins the alternation ("base"), so old and new
unmasked kernels are compared in the same process on the same data.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rag_llm_k8s_amd.index.flat import pack_masks  # noqa: E402
from rag_llm_k8s_amd.ops import _lib  # noqa: E402
from rag_llm_k8s_amd.ops import native as N  # noqa: E402

SHAPES = [(10000, 384, 32, 4), (1000000, 384, 1, 4), (1000000, 384, 32, 4)]


def event_time(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def direct_search(h, masked=False):
    """The C entry point of kernel library h (ragk_l2_search, or ragk_l2_search_masked) on preallocated buffers:
    the two kernels and two ctypes calls, without the Python wrapper's checks and allocations."""
    name = "ragk_l2_search_masked" if masked else "ragk_l2_search"
    fn = getattr(h, name)
    fn.argtypes, fn.restype = _lib._SIGS[name], ctypes.c_int
    groups = _lib.lib().ragk_l2_search_groups

    def search(xt, n, q, k, masks=None, qmask=None):
        nq, d = q.shape
        G = groups(0, n, nq, k, d)
        pd = torch.empty(nq * G * k, dtype=torch.float32, device=q.device)
        pi = torch.empty(nq * G * k, dtype=torch.int32, device=q.device)
        od, oi = N._search_out(nq, k, q.device)
        head = (xt.data_ptr(), xt.shape[1], d, 0, n, q.data_ptr(), nq, k, None)
        mid = (masks.data_ptr(), masks.shape[1], 32 * masks.shape[1], qmask.data_ptr()) if masked else ()
        tail = (pd.data_ptr(), pi.data_ptr(), od.data_ptr(), oi.data_ptr())

        def run():
            N.check(fn(*head, *mid, *tail, N.stream_ptr()), name)
            return od, oi
        return run
    return search


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="10k x 384 only")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="bench_out/filtered_search.json")
    args = ap.parse_args()
    dev = "cuda"
    plain, masked = direct_search(_lib.lib()), direct_search(_lib.lib(), masked=True)
    base = direct_search(ctypes.CDLL(args.baseline_lib)) if args.baseline_lib else None
    rows = []
    for n, d, nq, k in (SHAPES[:1] if args.quick else SHAPES):
        torch.manual_seed(0)
        xt = torch.randn(d, n, device=dev)
        q = torch.randn(nq, d, device=dev)
        g = np.random.default_rng(0)
        m100 = torch.from_numpy(pack_masks(np.ones((1, n), dtype=bool)).view(np.int32)).to(dev)
        m50 = torch.from_numpy(pack_masks(g.random((1, n)) < 0.5).view(np.int32)).to(dev)
        qm = torch.zeros(nq, dtype=torch.int32, device=dev)
        qnone = torch.full((nq,), -1, dtype=torch.int32, device=dev)
        hq = torch.zeros(nq, dtype=torch.int32)  # a host qmask, as DocumentStore.search passes it
        variants = {"unmasked": plain(xt, n, q, k),
                    "mask100": masked(xt, n, q, k, m100, qm),
                    "mask50": masked(xt, n, q, k, m50, qm),
                    # every query unfiltered (qmask -1): the masked kernels without any bitmap load -- what
                    # remains over "unmasked" is the per-query id bookkeeping
                    "masknone": masked(xt, n, q, k, m100, qnone),
                    # through ops/native (argument checks, output allocation, qmask upload): what a caller pays
                    "unmasked_call": lambda: N.l2_search(xt, n, n, q, k),
                    "mask50_call": lambda: N.l2_search(xt, n, n, q, k, masks=m50, qmask=hq)}
        if base is not None:
            variants["base"] = base(xt, n, q, k)
        ref = variants["unmasked"]()
        for name in ("mask100", "masknone", "base"):  # same results: all allowed, and the other build's kernels
            if name in variants:
                got = variants[name]()
                assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), name
        iters = max(5, args.iters // (20 if n >= 1000000 else 1))
        for fn in variants.values():  # warm-up: code objects loaded, workspace grown
            event_time(fn, 3)
        times = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                times[name].append(event_time(fn, iters))
        row = dict(N=n, d=d, nq=nq, k=k, iters=iters, rounds=args.rounds)
        for name, t in times.items():
            row[name + "_us"] = round(statistics.median(t), 2)
            row[name + "_min_us"], row[name + "_max_us"] = round(min(t), 2), round(max(t), 2)
        row["GBps_unmasked"] = round(n * d * 4 / row["unmasked_us"] / 1e3, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(), "time": time.time(), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
