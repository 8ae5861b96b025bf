#!/usr/bin/env python3
"""Per-projection times of the quantised-weight routes on one GPU: ops.linear_w8, ops.linear_w8a8
(M > 4), ops.linear_w4 (G = 128) and ops.linear_mxfp4 at Llama-3-8B's four projection shapes,
alternated in one process over rotating weight copies (600 MB or more per format, so no copy is
served from cache), median of --windows windows, device events around each window.  Prints the
markdown table of profiles/weights_mxfp4/README.md; GB/s = codes + scales (+ zero points) / time."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from langstream_amd import ops  # noqa: E402

DEV = "cuda"
SHAPES = {"6144 x 4096": (6144, 4096), "4096 x 4096": (4096, 4096), "28672 x 4096": (28672, 4096),
          "4096 x 14336": (4096, 14336)}


def copies(make, nbytes):
    return [make() for _ in range(max(2, min(8, -(-(600 << 20) // nbytes))))]


def window(fn, ws, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(ws[i % len(ws)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 4, 16, 64, 256, 2048])
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda hi, *shape: torch.randint(0, hi, shape, device=DEV, dtype=torch.uint8, generator=g)  # noqa: E731
    print("| N x K | M | w8 us | w8a8 us | w4 us | mxfp4 us | w8 GB/s | w4 GB/s | mxfp4 GB/s | fp8 time / mxfp4 time |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name, (N, K) in SHAPES.items():
        w8s = copies(lambda: (rnd(120, N, K).view(torch.float8_e4m3fn), torch.rand(N, device=DEV) + 0.5), N * K)
        w4s = copies(lambda: (rnd(256, N, K // 2), torch.rand(N, K // 128, device=DEV) * 0.01 + 0.001,
                              rnd(16, N, K // 128)), N * K // 2)
        mxs = copies(lambda: (rnd(256, N, K // 2), rnd(10, N, K // 32) + 120), N * K // 2)
        b8, b4, bx = N * K + 4 * N, N * K // 2 + 5 * N * K // 128, N * K // 2 + N * K // 32
        for M in args.rows:
            x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
            out = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
            fns = {"w8": (lambda w: ops.linear_w8(x, w[0], w[1], out=out), w8s),
                   "w8a8": (lambda w: ops.linear_w8a8(x, w[0], w[1], out=out), w8s),
                   "w4": (lambda w: ops.linear_w4(x, w[0], w[1], w[2], out=out), w4s),
                   "mx": (lambda w: ops.linear_mxfp4(x, w[0], w[1], out=out), mxs)}
            if M <= 4:
                del fns["w8a8"]
            iters = 40 if M <= 256 else 12
            for fn, ws in fns.values():
                window(fn, ws, 8)          # warm every shape of the timed windows
            t = {k: [] for k in fns}
            for _ in range(args.windows):
                for k, (fn, ws) in fns.items():
                    t[k].append(window(fn, ws, iters))
            m = {k: statistics.median(v) for k, v in t.items()}
            best8 = min(m["w8"], m.get("w8a8", float("inf")))
            a8 = f"{m['w8a8']:.1f}" if "w8a8" in m else "-"
            print(f"| {name} | {M} | {m['w8']:.1f} | {a8} | {m['w4']:.1f} | {m['mx']:.1f} | {b8 / m['w8'] / 1e3:.0f} | "
                  f"{b4 / m['w4'] / 1e3:.0f} | {bx / m['mx'] / 1e3:.0f} | "
                  f"{'faster' if m['mx'] < best8 else 'slower'} ({best8 / m['mx']:.2f}x) |", flush=True)
        del w8s, w4s, mxs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
