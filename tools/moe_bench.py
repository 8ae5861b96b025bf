"""One mixture-of-experts layer (ops/csrc/moe.hip: route, align, two grouped GEMMs, combine) with
bf16, fp8 and int4 experts, alternated in one process over rotating weight copies larger than the
caches.  Prints one JSON line per (T, variant): median (min - max) us per call over the windows and
the GB/s of the weights actually read (router, the three matrices of every expert that received a
token, and their scales and zero points).

  python tools/moe_bench.py --shape qwen3 --T 1 16 256 4096
  python tools/moe_bench.py --shape mixtral --T 16 --variants bf16 --so <another build's _hip_ops.so>
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from langstream_amd import ops  # noqa: E402
from langstream_amd.models.llama import quantize_experts_fp8, quantize_experts_int4  # noqa: E402

SHAPES = {"qwen3": (128, 8, 2048, 768, 4), "mixtral": (8, 2, 4096, 14336, 3)}   # E, k, H, F, weight copies


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="qwen3")
    ap.add_argument("--T", type=int, nargs="+", default=[1, 16, 256, 4096])
    ap.add_argument("--variants", nargs="+", choices=("bf16", "fp8", "int4"), default=["bf16", "fp8", "int4"])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--so", help="time another build of the extension (bf16 only before fp8 experts, no int4 before int4 experts)")
    args = ap.parse_args()
    if args.so:
        ops._SO = os.path.abspath(args.so)
    hip = ops.hip()
    E, k, H, F, copies = SHAPES[args.shape]
    dev = "cuda"
    torch.manual_seed(0)
    wr = torch.randn(E, H, device=dev, dtype=torch.bfloat16)
    gu = (torch.randn(E, 2 * F, H, device=dev, dtype=torch.bfloat16) / H ** 0.5)
    dn = (torch.randn(E, H, F, device=dev, dtype=torch.bfloat16) / F ** 0.5)
    sets = {}
    if "bf16" in args.variants:
        sets["bf16"] = [(gu.clone(), dn.clone(), {}) for _ in range(copies)]
    if "fp8" in args.variants:
        (gc, gs), (dc, ds) = quantize_experts_fp8(gu), quantize_experts_fp8(dn)
        sets["fp8"] = [(gc.clone(), dc.clone(), dict(gate_up_s=gs.clone(), down_s=ds.clone())) for _ in range(copies)]
    if "int4" in args.variants:   # groups of 128 input columns: 0.5 B + 5 / 128 B per weight
        (gc, gs, gz), (dc, ds, dz) = quantize_experts_int4(gu), quantize_experts_int4(dn)
        sets["int4"] = [(gc.clone(), dc.clone(), dict(gate_up_s=gs.clone(), down_s=ds.clone(), gate_up_z=gz.clone(),
                                                      down_z=dz.clone())) for _ in range(copies)]
    del gu, dn

    def call(x, out, ids, w, ws):
        hip.moe_route(ids, w, x, wr, True)
        hip.moe_experts(out, x, ws[0], ws[1], ids, w, 0, **ws[2])

    for T in args.T:
        x = torch.randn(T, H, device=dev, dtype=torch.bfloat16)
        out = torch.empty_like(x)
        ids = torch.empty(T, k, device=dev, dtype=torch.int32)
        w = torch.empty(T, k, device=dev, dtype=torch.float32)
        for v in sets:
            for ws in sets[v]:
                call(x, out, ids, w, ws)   # warm-up of every copy
        torch.cuda.synchronize()
        used = int(ids.unique().numel())
        times = {v: [] for v in sets}
        for _ in range(args.windows):
            for v in sets:   # alternate the variants window by window
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for i in range(args.calls):
                    call(x, out, ids, w, sets[v][i % copies])
                b.record()
                torch.cuda.synchronize()
                times[v].append(a.elapsed_time(b) * 1e3 / args.calls)
        for v, ts in times.items():
            wbytes = E * H * 2 + {"bf16": used * 3 * H * F * 2, "fp8": used * (3 * H * F + (2 * F + H) * 4),
                                  "int4": used * (3 * H * F // 2 + 3 * H * F // 128 * 5)}[v]
            med = statistics.median(ts)
            print(json.dumps({"shape": args.shape, "T": T, "variant": v, "experts_used": used, "weight_MB": round(wbytes / 1e6, 1), "us": round(med, 1),
                              "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                              "GB_s": round(wbytes / med / 1e3)}), flush=True)


if __name__ == "__main__":
    main()
