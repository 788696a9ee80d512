#!/usr/bin/env python3
"""Time the built-in denoiser (rt_denoise_async) on device-resident frames.

    tools/denoise_bench.py [--sizes 1200x900,3840x2880] [--iterations 5] [--reps 20] [--warmup 3] [--label TAG]

Seeded random planes (the tests' distribution); per size one JSON line with
the mean call time from device events, the compulsory bytes of one pass (48 B
per pixel: three float3 planes read, one written) and a SHA-1 of the filtered
canva, so two builds can be compared on what they compute as well as on how
fast.  Per-pass kernel times come from running this under
`rocprofv3 --kernel-trace --stats` (a run of its own) and
tools/denoise_trace_summary.py."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tipe-raytracer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1200x900,3840x2880")
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    import torch
    import tipe_rt
    if not torch.cuda.is_available():
        sys.exit("denoise_bench: needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    params = tipe_rt.denoise_params(iterations=args.iterations)
    stream = torch.cuda.current_stream().cuda_stream
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        g = torch.Generator(device=dev).manual_seed(W * 10007 + H)
        canva0 = torch.randint(0, 256, (H, W, 3), generator=g, device=dev).to(torch.float64)
        albedo = torch.rand((H, W, 3), generator=g, device=dev, dtype=torch.float64)
        normal = torch.rand((H, W, 3), generator=g, device=dev, dtype=torch.float64) * 2 - 1
        nbytes = tipe_rt.lib().rt_denoise_workspace_bytes(W, H)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        canva = canva0.clone()

        def call():
            canva.copy_(canva0)
            tipe_rt.denoise_async(W, H, canva.data_ptr(), albedo.data_ptr(), normal.data_ptr(), params,
                                  ws.data_ptr(), nbytes, None, stream)

        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            call()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.reps
        digest = hashlib.sha1(canva.cpu().numpy().tobytes()).hexdigest()
        print(json.dumps({"label": args.label, "W": W, "H": H, "iterations": args.iterations, "reps": args.reps,
                          "call_ms_incl_frame_copy": round(ms, 4), "pass_compulsory_bytes": 48 * W * H,
                          "canva_sha1": digest}), flush=True)


if __name__ == "__main__":
    main()
