#!/usr/bin/env python3
"""Time the built-in denoisers (rt_denoise_async, rt_vdenoise_async, rt_vdenoise_adaptive_async) on
device-resident frames.

    tools/denoise_bench.py [--sizes 1200x900,3840x2880] [--iterations 5] [--reps 20] [--warmup 3] [--label TAG]
                           [--filter atrous|vdenoise|vdenoise_px|both|vpair] [--rounds 1]

Seeded random inputs (the tests' distributions); per size, round and filter
one JSON line with the mean call time from device events, the compulsory
bytes of one pass and a SHA-1 of the filtered canva, so two builds can be
compared on what they compute as well as on how fast.
  atrous    rt_denoise_async on random planes; 48 B per pixel and pass (three
            float3 planes read, one written); the call time includes the copy
            that restores the canva it filters in place.
  vdenoise  rt_vdenoise_async on two random accumulators (radiance in [0, 4] n,
            albedo in [0, 1] n, normal in [-1, 1] n, n = --spp-half); 68 B per
            pixel and pass (the pass reads c, v, a, nn and L and writes c and
            v: 60 B; the variance blur reads v and writes L: 8 B).
  vdenoise_px  rt_vdenoise_adaptive_async on two random accumulators whose pixel p holds
            n_p = spp_half * 2^(k-1) samples' worth, k seeded in 1..5 per pixel (first_half = --spp-half):
            the same passes; prepare and finish read 4 more bytes per pixel on 144.
  both      atrous and vdenoise alternate, round by round, in one process.
  vpair     vdenoise and vdenoise_px alternate, round by round, in one process.
Per-pass kernel times come from running this under
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
    ap.add_argument("--filter", choices=("atrous", "vdenoise", "vdenoise_px", "both", "vpair"), default="atrous")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--spp-half", type=int, default=8)
    args = ap.parse_args()
    import torch
    import tipe_rt
    if not torch.cuda.is_available():
        sys.exit("denoise_bench: needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def atrous(W, H):
        """(call, canva, extra fields of the JSON line)"""
        params = tipe_rt.denoise_params(iterations=args.iterations)
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

        return call, canva, "call_ms_incl_frame_copy", 48 * W * H

    def vdenoise(W, H, per_pixel=False):
        params = tipe_rt.vdenoise_params(iterations=args.iterations)
        n = args.spp_half
        g = torch.Generator(device=dev).manual_seed(W * 10007 + H + 1)
        lo = torch.tensor([0.0] * 6 + [-1.0] * 3, dtype=torch.float64, device=dev)
        hi = torch.tensor([4.0] * 3 + [1.0] * 6, dtype=torch.float64, device=dev)
        rounds = torch.randint(1, 6, (H, W), generator=g, device=dev).to(torch.int32)
        count = (n * 2.0 ** (rounds - 1).to(torch.float64))[..., None] if per_pixel else n
        acc = [(lo + (hi - lo) * torch.rand((H, W, 9), generator=g, device=dev, dtype=torch.float64)) * count
               for _ in range(2)]
        nbytes = tipe_rt.lib().rt_vdenoise_workspace_bytes(W, H)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        canva = torch.zeros((H, W, 3), dtype=torch.float64, device=dev)

        def call():
            if per_pixel:
                tipe_rt.vdenoise_adaptive_async(W, H, acc[0].data_ptr(), acc[1].data_ptr(), rounds.data_ptr(), n,
                                                params, ws.data_ptr(), nbytes, canva.data_ptr(), stream=stream)
            else:
                tipe_rt.vdenoise_async(W, H, acc[0].data_ptr(), acc[1].data_ptr(), n, params, ws.data_ptr(), nbytes,
                                       canva.data_ptr(), stream=stream)

        return call, canva, "call_ms", 68 * W * H

    def vdenoise_px(W, H):
        return vdenoise(W, H, per_pixel=True)

    filters = {"atrous": [atrous], "vdenoise": [vdenoise], "vdenoise_px": [vdenoise_px], "both": [atrous, vdenoise],
               "vpair": [vdenoise, vdenoise_px]}[args.filter]
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        made = [(f.__name__,) + f(W, H) for f in filters]
        for _, call, _, _, _ in made:
            for _ in range(args.warmup):
                call()
        torch.cuda.synchronize()
        for rnd in range(args.rounds):
            for name, call, canva, key, nbytes_pass in made:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.reps):
                    call()
                t1.record()
                torch.cuda.synchronize()
                ms = t0.elapsed_time(t1) / args.reps
                digest = hashlib.sha1(canva.cpu().numpy().tobytes()).hexdigest()
                print(json.dumps({"label": args.label, "filter": name, "round": rnd, "W": W, "H": H,
                                  "iterations": args.iterations, "reps": args.reps, key: round(ms, 4),
                                  "pass_compulsory_bytes": nbytes_pass, "canva_sha1": digest}), flush=True)


if __name__ == "__main__":
    main()
