#!/usr/bin/env python3
"""Timings for the packed canva transport (profiles/packed_canva/README.md).

    tools/packed_canva_bench.py dropin [--spp 16 64 1000] [--reps 10]
        rt_render_rows of the C2 frame (README box, 1200x900, 6 bounces,
        spp_chunks AUTO) into host arrays, host clock around the synchronous
        call, with rt_set_fill_packed_canva off and (where the library has it)
        on.  RT_HIP_LIB selects the library, so a parent build can be timed
        by the same script.
    tools/packed_canva_bench.py gather [--size 3840 2880] [--slots 8] [--reps 10]
        rt_render_gather_async over `slots` slots of device 0 with peer copies,
        canva only, 1 spp and no bounces, flag off and on: HIP events on the
        destination stream around the call (the slots' 1-spp renders are
        inside the interval; `render_ms` is a single-device 1-spp render of the
        same frame for scale).
    tools/packed_canva_bench.py trace [--size 3840 2880] [--slots 8]
        three gathers of each kind and nothing else: the workload for a
        `rocprofv3 --kernel-trace --stats` run.

One JSON line per case; every repetition is in it.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tipe-raytracer_amd"))
import torch  # noqa: E402,F401  (share torch's HIP runtime)

import tipe_rt  # noqa: E402
from tipe_rt import scenes  # noqa: E402

PACKED = 0x100      # RT_GATHER_PACKED_CANVA


def c2(W, H, spp, bounces=6):
    cam = tipe_rt.init_camera(**{k: scenes.README_CAMERA[k] for k in ("origin", "target", "up", "vfov", "ratio")})
    scene = tipe_rt.make_scene(scenes.cornell_spheres())
    return scene, tipe_rt.make_params(W, H, spp, bounces, cam, focus=3.0, seed=1010, chunks=tipe_rt.RT_SPP_CHUNKS_AUTO)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "reps_ms": [round(x, 3) for x in ms]}


def dropin(args):
    lib = tipe_rt.lib()
    has = hasattr(lib, "rt_set_fill_packed_canva")
    W, H = 1200, 900
    for spp in args.spp:
        scene, p = c2(W, H, spp)
        for on in ([False, True] if has else [False]):
            if has:
                tipe_rt.set_fill_packed_canva(on)
            for _ in range(2):
                canva, _, _ = tipe_rt.render_rows(scene, p)
            ms = []
            for _ in range(args.reps):
                t = time.perf_counter()
                canva, alb, nrm = tipe_rt.render_rows(scene, p)
                ms.append((time.perf_counter() - t) * 1e3)
            out = {"case": "rt_render_rows", "lib": os.path.basename(os.path.dirname(tipe_rt.LIB_PATH)) + "/" +
                   os.path.basename(tipe_rt.LIB_PATH), "spp": spp, "packed": on, "canva_sum": float(canva.sum())}
            out.update(summary(ms))
            out["msamples_per_s"] = round(W * H * spp / out["median_ms"] / 1e3, 1)
            print(json.dumps(out), flush=True)
    if has:
        tipe_rt.set_fill_packed_canva(False)


def gather_once(scene, p, out, st):
    tipe_rt.render_gather_async(scene, p, 1, out.data_ptr(), stream=st.cuda_stream)


def gather(args, trace=False):
    lib = tipe_rt.lib()
    W, H = args.size
    G = args.slots
    scene, p = c2(W, H, 1, bounces=0)
    st = torch.cuda.Stream()
    out = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    ds = tipe_rt.DeviceScene(scene, 0)
    render_ms = []
    for _ in range(2 if trace else 5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            e0.record(st)
            tipe_rt.render_async(ds, p, tipe_rt.band_tiling(0, H - 1), out.data_ptr(), stream=st.cuda_stream)
            e1.record(st)
        st.synchronize()
        render_ms.append(e0.elapsed_time(e1))
    ds.close()
    with torch.cuda.stream(st):
        ref = out.clone()
    st.synchronize()
    tipe_rt.check(lib.rt_init(G, (C.c_int * G)(*([0] * G))))
    rows_pr = (H + G - 1) // G
    try:
        for flag in (0, PACKED):
            p.gather = 1 | flag      # RT_GATHER_PEER
            ms = []
            for rep in range(3 if trace else args.reps + 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(st):
                    out.fill_(-1.0)
                    e0.record(st)
                    gather_once(scene, p, out, st)
                    e1.record(st)
                st.synchronize()
                if rep >= 2:
                    ms.append(e0.elapsed_time(e1))
            assert torch.equal(out, ref), "the gathered frame differs from one device's"
            if trace:
                continue
            res = {"case": "rt_render_gather_async, peer, canva only, 1 spp", "size": [W, H], "slots": G,
                   "packed": bool(flag), "transport": tipe_rt.last_gather_transport(),
                   "canva_bytes_copied": G * rows_pr * W * (4 if flag else 24),
                   "render_ms_one_device": round(statistics.median(render_ms), 3)}
            res.update(summary(ms))
            print(json.dumps(res), flush=True)
    finally:
        lib.rt_shutdown()
        tipe_rt.check(lib.rt_init(0, None))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["dropin", "gather", "trace"])
    ap.add_argument("--spp", type=int, nargs="+", default=[16, 64, 1000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", type=int, nargs=2, default=[3840, 2880])
    ap.add_argument("--slots", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: there is no CPU fallback")
    if args.mode == "dropin":
        dropin(args)
    else:
        gather(args, trace=args.mode == "trace")


if __name__ == "__main__":
    main()
