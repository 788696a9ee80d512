#!/usr/bin/env python3
"""Per-pass kernel times of the built-in denoisers from a rocprofv3 kernel trace.

    tools/denoise_trace_summary.py KERNEL_TRACE.csv [--sizes 1200x900,3840x2880] [--skip 3] [--filter atrous|vdenoise|vdenoise_px]

Reads the dispatches of a `rocprofv3 --kernel-trace` run of
tools/denoise_bench.py.  A denoise call is prepare, one pass kernel per
iteration, finish; the frame of a call is recognised by the grid of its first
pass (ceil(W/64) * ceil(H/4) blocks).  A call of the variance-guided filter
(--filter vdenoise: the vdenoise_* kernels) has the variance blur (lum) in
front of each pass kernel; it is reported next to its pass.  --filter
vdenoise_px takes the calls of rt_vdenoise_adaptive_async instead (prepare and
finish are the <const int*, int> instantiations of their kernels, the uniform
forms <double>), --filter vdenoise those of rt_vdenoise_async.  The first --skip
calls of each size are warm-up.  Prints, per size and pass, the median and
minimum kernel time and the compulsory-traffic rate (48 B/pixel for the
a-trous pass, 68 B/pixel for the variance-guided pass with its blur) / median
against the 6.3 TB/s an MI355X streams at most (8 TB/s HBM3E spec)."""
import argparse
import csv
import json
import statistics

HBM_ACHIEVABLE = 6.3e12
# vdenoise_prepare_kernel's per-pixel instantiation, as a trace names it demangled or mangled
PREPARE_PX = ("prepare_kernel<int const", "prepare_kernel<const int", "prepare_kernelIJrPKi")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--sizes", default="1200x900,3840x2880")
    ap.add_argument("--skip", type=int, default=3)
    ap.add_argument("--filter", choices=("atrous", "vdenoise", "vdenoise_px"), default="atrous")
    args = ap.parse_args()
    vd, px = args.filter != "atrous", args.filter == "vdenoise_px"
    pass_bytes = 68.0 if vd else 48.0
    sizes = {}
    for s in args.sizes.split(","):
        W, H = (int(v) for v in s.split("x"))
        sizes[((W + 63) // 64) * ((H + 3) // 4)] = (W, H)
    rows = [r for r in csv.DictReader(open(args.trace))
            if "denoise_" in r["Kernel_Name"] and ("vdenoise_" in r["Kernel_Name"]) == vd]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        short = ("prepare" if "prepare" in name else "finish" if "finish" in name else
                 "lum" if "_lum_" in name else "tiled" if "tiled" in name else "plain")
        if short == "prepare" and any(p in name for p in PREPARE_PX) != px:
            cur = None                           # the other form's call
        elif short == "prepare":
            cur = {"prepare": us, "passes": [], "lum": [], "grid0": None, "t0": int(r["Start_Timestamp"])}
        elif cur is not None and short == "finish":
            cur["finish"] = us
            cur["span"] = (int(r["End_Timestamp"]) - cur["t0"]) / 1e3
            calls.append(cur)
            cur = None
        elif cur is not None and short == "lum":
            cur["lum"].append(us)
        elif cur is not None:
            if cur["grid0"] is None:
                threads = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
                cur["grid0"] = threads // (int(r["Workgroup_Size_X"]) * int(r["Workgroup_Size_Y"]) *
                                           int(r["Workgroup_Size_Z"]))
            cur["passes"].append((short, us, int(r["Scratch_Size"])))
    for grid0, (W, H) in sizes.items():
        mine = [c for c in calls if c["grid0"] == grid0][args.skip:]
        if not mine:
            continue
        out = {"filter": args.filter, "W": W, "H": H, "calls": len(mine),
               "prepare_us": round(statistics.median(c["prepare"] for c in mine), 2),
               "finish_us": round(statistics.median(c["finish"] for c in mine), 2),
               "call_span_us": round(statistics.median(c["span"] for c in mine), 2), "passes": []}
        for i in range(len(mine[0]["passes"])):
            us = [c["passes"][i][1] for c in mine]
            med = statistics.median(us)
            kind, _, scratch = mine[0]["passes"][i]
            row = {"step": 1 << i, "kernel": kind, "median_us": round(med, 2), "min_us": round(min(us), 2),
                   "scratch": scratch}
            if vd:
                lum = statistics.median(c["lum"][i] for c in mine)
                row["lum_median_us"] = round(lum, 2)
                med += lum
            rate = pass_bytes * W * H / (med * 1e-6)
            row.update({"compulsory_TBps": round(rate / 1e12, 3), "share_of_6.3TBps": round(rate / HBM_ACHIEVABLE, 3)})
            out["passes"].append(row)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
