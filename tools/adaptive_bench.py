#!/usr/bin/env python3
"""Time adaptive sampling (rt_adaptive_async) against uniform renders of the same scene.

    tools/adaptive_bench.py [--scenes box,nature] [--size 1200x900] [--reps 5] [--warmup 1] [--label TAG]
                            [--first-half 8] [--max-rounds 5] [--tolerance 0.015625] [--no-rounds]
                            [--queue off|on|both] [--ceiling SPP]

Per scene, JSON lines (device-event times, every repetition listed so the spread shows):
  adaptive        rt_adaptive_async at the given parameters (A, B, d_rounds and the frame planes), its total
                  samples, the mean per pixel and the share of pixels per round count;
  adaptive_vdenoised   rt_adaptive_async with frame = NULL followed by rt_vdenoise_adaptive_async at its defaults
                  on the same stream (rt_render_adaptive_vdenoised's device work);
  uniform_vdenoised    rt_render_vdenoised's device composition (two rt_accumulate_async calls +
                  rt_vdenoise_async) at the even count nearest the adaptive frame's mean;
  uniform_max     two rt_accumulate_async calls + rt_resolve_async at the adaptive schedule's maximum count;
  uniform_mean    the same at the even count nearest the adaptive frame's mean;
  round           for each round, host-driven through the public calls (accumulate, select, one read of the
                  count): the list size and, for rounds >= 1, the list kernel's samples per second next to the
                  dense fixed-grid kernel's on the same batch size over the whole frame (rt_accumulate_async:
                  the parent's code, the yardstick); round 0 also times the list kernel on a list of every
                  pixel, which separates the cost of the entry map from that of the pixels a list keeps.
--queue: rt_set_accumulate_queue's setting for every timed call (default off; a library without the switch
runs off only).  With "both" each repetition of a case runs once off and once on, alternating, and the case
prints one line per setting ("queue": 0 / 1), so the two share the device's state.  What the accumulators hold
is the same either way.
--ceiling SPP adds two lines per scene: ceiling_accumulate, SPP samples as two rt_accumulate_async halves, and
ceiling_render, rt_render_async at SPP (always the task-queue kernel: what an accumulate launch can reach).
The box is the README scene (spheres only), nature the reference's RTX_MAP/nature mesh under its own camera."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tipe-raytracer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="box,nature")
    ap.add_argument("--size", default="1200x900")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--label", default="")
    ap.add_argument("--first-half", type=int, default=None)
    ap.add_argument("--max-rounds", type=int, default=None)
    ap.add_argument("--tolerance", type=float, default=None)
    ap.add_argument("--no-rounds", action="store_true", help="skip the round-by-round lines")
    ap.add_argument("--queue", choices=["off", "on", "both"], default="off")
    ap.add_argument("--ceiling", type=int, default=0, help="SPP of the ceiling_accumulate / ceiling_render lines")
    args = ap.parse_args()
    import torch
    import tipe_rt
    from tipe_rt import scenes
    if not torch.cuda.is_available():
        sys.exit("adaptive_bench: needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    W, H = (int(v) for v in args.size.split("x"))
    npx = W * H
    adp = tipe_rt.adaptive_params(first_half=args.first_half, max_rounds=args.max_rounds, tolerance=args.tolerance)
    fh, R = adp.first_half, adp.max_rounds
    band = tipe_rt.band_tiling(0, H - 1)
    has_switch = hasattr(tipe_rt.lib(), "rt_set_accumulate_queue")
    if args.queue != "off" and not has_switch:
        sys.exit("adaptive_bench: this library has no rt_set_accumulate_queue")
    settings = {"off": [0], "on": [1], "both": [0, 1]}[args.queue]

    def set_queue(q):
        if has_switch:
            tipe_rt.set_accumulate_queue(bool(q))

    def timed(call, reps=args.reps, warmup=args.warmup):
        """{setting: milliseconds of each repetition}; the settings alternate within a repetition."""
        for _ in range(warmup):
            for q in settings:
                set_queue(q)
                call()
        torch.cuda.synchronize()
        out = {q: [] for q in settings}
        for _ in range(reps):
            for q in settings:
                set_queue(q)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call()
                t1.record()
                torch.cuda.synchronize()
                out[q].append(round(t0.elapsed_time(t1), 3))
        set_queue(0)
        return out

    def emit(**kw):
        print(json.dumps(dict(label=args.label, W=W, H=H, first_half=fh, max_rounds=R,
                              tolerance=float(adp.tolerance), **kw)), flush=True)

    def emit_each(ms, **kw):
        """One line per setting of a timed() result."""
        for q in settings:
            emit(queue=q, ms=ms[q], **kw)

    def rate(n, ms):
        return round(n / (float(np.median(ms)) * 1e-3) / 1e6, 1) if n else None

    for name in args.scenes.split(","):
        if name == "nature":
            tris, qm, mats, tw, th, nm = scenes.nature_mesh()
            scene = tipe_rt.make_scene(scenes.main_spheres(), tris, qm, mats, tw, th, nm)
            spec, bounces = scenes.NATURE_CAMERA, 10
        else:
            scene = tipe_rt.make_scene(scenes.cornell_spheres())
            spec, bounces = scenes.README_CAMERA, 6
        cam = tipe_rt.init_camera(**{k: spec[k] for k in ("origin", "target", "up", "vfov", "ratio")})
        p = tipe_rt.make_params(W, H, 1, bounces, cam, focus=3.0, chunks=tipe_rt.RT_SPP_CHUNKS_AUTO)
        ds = tipe_rt.DeviceScene(scene, 0)
        acc = torch.zeros((2, H, W, 9), dtype=torch.float64, device=dev)
        rounds = torch.zeros((H, W), dtype=torch.int32, device=dev)
        planes = torch.zeros((3, H, W, 3), dtype=torch.float64, device=dev)
        nbytes = tipe_rt.lib().rt_adaptive_workspace_bytes(W, H)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

        def with_spp(n):
            q = type(p).from_buffer_copy(p)
            q.nbRayonParPixel = n
            return q

        def adaptive():
            tipe_rt.adaptive_async(ds, p, adp, acc[0].data_ptr(), acc[1].data_ptr(), rounds.data_ptr(), ws.data_ptr(),
                                   nbytes, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), stream=st)

        ms = timed(adaptive)
        k = rounds.cpu().numpy()
        counts = 2.0 * fh * 2.0 ** (k - 1)
        mean = float(counts.mean())
        emit_each(ms, scene=name, what="adaptive", bounces=bounces, total_samples=float(counts.sum()),
                  mean_spp=round(mean, 3), share_per_round=[round(float((k == r).mean()), 4) for r in range(1, R + 1)])

        def uniform(half):
            def call():
                acc.zero_()
                for j in range(2):
                    tipe_rt.accumulate_async(ds, with_spp(half), j * half, band, acc[j].data_ptr(), st)
                acc[0].add_(acc[1])
                tipe_rt.resolve_async(acc[0].data_ptr(), p, 2 * half, band, planes[0].data_ptr(), planes[1].data_ptr(),
                                      planes[2].data_ptr(), stream=st)
            return call

        half_max = fh << (R - 1)
        half_mean = max(1, int(round(mean / 2.0)))

        vdp = tipe_rt.vdenoise_params()
        vbytes = tipe_rt.lib().rt_vdenoise_workspace_bytes(W, H)
        vws = torch.empty(vbytes, dtype=torch.uint8, device=dev)

        def adaptive_vdenoised():
            tipe_rt.adaptive_async(ds, p, adp, acc[0].data_ptr(), acc[1].data_ptr(), rounds.data_ptr(), ws.data_ptr(),
                                   nbytes, stream=st)
            tipe_rt.vdenoise_adaptive_async(W, H, acc[0].data_ptr(), acc[1].data_ptr(), rounds.data_ptr(), fh, vdp,
                                            vws.data_ptr(), vbytes, planes[0].data_ptr(), planes[1].data_ptr(),
                                            planes[2].data_ptr(), stream=st)

        def uniform_vdenoised():
            acc.zero_()
            for j in range(2):
                tipe_rt.accumulate_async(ds, with_spp(half_mean), j * half_mean, band, acc[j].data_ptr(), st)
            tipe_rt.vdenoise_async(W, H, acc[0].data_ptr(), acc[1].data_ptr(), half_mean, vdp, vws.data_ptr(), vbytes,
                                   planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), stream=st)

        emit_each(timed(adaptive_vdenoised), scene=name, what="adaptive_vdenoised", mean_spp=round(mean, 3),
                  iterations=vdp.iterations)
        emit_each(timed(uniform_vdenoised), scene=name, what="uniform_vdenoised", spp=2 * half_mean,
                  iterations=vdp.iterations)
        emit_each(timed(uniform(half_max)), scene=name, what="uniform_max", spp=2 * half_max,
                  total_samples=2.0 * half_max * npx)
        emit_each(timed(uniform(half_mean)), scene=name, what="uniform_mean", spp=2 * half_mean,
                  total_samples=2.0 * half_mean * npx)
        if args.ceiling:
            half_c = args.ceiling // 2

            def ceiling_accumulate():
                for j in range(2):
                    tipe_rt.accumulate_async(ds, with_spp(half_c), j * half_c, band, acc[j].data_ptr(), st)

            def ceiling_render():
                tipe_rt.render_async(ds, with_spp(2 * half_c), band, planes[0].data_ptr(), planes[1].data_ptr(),
                                     planes[2].data_ptr(), None, st)

            for what, call in (("ceiling_accumulate", ceiling_accumulate), ("ceiling_render", ceiling_render)):
                ms = timed(call)
                for q in settings:
                    emit(queue=q, ms=ms[q], scene=name, what=what, spp=2 * half_c, bounces=bounces,
                         kernel=tipe_rt.last_render_kernel() if q == settings[-1] else None,
                         msamples_per_s=rate(2.0 * half_c * npx, ms[q]))

        if args.no_rounds:
            ds.close()
            continue
        # round by round through the public calls
        lst = torch.zeros(npx, dtype=torch.int32, device=dev)
        cnt = torch.zeros(4, dtype=torch.int32, device=dev)
        acc.zero_()
        scratch = torch.zeros((H, W, 9), dtype=torch.float64, device=dev)
        n_list = npx
        for r in range(R):
            n_r = fh << r
            b, o = (n_r, 0) if r == 0 else (n_r // 2, n_r)
            pb = with_spp(b)

            def dense():
                tipe_rt.accumulate_async(ds, pb, o, band, scratch.data_ptr(), st)

            dense_ms = timed(dense)
            lines = {q: dict(scene=name, what="round", queue=q, round=r, batch=b, list_size=n_list, dense_ms=dense_ms[q],
                             dense_msamples_per_s=rate(npx * b, dense_ms[q])) for q in settings}
            if r == 0:
                # the list kernel on every pixel against the dense kernel: what the entry map costs by itself
                every = torch.arange(npx, dtype=torch.int32, device=dev)
                n_every = torch.tensor([npx, 0, 0, 0], dtype=torch.int32, device=dev)

                def full_list():
                    tipe_rt.accumulate_list_async(ds, pb, o, every.data_ptr(), n_every.data_ptr(), npx,
                                                  scratch.data_ptr(), st)

                full_ms = timed(full_list)
                for q in settings:
                    lines[q].update(full_list_ms=full_ms[q], full_list_msamples_per_s=rate(npx * b, full_ms[q]))
                for j in range(2):
                    tipe_rt.accumulate_async(ds, pb, o + j * b, band, acc[j].data_ptr(), st)
            else:
                def listed():
                    tipe_rt.accumulate_list_async(ds, pb, o, lst.data_ptr(), cnt.data_ptr(), npx, scratch.data_ptr(),
                                                  st)

                list_ms = timed(listed)
                for q in settings:
                    lines[q].update(list_ms=list_ms[q], list_msamples_per_s=rate(n_list * b, list_ms[q]))
                for j in range(2):
                    tipe_rt.accumulate_list_async(ds, pb, o + j * b, lst.data_ptr(), cnt.data_ptr(), npx,
                                                  acc[j].data_ptr(), st)
            for q in settings:
                emit(**lines[q])
            if r < R - 1:
                tipe_rt.adaptive_select_async(W, H, acc[0].data_ptr(), acc[1].data_ptr(), n_r, float(adp.tolerance), r,
                                              lst.data_ptr(), cnt.data_ptr(), rounds.data_ptr(), ws.data_ptr(), nbytes,
                                              stream=st)
                torch.cuda.synchronize()
                n_list = int(cnt[0])
        ds.close()


if __name__ == "__main__":
    main()
