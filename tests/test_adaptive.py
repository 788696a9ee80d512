"""rt_adaptive_async, rt_resolve_adaptive_async and rt_render_adaptive (rt.h
"adaptive sampling", layer 3) against a host-driven reference: whole-frame
rt_accumulate_async sequences for k = 1..R rounds, the float32 restatement of
the selection pass deciding each pixel's k, pixel p taken from the k-round
accumulators; the frame planes against rt_resolve_async over A + B per round
group; each group's radiance against the CPU oracle at its own sample count."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import tipe_rt
from adaptive_support import device_adaptive, glass_cornell, pick, reference_rounds, schedule, u64
from gpu_driver import device_planes
from tipe_rt import scenes
from tipe_rt import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 40, 30
BOUNCES = 5


def lamp_behind_the_camera():
    """A short box (x, y in [-1, 1], z in [-1.5, 1]) with plain diffuse walls and
    no lamp in it; the wall behind the camera (z = 1) is the lamp.  Every pixel
    sees a diffuse wall whose light arrives by chance, at roughly every second
    sample: noise everywhere, and no 3x3 neighbourhood of all-black samples."""
    wall = scenes.material((0.8, 0.7, 0.6))
    return helpers.SceneBundle(helpers.sphere_array(
        [(c, 500.0, wall) for c in ((-501.0, 0.0, 0.0), (501.0, 0.0, 0.0), (0.0, -501.0, 0.0), (0.0, 501.0, 0.0),
                                    (0.0, 0.0, -501.5))] +
        [((0.0, 0.0, 501.0), 500.0, scenes.material((0.0, 0.0, 0.0), (1.0, 0.9, 0.8), 2.0))]))


def inside_a_lamp():
    """Every sample of every pixel returns the lamp's colour: no variance at all."""
    return helpers.SceneBundle(helpers.sphere_array([
        ((0.0, 0.0, 0.0), 50.0, scenes.material((0.5, 0.5, 0.5), (0.9, 0.8, 0.7), 1.0))]))


def with_spp(p, spp):
    q = type(p).from_buffer_copy(p)
    q.nbRayonParPixel = spp
    return q


def round_accumulators(ds, p, first_half, max_rounds):
    """[(A_k, B_k)] for k = 1..R: the whole frame after k rounds of the schedule, by rt_accumulate_async."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    band = tipe_rt.band_tiling(0, H - 1)
    acc = torch.zeros((2, H, W, 9), dtype=torch.float64, device="cuda:0")
    out = []
    for o, b, n in schedule(first_half, max_rounds):
        for k in range(2):
            tipe_rt.accumulate_async(ds, with_spp(p, b), o + k * b, band, acc[k].data_ptr(), st)
        torch.cuda.synchronize()
        host = acc.cpu().numpy()
        out.append((host[0].copy(), host[1].copy()))
    return out


def reference_planes(per_round, rounds, p, first_half):
    """rt_resolve_async over A_k + B_k with 2 n_(k-1) samples, pixel p from its own k."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    band = tipe_rt.band_tiling(0, H - 1)
    out = [np.empty((H, W, 3)) for _ in range(4)]
    for k in range(1, len(per_round) + 1):
        A, B = per_round[k - 1]
        s = torch.from_numpy(A).to("cuda:0") + torch.from_numpy(B).to("cuda:0")
        planes = device_planes(H, W)
        tipe_rt.resolve_async(s.data_ptr(), p, 2 * (first_half << (k - 1)), band, *[t.data_ptr() for t in planes],
                              stream=st)
        torch.cuda.synchronize()
        for o, t in zip(out, planes):
            o[rounds == k] = t.cpu().numpy()[rounds == k]
    return out


def same_bits(got, want, what):
    bad = u64(got) != u64(want)
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, bad.sum(), bad.size,
                                                                      tuple(np.argwhere(bad)[0]))


def check_against_reference(bundle, first_half, max_rounds, tolerance=None, min_share=0.0, oracle=True, chunks=1):
    """tolerance None: the first of 2^(-e/2), e = 0..24, at which every round
    count 1..R holds at least min_share of the reference's pixels."""
    ds = tipe_rt.DeviceScene(bundle.scene, 0)
    try:
        p = helpers.params(W, H, 999, BOUNCES, chunks=chunks)             # nbRayonParPixel is ignored
        per_round = round_accumulators(ds, p, first_half, max_rounds)
        shares = None
        for tol in ([tolerance] if tolerance is not None else [2.0 ** (-e / 2.0) for e in range(25)]):
            rounds = reference_rounds(per_round, first_half, tol)
            shares = [float((rounds == k).mean()) for k in range(1, max_rounds + 1)]
            print("tolerance %.5f: share of pixels per round count %s" % (tol, ["%.3f" % s for s in shares]))
            if min(shares) >= min_share:
                break
        assert min(shares) >= min_share, "no tolerance spreads the reference's round counts: %r" % (shares,)
        ap = tipe_rt.adaptive_params(first_half=first_half, max_rounds=max_rounds, tolerance=tol)
        A, B, got_rounds, planes = device_adaptive(ds, p, ap)
        assert (got_rounds == rounds).all(), "d_rounds differs at %d pixels" % int((got_rounds != rounds).sum())
        same_bits(A, pick(per_round, rounds, 0), "A")
        same_bits(B, pick(per_round, rounds, 1), "B")
        for name, g, w in zip(("canva", "albedo", "normal", "radiance"), planes,
                              reference_planes(per_round, rounds, p, first_half)):
            same_bits(g, w, name)
        if oracle:
            # the same sample set, re-associated (A's fold + B's fold): test_chunked_batches_are_deterministic's bound
            for k in range(1, max_rounds + 1):
                m = rounds == k
                if not m.any():
                    continue
                ref = helpers.oracle_render(bundle, with_spp(p, 2 * (first_half << (k - 1))), nthreads=8)
                e = helpers.rmse_per_channel(planes[3][m], ref["radiance"][m])
                print("k = %d: %d pixels, radiance RMSE per channel vs the oracle %r" % (k, m.sum(), e))
                assert (e <= 1e-12).all(), (k, e)
        return rounds, A, B, planes
    finally:
        ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene,first_half,max_rounds", [("glass", 2, 4), ("tree", 3, 3)])
def test_loop_equals_the_host_driven_reference(scene, first_half, max_rounds):
    bundle = glass_cornell() if scene == "glass" else helpers.tree_scene()
    check_against_reference(bundle, first_half, max_rounds, min_share=0.05)


@pytest.mark.gpu
def test_loop_with_sample_slices_and_several_entry_bands(monkeypatch):
    """spp_chunks AUTO: P = 4, 4, 8, 16 over the four rounds' batches; bands of
    256 entries, so the rounds' lists (counted on the device) take up to five
    banded launches each.  The reference is rt_accumulate_async with the same
    params, whose slice grouping per batch the list launches must reproduce."""
    monkeypatch.setenv("RT_LIST_BAND", "256")
    check_against_reference(glass_cornell(), 4, 4, min_share=0.05, chunks=T.RT_SPP_CHUNKS_AUTO)


@pytest.mark.gpu
def test_largest_tolerance_on_a_scene_without_variance_is_one_round():
    rounds, _, _, _ = check_against_reference(inside_a_lamp(), 3, 3, tolerance=1.0)
    assert (rounds == 1).all()


@pytest.mark.gpu
def test_smallest_tolerance_on_a_noisy_scene_is_a_uniform_render():
    """Every pixel takes all rounds (asserted on the reference): A + B resolved
    is the uniform render of 2 n_(R-1) samples, the strongest whole-frame check."""
    rounds, _, _, _ = check_against_reference(lamp_behind_the_camera(), 4, 3, tolerance=2.0 ** -12)
    assert (rounds == 3).all()


@pytest.mark.gpu
def test_one_round_only_marks():
    rounds, _, _, _ = check_against_reference(glass_cornell(), 3, 1, tolerance=0.25, oracle=False)
    assert (rounds == 1).all()


@pytest.mark.gpu
def test_host_entry_equals_the_device_path():
    bundle = glass_cornell()
    p = helpers.params(W, H, 1, BOUNCES)
    ap = tipe_rt.adaptive_params(first_half=3, max_rounds=3, tolerance=0.125)
    ds = tipe_rt.DeviceScene(bundle.scene, 0)
    try:
        _, _, rounds, planes = device_adaptive(ds, p, ap)
    finally:
        ds.close()
    canva, alb, nrm, got_rounds = tipe_rt.render_adaptive(bundle.scene, p, ap)
    assert (got_rounds == rounds).all() and len(np.unique(rounds)) > 1
    for name, g, w in zip(("canva", "albedo", "normal"), (canva, alb, nrm), planes):
        same_bits(g, w, name)
    canva2, alb2, nrm2, _ = tipe_rt.render_adaptive(bundle.scene, p, ap, albedo=False, normal=False)
    assert alb2 is None and nrm2 is None
    same_bits(canva2, canva, "canva without the other planes")


# ---- without a device ---------------------------------------------------------------

def bad_adaptive_params():
    ok = dict(first_half=4, max_rounds=3, tolerance=0.1)
    for kw in (dict(first_half=0), dict(first_half=-1), dict(max_rounds=0), dict(max_rounds=17),
               dict(first_half=1 << 20, max_rounds=12),         # 2^32 samples per pixel
               dict(tolerance=math.nan), dict(tolerance=math.inf), dict(tolerance=0.0), dict(tolerance=-0.1),
               dict(tolerance=2.0 ** -13), dict(tolerance=1.5)):
        yield tipe_rt.adaptive_params(**dict(ok, **kw))


def test_validation_fails_before_any_device_work():
    L = tipe_rt.lib()
    fake = 0x10000
    nbytes = L.rt_adaptive_workspace_bytes(8, 6)
    good = tipe_rt.adaptive_params(first_half=4, max_rounds=3, tolerance=0.1)
    frame = T.Frame(fake, fake, fake, fake)

    def run(scene=fake, p=None, ap=good, a=fake, b=fake, rounds=fake, ws=fake, nbytes=nbytes, fr=frame, **kw):
        p = p if p is not None else helpers.params(8, 6, 0, 3, **kw)     # nbRayonParPixel 0: ignored
        return L.rt_adaptive_async(scene, C.byref(p), None if ap is None else C.byref(ap), a, b, rounds, ws, nbytes,
                                   None if fr is None else C.byref(fr), None)

    def refused(rc, code=T.RT_EINVAL):
        assert rc == code, rc
        assert L.rt_last_error()

    for kw in (dict(scene=None), dict(ap=None), dict(a=None), dict(b=None), dict(rounds=None), dict(ws=None),
               dict(nbytes=nbytes - 1), dict(ws=fake + 8), dict(fr=T.Frame(None, fake, fake, fake))):
        refused(run(**kw))
    for ap in bad_adaptive_params():
        refused(run(ap=ap))
    refused(run(semantics=1), T.RT_EUNSUPPORTED)


def test_host_entry_leaves_its_outputs_untouched_on_failure():
    L = tipe_rt.lib()
    bundle = helpers.cornell()
    p = helpers.params(8, 6, 1, 3)
    canva, alb, nrm = (np.full((6, 8, 3), -3.0) for _ in range(3))
    rounds = np.full((6, 8), -3, dtype=np.int32)

    def host(ap, scene=bundle.scene, canva_ptr=canva.ctypes.data, p=p):
        return L.rt_render_adaptive(None if scene is None else C.byref(scene), C.byref(p),
                                    None if ap is None else C.byref(ap), canva_ptr, alb.ctypes.data, nrm.ctypes.data,
                                    rounds.ctypes.data)

    good = tipe_rt.adaptive_params()
    for ap in bad_adaptive_params():
        assert host(ap) == T.RT_EINVAL and L.rt_last_error()
    assert host(None) == T.RT_EINVAL
    assert host(good, scene=None) == T.RT_EINVAL
    assert host(good, canva_ptr=None) == T.RT_EINVAL
    assert host(good, p=helpers.params(8, 6, 1, 3, semantics=1)) == T.RT_EUNSUPPORTED
    assert (canva == -3).all() and (alb == -3).all() and (nrm == -3).all() and (rounds == -3).all()


DENSE_TWIN = {"render_kernel_listILb0ELb0E": "render_kernelILb0ELb0ELb0E",
              "render_kernel_listILb0ELb1E": "render_kernelILb0ELb0ELb1E",
              "render_kernel_listILb1ELb0E": "render_kernelILb0ELb1ELb0E",
              "render_kernel_listILb1ELb1E": "render_kernelILb0ELb1ELb1E",
              "render_kernel_list_wILb0E": "render_kernel_wILb0ELb0E",
              "render_kernel_list_wILb1E": "render_kernel_wILb0ELb1E"}


def test_list_kernels_spill_no_more_than_their_dense_twins():
    """The resource-usage target's lines (the Makefile's own flags): each of the
    six list kernels has at most its dense twin's spilled VGPRs, scratch bytes
    and spilled SGPRs, and its occupancy; the other new kernels use no scratch."""
    mk = ["make", "-C", os.path.join(ROOT, "tipe-raytracer_amd")]
    lines = subprocess.run(mk + ["-n", "-B", "resource-usage"], capture_output=True, text=True, check=True).stdout
    txt = ""
    for src in ("rt_kernels.hip", "rt_adaptive.hip"):
        cmd = [ln for ln in lines.splitlines() if src in ln and "kernel-resource-usage" in ln]
        assert len(cmd) == 1, lines
        out = subprocess.run(cmd[0], shell=True, cwd=os.path.join(ROOT, "tipe-raytracer_amd"), capture_output=True,
                             text=True)
        assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
        txt += out.stdout + out.stderr

    def usage(sym):
        m = re.search(r"Function Name: \S*" + sym + r"\S*.*?ScratchSize \[bytes/lane\]: (\d+).*?"
                      r"Occupancy \[waves/SIMD\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", txt, re.S)
        assert m, sym
        return dict(scratch=int(m.group(1)), occupancy=int(m.group(2)), sgpr_spill=int(m.group(3)),
                    spill=int(m.group(4)))

    for new, twin in DENSE_TWIN.items():
        a, b = usage(new), usage(twin + "EEvNS_7KParamsE")
        print(new, a, "twin", b)
        assert a["spill"] <= b["spill"] and a["scratch"] <= b["scratch"] and a["occupancy"] >= b["occupancy"], (new, a, b)
        assert a["sgpr_spill"] <= b["sgpr_spill"], (new, a, b)
    for name in ("combine_list_kernel", "adaptive_measure_kernel", "adaptive_flag_kernel", "adaptive_scan_kernel",
                 "adaptive_scatter_kernel", "adaptive_mark_kernel", "adaptive_resolve_kernel"):
        u = usage(name)
        assert (u["scratch"], u["spill"]) == (0, 0), (name, u)
