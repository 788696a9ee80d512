"""The whole-frame entry points into host arrays -- rt_render_vdenoised,
rt_render_adaptive, rt_render_adaptive_vdenoised, rt_denoise_host -- which
share one job on the host side (rt_host_slots.h HostFrameJob: pooled stream,
pinned staging, one carved device buffer, copies out only on success).

Each is compared bit for bit with the same result built from the async entry
points on caller-owned torch buffers (the support modules' drivers), on the
Cornell spheres at 3 bounces.  The frame sizes run 8x6, 33x17, 8x6 in one
process: the pooled stream's staging first has to grow and is then larger than
needed, and 33x17 is no multiple of anything the kernels tile by."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers
import tipe_rt
from adaptive_support import accumulate_dense, device_adaptive, u64
from denoise_support import device_denoise
from tipe_rt import types as T
from vdenoise_adaptive_support import device_filter
from vdenoise_support import device_vdenoise

pytestmark = pytest.mark.gpu

SIZES = [(8, 6), (33, 17), (8, 6)]
BOUNCES, SPP = 3, 4
SENTINEL = -7.0


def adaptive():
    return tipe_rt.adaptive_params(first_half=2, max_rounds=2, tolerance=1.0 / 64.0)


@functools.lru_cache(maxsize=None)
def bundle():
    return helpers.cornell()


def params(W, H, spp):
    return helpers.params(W, H, spp, BOUNCES)


@functools.lru_cache(maxsize=None)
def reference(W, H):
    """What the async entry points give on torch buffers; computed once per size and never written."""
    ds = tipe_rt.DeviceScene(bundle().scene, 0)
    try:
        half, zero = params(W, H, SPP // 2), np.zeros((H, W, 9))
        A, B = (accumulate_dense(ds, half, [k * (SPP // 2)], zero) for k in (0, 1))
        vdenoised = device_vdenoise(A, B, SPP // 2)
        aA, aB, rounds, planes = device_adaptive(ds, params(W, H, 1), adaptive())
        filtered = device_filter(aA, aB, rounds, adaptive().first_half)[0]
    finally:
        ds.close()
    frame = planes[:3]                               # a rendered canva, albedo, normal for the a-trous filter
    return dict(vdenoised=[vdenoised[k] for k in ("canva", "albedo", "normal")], adaptive=frame, rounds=rounds,
                filtered=[filtered[k] for k in ("canva", "albedo", "normal")], frame=frame,
                denoised=device_denoise(*frame)[1])


def same(got, want, what):
    assert got.shape == want.shape and (u64(got) == u64(want)).all(), what


def check_size(W, H, albedo=True, normal=True):
    """Every host entry point at W x H against the reference; planes not asked for come back as None."""
    ref, scene, kw = reference(W, H), bundle().scene, dict(albedo=albedo, normal=normal)
    asked = (True, albedo, normal)
    for name, got, want in (("rt_render_vdenoised", tipe_rt.render_vdenoised(scene, params(W, H, SPP), **kw),
                             ref["vdenoised"]),
                            ("rt_render_adaptive", tipe_rt.render_adaptive(scene, params(W, H, 1), adaptive(), **kw),
                             ref["adaptive"]),
                            ("rt_render_adaptive_vdenoised",
                             tipe_rt.render_adaptive_vdenoised(scene, params(W, H, 1), adaptive(), **kw),
                             ref["filtered"])):
        for k in range(3):
            if asked[k]:
                same(got[k], want[k], "%s %dx%d plane %d" % (name, W, H, k))
            else:
                assert got[k] is None, name
        if len(got) == 4:
            assert got[3].dtype == np.int32 and (got[3] == ref["rounds"]).all(), name
    same(tipe_rt.denoise(*ref["frame"]), ref["denoised"], "rt_denoise_host %dx%d" % (W, H))


def test_host_frames_equal_the_async_entry_points_as_the_staging_grows_and_shrinks():
    tipe_rt.lib().rt_shutdown()          # the pooled streams go: the first size starts from no staging at all
    for W, H in SIZES:
        check_size(W, H)


def test_planes_not_asked_for_change_nothing():
    check_size(33, 17, albedo=False, normal=False)


def test_a_refused_call_writes_nothing_and_the_next_good_call_is_unchanged():
    W, H = 33, 17
    check_size(W, H)
    L, scene = tipe_rt.lib(), bundle().scene
    planes = [np.full((H, W, 3), SENTINEL) for _ in range(3)]
    rounds = np.full((H, W), int(SENTINEL), dtype=np.int32)
    ptr = [a.ctypes.data for a in planes]
    p, ap, vp, dp = params(W, H, SPP), adaptive(), tipe_rt.vdenoise_params(), tipe_rt.denoise_params()
    bad = tipe_rt.adaptive_params(first_half=0, max_rounds=2, tolerance=1.0 / 64.0)
    refused = [
        L.rt_render_adaptive(C.byref(scene), C.byref(p), C.byref(bad), *ptr, rounds.ctypes.data),
        L.rt_render_adaptive_vdenoised(C.byref(scene), C.byref(p), C.byref(bad), C.byref(vp), *ptr, rounds.ctypes.data),
        L.rt_render_adaptive(C.byref(scene), C.byref(p), C.byref(ap), None, ptr[1], ptr[2], rounds.ctypes.data),
        L.rt_render_adaptive_vdenoised(C.byref(scene), C.byref(p), C.byref(ap), C.byref(vp), None, ptr[1], ptr[2],
                                       rounds.ctypes.data),
        L.rt_render_vdenoised(C.byref(scene), C.byref(p), C.byref(vp), None, ptr[1], ptr[2]),
        L.rt_denoise_host(W, H, None, ptr[1], ptr[2], C.byref(dp)),
    ]
    assert refused == [T.RT_EINVAL] * len(refused), refused
    assert all((a == SENTINEL).all() for a in planes) and (rounds == int(SENTINEL)).all()
    check_size(W, H)
