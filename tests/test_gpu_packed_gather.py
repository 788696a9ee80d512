"""The packed canva where a frame leaves a device (rt.h "packed canva
transport"): rt_render_gather_async with RT_GATHER_PACKED_CANVA over peer
copies and over RCCL, rt_assemble_packed_async on a crafted frame that holds
the NaN marker, and the host-buffer drop-ins with rt_set_fill_packed_canva.
Every result must equal the unpacked path's bit for bit (uint64 views).
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import helpers
import tipe_rt
from gpu_driver import PLANES, device_planes, gpu_render
from packed_canva_support import MARKER, np_pack, same_bits
from tipe_rt.types import RT_GATHER_PACKED_CANVA, RT_GATHER_PEER, RT_GATHER_RCCL, Sphere, ThreadData

pytestmark = pytest.mark.gpu

SUFFIX = ", canva 4 B/px"


# ---- rt_render_gather_async -----------------------------------------------------

def gather_params(W, H):
    return helpers.params(W, H, 4, 4, chunks=2)


@functools.lru_cache(maxsize=None)
def one_device_frame(W, H):
    """The frame of a single rt_render_async launch: what every gather must equal."""
    return gpu_render(helpers.cornell(), gather_params(W, H))


def gathered_frame(W, H, tile_rows, gather, nplanes):
    import torch
    p = gather_params(W, H)
    p.gather = gather
    planes = device_planes(H, W, fill=-3.0)
    ptrs = [planes[k].data_ptr() if k < nplanes else None for k in range(4)]
    tipe_rt.render_gather_async(helpers.cornell().scene, p, tile_rows, *ptrs,
                                stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in planes], tipe_rt.last_gather_transport()


@pytest.mark.parametrize("nplanes", [1, 4])
@pytest.mark.parametrize("transport,slots,W,H,tile_rows", [
    (RT_GATHER_PEER, 3, 5, 7, 2),       # 4 tiles on 3 slots: H not divisible, every slot has padding rows
    (RT_GATHER_PEER, 8, 33, 9, 2),      # 5 tiles on 8 slots: three slots hold padding only
    (RT_GATHER_RCCL, 1, 5, 7, 2),       # the real library, one rank
    (RT_GATHER_RCCL, 1, 33, 9, 2)])
def test_gather_flag_on_equals_flag_off(transport, slots, W, H, tile_rows, nplanes):
    lib = tipe_rt.lib()
    tipe_rt.check(lib.rt_init(slots, (C.c_int * slots)(*([0] * slots))))
    try:
        ref = one_device_frame(W, H)
        off, tr_off = gathered_frame(W, H, tile_rows, transport, nplanes)
        on, tr_on = gathered_frame(W, H, tile_rows, transport | RT_GATHER_PACKED_CANVA, nplanes)
        for k in range(4):
            if k < nplanes:
                same_bits(off[k], ref[k])
                same_bits(on[k], off[k])
            else:
                assert (on[k] == -3.0).all() and (off[k] == -3.0).all(), PLANES[k] + " was not requested"
        assert tr_off.startswith("rccl: ncclGather" if transport == RT_GATHER_RCCL else "peer:")
        assert not tr_off.endswith(SUFFIX) and SUFFIX not in tr_off
        assert tr_on == tr_off + SUFFIX
    finally:
        lib.rt_shutdown()
        tipe_rt.check(lib.rt_init(0, None))


# ---- a frame with NaN radiance channels, crafted ----------------------------------

def rank_major(full, world, tile_rows, rows_per_rank, pad):
    """The per-rank local planes of a frame (rt.h rt_tiling), padding rows set to `pad`."""
    H, W = full.shape[:2]
    loc = np.full((world, rows_per_rank, W, 3), pad)
    for g in range(H):
        t, y = divmod(g, tile_rows)
        loc[t % world, t // world * tile_rows + y] = full[g]
    return loc


@pytest.mark.parametrize("stride_pad", [0, 3])
def test_marker_arrives_intact_through_the_packed_assemble(stride_pad):
    """A canva whose pixels hold -2147483648.0 (a NaN radiance channel, as
    write_color_canva stores it) in one, two and three channels: packed on
    the device from the slots' local planes, then un-permuted and widened."""
    import torch
    W, H, world, tile_rows = 5, 7, 3, 2
    rows_pr = 4
    rng = np.random.default_rng(5)
    full = rng.integers(0, 256, (H, W, 3)).astype(np.float64)
    full[0, 0] = MARKER
    full[6, 4, 1] = MARKER
    full[3, 2, 0] = full[3, 2, 2] = MARKER
    full[2, :, 2] = MARKER
    loc = rank_major(full, world, tile_rows, rows_pr, 77.0)
    n = rows_pr * W
    stride = n + stride_pad
    st = torch.cuda.Stream()
    d_loc = torch.from_numpy(loc).to("cuda:0")
    words = torch.full((world * stride,), 0x1ff, dtype=torch.int32, device="cuda:0")
    out, = device_planes(H + 1, W, n=1, fill=-9.0)                 # one guard row behind the frame
    with torch.cuda.stream(st):
        for r in range(world):
            tipe_rt.canva_pack_async(n, d_loc[r].data_ptr(), words[r * stride:].data_ptr(), st.cuda_stream)
        tipe_rt.assemble_packed_async(words.data_ptr(), world, tile_rows, rows_pr, W, H, out.data_ptr(),
                                      st.cuda_stream, rank_stride=stride if stride_pad else 0)
    st.synchronize()
    w = words.cpu().numpy().view(np.uint32).reshape(world, stride)
    assert (w[:, :n] == np_pack(loc.reshape(world, n, 3))).all()
    assert (w[:, n:] == 0x1ff).all()
    got = out.cpu().numpy()
    same_bits(got[:H], full)
    assert (got[H] == -9.0).all(), "the assemble wrote behind the frame"
    assert (got[:H] == MARKER).sum() == 3 + 1 + 2 + W


# ---- host-buffer drop-ins -----------------------------------------------------------

DROP_W, DROP_H = 64, 48
BANDS = [(47, 36), (35, 24), (23, 12), (11, 0)]


def drop_bundle(scene):
    return helpers.cornell() if scene == "cornell" else helpers.pyramid_scene()


def drop_params():
    return helpers.params(DROP_W, DROP_H, 4, 5, chunks=tipe_rt.RT_SPP_CHUNKS_AUTO, compat=0)


def fill_canva_frame(bundle):
    """rt_fill_canva over BANDS from one thread each, main.c's ThreadData."""
    W, H = DROP_W, DROP_H
    p = drop_params()
    planes = [np.full((H, W, 3), -7.0) for _ in range(3)]
    tds = []
    for hi, lo in BANDS:
        td = ThreadData()
        td.start_row, td.end_row = hi, lo
        td.canva, td.albedo_tab, td.normal_tab = (C.cast(a.ctypes.data, C.POINTER(tipe_rt.Vec3)) for a in planes)
        td.cam = p.cam
        td.largeur_image, td.hauteur_image = W, H
        td.nbRayonParPixel, td.nbRebondMax = p.nbRayonParPixel, p.nbRebondMax
        td.total_pixels = W * H
        td.sphere_list = C.cast(bundle.spheres, C.POINTER(Sphere))
        td.nbSpheres = len(bundle.spheres)
        sc = bundle.scene
        td.triangle_list, td.nbTriangles, td.quelMatPourTri = sc.triangle_list, sc.nbTriangles, sc.quelMatPourTri
        td.mat_list, td.tex_width, td.tex_height = sc.mat_list, sc.tex_width, sc.tex_height
        td.focus_distance = 3
        tds.append(td)
    res = []
    ths = [threading.Thread(target=lambda t=t: res.append(tipe_rt.lib().rt_fill_canva(C.byref(t)))) for t in tds]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert all(r is None for r in res), tipe_rt.lib().rt_last_error()
    return planes


def band_frame(bundle, hi, lo):
    planes = [np.full((DROP_H, DROP_W, 3), -7.0) for _ in range(3)]
    p = drop_params()
    tipe_rt.check(tipe_rt.lib().rt_render_rows(C.byref(bundle.scene), C.byref(p), hi, lo,
                                               *[a.ctypes.data for a in planes]))
    return planes


@functools.lru_cache(maxsize=None)
def drop_in_results(scene, packed):
    """(rt_render_rows whole frame, rt_fill_canva from 4 threads, rt_render_rows
    on rows 9..20) with the switch as given; the switch is off again afterwards."""
    bundle = drop_bundle(scene)
    prev = tipe_rt.set_fill_packed_canva(packed)
    try:
        assert prev is False
        return (tipe_rt.render_rows(bundle.scene, drop_params()), fill_canva_frame(bundle),
                band_frame(bundle, 20, 9))
    finally:
        tipe_rt.set_fill_packed_canva(False)


@pytest.mark.parametrize("scene", ["cornell", "pyramid"])
def test_drop_ins_switch_on_equals_switch_off(scene):
    off_rows, off_fill, off_band = drop_in_results(scene, False)
    on_rows, on_fill, on_band = drop_in_results(scene, True)
    ref = helpers.oracle_render(drop_bundle(scene), drop_params())
    for k in range(3):
        same_bits(off_rows[k], ref[PLANES[k]])            # the switch-off frame is the oracle's
        same_bits(on_rows[k], off_rows[k])
        same_bits(on_fill[k], off_fill[k])
        same_bits(off_fill[k], off_rows[k])
        same_bits(on_band[k], off_band[k])
        # only the named rows are written
        outside = np.ones(DROP_H, bool)
        outside[9:21] = False
        assert (on_band[k][outside] == -7.0).all()
        same_bits(on_band[k][9:21], off_rows[k][9:21])
    assert on_rows[0].max() > 0 and set(np.unique(on_rows[0])) <= set(np.arange(256.0))
