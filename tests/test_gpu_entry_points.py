"""The library's other entry points on the README box, against the oracle:
rt_render_rows on a band of a host buffer, a rank's cyclic row tiles put
together by rt_assemble_async, rt_fill_canva called from pthreads with
main.c's ThreadData, and arguments that must be refused."""
import ctypes as C
import threading

import numpy as np
import pytest

import helpers
import tipe_rt
from tipe_rt.types import ThreadData, Sphere

pytestmark = pytest.mark.gpu


def test_task_queue_kernel_cyclic_tiles():
    """The queue kernel on a rank's cyclic row tiles (multi-GPU layout)."""
    import torch
    bundle = helpers.cornell()
    W, H, k, world = 40, 30, 2, 3
    p = helpers.params(W, H, 8, 5, chunks=4)
    ref = helpers.oracle_render(bundle, p)
    ds = tipe_rt.DeviceScene(bundle.scene, 0)
    stream = torch.cuda.current_stream().cuda_stream
    per_rank = tipe_rt.cyclic_tiling(H, k, 0, world).n_tiles
    gathered = torch.zeros((world, per_rank * k, W, 3), dtype=torch.float64, device="cuda:0")
    for r in range(world):
        t = tipe_rt.cyclic_tiling(H, k, r, world)
        tipe_rt.render_async(ds, p, t, gathered[r].data_ptr(), stream=stream)
    full = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    tipe_rt.assemble_async(gathered.data_ptr(), world, k, per_rank * k, W, H, full.data_ptr(), stream)
    torch.cuda.synchronize()
    ds.close()
    assert (full.cpu().numpy() == ref["canva"]).all()


def test_render_rows_host_api_band():
    bundle = helpers.cornell()
    p = helpers.params(48, 36, 4, 5)
    ref = helpers.oracle_render(bundle, p)
    canva = np.full((36, 48, 3), -7.0)
    alb = np.full((36, 48, 3), -7.0)
    nrm = np.full((36, 48, 3), -7.0)
    tipe_rt.check(tipe_rt.lib().rt_render_rows(C.byref(bundle.scene), C.byref(p), 20, 9, canva.ctypes.data,
                                               alb.ctypes.data, nrm.ctypes.data))
    assert (canva[9:21] == ref["canva"][9:21]).all()
    assert (alb[9:21] == ref["albedo"][9:21]).all() and (nrm[9:21] == ref["normal"][9:21]).all()
    untouched = np.ones(36, bool)
    untouched[9:21] = False
    assert (canva[untouched] == -7.0).all()       # only the named rows are written


def test_cyclic_tiles_assemble_to_full_frame():
    import torch
    bundle = helpers.cornell()
    W, H, k, world = 40, 30, 4, 3
    p = helpers.params(W, H, 4, 5)
    ref = helpers.oracle_render(bundle, p)
    ds = tipe_rt.DeviceScene(bundle.scene, 0)
    stream = torch.cuda.current_stream().cuda_stream
    per_rank = tipe_rt.cyclic_tiling(H, k, 0, world).n_tiles
    gathered = torch.zeros((world, per_rank * k, W, 3), dtype=torch.float64, device="cuda:0")
    for r in range(world):
        t = tipe_rt.cyclic_tiling(H, k, r, world)
        tipe_rt.render_async(ds, p, t, gathered[r].data_ptr(), stream=stream)
    full = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    tipe_rt.assemble_async(gathered.data_ptr(), world, k, per_rank * k, W, H, full.data_ptr(), stream)
    torch.cuda.synchronize()
    ds.close()
    assert (full.cpu().numpy() == ref["canva"]).all()


def test_fill_canva_pthread_dropin():
    """rt_fill_canva takes main.c's ThreadData; 4 threads on disjoint bands."""
    bundle = helpers.cornell()
    W, H = 40, 30
    p = helpers.params(W, H, 4, 5)
    ref = helpers.oracle_render(bundle, p)
    canva, alb, nrm = (np.zeros((H, W, 3)) for _ in range(3))
    tds = []
    bands = [(29, 22), (21, 15), (14, 8), (7, 0)]
    for hi, lo in bands:
        td = ThreadData()
        td.start_row, td.end_row = hi, lo
        td.canva = C.cast(canva.ctypes.data, C.POINTER(tipe_rt.Vec3))
        td.albedo_tab = C.cast(alb.ctypes.data, C.POINTER(tipe_rt.Vec3))
        td.normal_tab = C.cast(nrm.ctypes.data, C.POINTER(tipe_rt.Vec3))
        td.cam = p.cam
        td.largeur_image, td.hauteur_image = W, H
        td.nbRayonParPixel, td.nbRebondMax = 4, 5
        td.total_pixels = W * H
        td.sphere_list = C.cast(bundle.spheres, C.POINTER(Sphere))
        td.nbSpheres = len(bundle.spheres)
        td.focus_distance = 3
        tds.append(td)
    res = []
    ths = [threading.Thread(target=lambda t=t: res.append(tipe_rt.lib().rt_fill_canva(C.byref(t)))) for t in tds]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert all(r is None for r in res), tipe_rt.lib().rt_last_error()
    assert (canva == ref["canva"]).all() and (alb == ref["albedo"]).all() and (nrm == ref["normal"]).all()


def test_invalid_arguments_fail_loudly():
    bundle = helpers.cornell()
    p = helpers.params(8, 6, 0, 5)
    canva = np.zeros((6, 8, 3))
    rc = tipe_rt.lib().rt_render_rows(C.byref(bundle.scene), C.byref(p), 5, 0, canva.ctypes.data, None, None)
    assert rc == tipe_rt.RT_EINVAL and b"nbRayonParPixel" in tipe_rt.lib().rt_last_error()
    p = helpers.params(8, 6, 1, 5, rng=tipe_rt.RT_RNG_GLIBC)
    rc = tipe_rt.lib().rt_render_rows(C.byref(bundle.scene), C.byref(p), 5, 0, canva.ctypes.data, None, None)
    assert rc == tipe_rt.RT_EUNSUPPORTED
