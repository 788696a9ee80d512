"""The GPU suite's one way onto the device and its one rule for "equal".

librt_hip.so (through the C-ABI) against the CPU oracle in RT_RNG_PHILOX mode
on identical seeded inputs.  The kernel performs the reference's IEEE
operations in the same order as the oracle, so the bar is BIT-EXACT equality
of canva (8-bit resolve), albedo, normal and pre-gamma radiance.  north_star's
tolerance (per-channel RMSE <= 1e-4 on float accumulation) is asserted as
well, as the outer bound.

Every rendered frame of the suite comes out of Uploaded.render and every
"frame equals frame" or "frame equals oracle" check goes through
assert_same_frame.  Tests of another entry point (rt_render_rows,
rt_fill_canva, the gathers, rt_accumulate_async / rt_resolve_async, the
denoiser) make their own calls and take device_planes and the comparisons
from here.  torch is imported inside the functions, so CPU tests can import
this module's users.

pytest rewrites `assert` in test modules only: every assertion here carries
its own message with the offending values.
"""
import numpy as np

import helpers
import tipe_rt

RMSE_TOL = 1e-4   # north_star: per-channel RMSE on identical seeds
PLANES = ("canva", "albedo", "normal", "radiance")


def device_planes(rows, W, n=4, fill=-1.0):
    """n (rows, W, 3) float64 planes on cuda:0, filled so an unwritten value shows."""
    import torch
    return [torch.full((rows, W, 3), fill, dtype=torch.float64, device="cuda:0") for _ in range(n)]


class Uploaded:
    """A SceneBundle and its rt_scene_upload handle, kept across renders and
    counter runs until close() (or the end of a `with` block)."""

    def __init__(self, bundle):
        self.bundle = bundle
        self.ds = tipe_rt.DeviceScene(bundle.scene, 0)
        self.kernel = None

    def close(self):
        self.ds.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def render(self, p, tiling=None, radiance=True):
        """rt_render_async into torch buffers: [canva, albedo, normal, radiance]
        over the tiling's rows (the whole frame by default); without radiance
        that plane keeps its fill.  self.kernel is rt_last_render_kernel's name."""
        import torch
        if tiling is None:
            tiling = tipe_rt.band_tiling(0, p.hauteur_image - 1)
        bufs = device_planes(tiling.n_tiles * tiling.tile_rows, p.largeur_image)
        tipe_rt.render_async(self.ds, p, tiling, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                             bufs[3].data_ptr() if radiance else None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        self.kernel = tipe_rt.last_render_kernel()
        return [b.cpu().numpy() for b in bufs]

    def counts(self, p, tiling=None, into=None):
        """rt_count_async over the tiling's rows (the whole frame by default):
        the RT_NCOUNTERS event totals.  into: an int64 device tensor of
        RT_NCOUNTERS entries the launch adds to (a fresh zeroed one by
        default); its values after the launch are returned."""
        import torch
        if tiling is None:
            tiling = tipe_rt.band_tiling(0, p.hauteur_image - 1)
        d = torch.zeros(tipe_rt.RT_NCOUNTERS, dtype=torch.int64, device="cuda:0") if into is None else into
        tipe_rt.count_async(self.ds, p, tiling, d.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return [int(x) for x in d.cpu()]


def gpu_render(bundle, p, tiling=None, radiance=True, kernel=False):
    """Upload, render once, release: the four planes (and the kernel's name)."""
    with Uploaded(bundle) as up:
        got = up.render(p, tiling, radiance)
    return (got, up.kernel) if kernel else got


def gpu_counts(bundle, p):
    with Uploaded(bundle) as up:
        return up.counts(p)


def assert_stack_bound_holds(bundle, p):
    """Every BVH push of the frame's walks stays inside the LDS stack of the
    kernel that renders the tree (rt.h RT_CNT_BVH_STACK_OVER == 0), i.e.
    the host's stack bound (rt_bvh.cpp) covers the kernel's push rule."""
    c = gpu_counts(bundle, p)
    assert c[tipe_rt.types.RT_CNT_BVH_STACK_OVER] == 0, c
    return c


def assert_same(gpu, ref, what, same_bytes=False):
    """Bit-for-bit equal values; NaN must sit at the same places (payloads
    may differ: x86 and gfx950 produce different default NaNs).  same_bytes
    compares zero signs and NaN payloads too (two runs of the same device)."""
    assert gpu.shape == ref.shape, "%s: shape %r vs %r" % (what, gpu.shape, ref.shape)
    diff = np.argwhere((gpu != ref) & ~(np.isnan(gpu) & np.isnan(ref)))
    if len(diff):
        j, i, c = diff[0]
        raise AssertionError("%s: %d mismatching values; first at row %d col %d ch %d: gpu %r oracle %r" %
                             (what, len(diff), j, i, c, gpu[j, i, c], ref[j, i, c]))
    if same_bytes and gpu.tobytes() != ref.tobytes():
        raise AssertionError("%s: equal values, but %d differ in a zero's sign or a NaN's payload" %
                             (what, (gpu.view(np.uint64) != ref.view(np.uint64)).sum()))


def assert_same_frame(got, ref, what="", planes=PLANES, same_bytes=False):
    """assert_same on each of the planes; a frame is a dict by plane name (as
    helpers.oracle_render returns) or a sequence in the order of `planes`."""
    for k, name in enumerate(planes):
        g, r = (x[name] if isinstance(x, dict) else x[k] for x in (got, ref))
        assert_same(g, r, (what + " " + name).strip(), same_bytes)


def render_and_compare(bundle, p, nthreads=1):
    """All four planes against the oracle; returns the kernel the launch took."""
    ref = helpers.oracle_render(bundle, p, nthreads=nthreads)
    got, kernel = gpu_render(bundle, p, kernel=True)
    assert_same_frame(got, ref)
    return kernel


def check_parity(bundle, p, nthreads=1):
    ref = helpers.oracle_render(bundle, p, nthreads=nthreads)
    got = gpu_render(bundle, p)
    canva, rad = got[0], got[3]
    fin = ~np.isnan(ref["radiance"])               # NaN radiance: the reference's own (e.g. AO 0)
    stray = np.isnan(rad) != ~fin
    assert not stray.any(), "radiance: NaN on one side only at %d values, first at %r" % (
        stray.sum(), tuple(np.argwhere(stray)[0]))
    e = helpers.rmse_per_channel(np.where(fin, rad, 0), np.where(fin, ref["radiance"], 0))
    assert (e <= RMSE_TOL).all(), "radiance: per-channel RMSE %r above %g" % (e, RMSE_TOL)
    e = helpers.rmse_per_channel(canva / 255.0, ref["canva"] / 255.0)
    assert (e <= RMSE_TOL).all(), "canva / 255: per-channel RMSE %r above %g" % (e, RMSE_TOL)
    assert_same_frame(got, ref)
    return ref
