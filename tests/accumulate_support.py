"""What the accumulate tests share: the scene table of the fixed-grid kernel
instantiations, the driver of the CPU oracle's oracle_accumulate (rt.h
"progressive rendering" restated in plain C), the device driver of
rt_accumulate_async, and the one rule for "equal": the uint64 bits of all nine
running sums of every local pixel, zero signs included; only a NaN on both
sides is let through.  Both sides perform the same IEEE operations from the
same starting bits, so there is no tolerance."""
import ctypes as C

import numpy as np

import helpers
import oracle_ffi
import tipe_rt
from adaptive_support import sentinel, u64
from tipe_rt import scenes
from tipe_rt.types import Tiling

# scene builder, extra params, the fixed-grid kernel an accumulate launch takes
# (accumulate launches never take the task-queue kernel: rt_launch_plan.cpp)
SCENES = {
    "cornell": (helpers.cornell, {}),                       # no tree: samples_flat
    "pyramid": (helpers.pyramid_scene, {}),                 # brute-force triangles
    "tree": (helpers.tree_scene, {}),                       # narrow tree: samples_coop
    "sky": (helpers.sky_scene, dict(sky_mode=1)),
    "sky_tree": (helpers.sky_tree_scene, dict(sky_mode=1)),
    # 66 248 triangles (test_gpu_big_mesh's builder): a wide tree
    "wide": (lambda: helpers.SceneBundle(scenes.cornell_spheres(),
                                         scenes.heightfield_mesh(182, 1, 0.25, scenes.README_FLOOR, alpha=0.5)), {}),
    "wide_sky": (lambda: helpers.SceneBundle(helpers.sky_scene().spheres,
                                             scenes.heightfield_mesh(182, 1, 0.25, scenes.README_FLOOR, alpha=0.5),
                                             sky=helpers.sky_scene().sky), dict(sky_mode=1)),
}
KERNEL = {"cornell": "render_kernel", "pyramid": "render_kernel", "sky": "render_kernel",
          "tree": "render_kernel<BVH>", "sky_tree": "render_kernel<BVH>",
          "wide": "render_kernel<BVH32>", "wide_sky": "render_kernel<BVH32>"}

# the offsets at which a batch of 4 samples crosses bit 31, ends exactly at
# 2^32, and crosses bit 16 of the Philox sample word
HIGH_OFFSETS = ((1 << 31) - 2, (1 << 32) - 4, (1 << 16) - 2)
LIST_OFFSETS = HIGH_OFFSETS[:2]                  # the ones rt_accumulate_list_async runs at


# scene -> (W, H, bounces) of the frames that run the high offsets (the wide
# tree at test_gpu_big_mesh's scale); two blocks wide, no multiple of 16
WORD_FRAMES = {"cornell": (21, 13, 5), "tree": (21, 13, 5), "wide": (16, 12, 2)}
WORD_BATCH = 4
GUARD = -7.0e6                                   # fills the device memory around an accumulator


def truncated_batches(offset, S, bits):
    """The P = 1 batches that feed a kernel's stream if it cut the sample word
    (offset + x) to `bits` bits: runs of consecutive truncated samples."""
    words = [(offset + x) & ((1 << bits) - 1) for x in range(S)]
    out = []
    for w in words:
        if out and out[-1][0] + out[-1][1] == w:
            out[-1][1] += 1
        else:
            out.append([w, 1])
    return [(w, n, 1) for w, n in out]


class Uploads:
    """name -> (bundle, device scene), each uploaded once and kept until release()."""

    def __init__(self, table=SCENES):
        self.table, self.up = table, {}

    def __call__(self, name):
        if name not in self.up:
            bundle = self.table[name][0]()
            self.up[name] = (bundle, tipe_rt.DeviceScene(bundle.scene, 0))
        return self.up[name]

    def release(self):
        while self.up:
            self.up.popitem()[1][1].close()


def whole(H):
    return tipe_rt.band_tiling(0, H - 1)


def local_rows(t):
    return t.n_tiles * t.tile_rows


def global_rows(t):
    """Global row of every local row of the tiling (rt.h rt_tiling)."""
    ly = np.arange(local_rows(t))
    lt, y = np.divmod(ly, t.tile_rows)
    return t.row_base + (t.tile_first + lt * t.tile_step) * t.tile_rows + y


def batch_params(p, S, chunks):
    q = type(p).from_buffer_copy(p)
    q.nbRayonParPixel, q.spp_chunks = S, chunks
    return q


def oracle_accumulate(bundle, p, offset, tiling, sums, nthreads=8):
    """oracle_accumulate in place on `sums` (local_rows, W, 9) float64; returns its status."""
    assert sums.dtype == np.float64 and sums.flags.c_contiguous
    assert sums.shape == (local_rows(tiling), p.largeur_image, 9), sums.shape
    return oracle_ffi.oracle().oracle_accumulate(C.byref(bundle.scene), C.byref(p), offset, C.byref(tiling), nthreads,
                                                 sums.ctypes.data)


def oracle_batches(bundle, p, batches, tiling, start, nthreads=8):
    """The oracle's sums after the batches [(offset, S, spp_chunks)] onto a copy of `start`."""
    sums = np.array(start, dtype=np.float64, order="C")
    for off, S, chunks in batches:
        rc = oracle_accumulate(bundle, batch_params(p, S, chunks), off, tiling, sums, nthreads)
        assert rc == 0, rc
    return sums


def device_batches(ds, p, batches, tiling, start):
    """rt_accumulate_async for the same batches onto a copy of `start`: (sums, kernel names)."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    # the accumulator lies between two guards of a whole frame's size each, so an access at a global
    # index where the local one belongs stays inside this allocation, and a write there is seen
    n, guard = start.size, p.largeur_image * p.hauteur_image * 9
    buf = torch.full((guard + n + guard,), GUARD, dtype=torch.float64, device="cuda:0")
    sums = buf[guard:guard + n].view(start.shape)
    sums.copy_(torch.from_numpy(np.ascontiguousarray(start)))
    kernels = []
    for off, S, chunks in batches:
        tipe_rt.accumulate_async(ds, batch_params(p, S, chunks), off, tiling, sums.data_ptr(), st)
        kernels.append(tipe_rt.last_render_kernel())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    outside = np.concatenate([host[:guard], host[guard + n:]])
    assert (outside == GUARD).all(), "%d values outside the accumulator were written" % (outside != GUARD).sum()
    return host[guard:guard + n].reshape(start.shape).copy(), kernels


def assert_same_sums(got, want, what):
    """The rule for "equal" (pytest rewrites asserts in test modules only: the message is made here)."""
    assert got.shape == want.shape, "%s: shape %r vs %r" % (what, got.shape, want.shape)
    bad = (u64(got) != u64(want)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        k = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d sums differ in their bits; first at local row %d col %d slot %d: "
                             "device %r (%#x) oracle %r (%#x)" % (what, bad.sum(), bad.size, k[0], k[1], k[2], got[k],
                                                                   int(u64(got)[k]), want[k], int(u64(want)[k])))


def assert_rendered_rows_moved(sums, start, tiling, H, what):
    """Every pixel of a rendered row left its start; a row past H kept its bits."""
    rendered = global_rows(tiling) < H
    moved = (u64(sums) != u64(start)).any(axis=2)
    assert moved[rendered].all(), "%s: %d rendered pixels kept their start values" % (what, (~moved[rendered]).sum())
    assert not moved[~rendered].any(), "%s: %d pixels of rows past H were written" % (what, moved[~rendered].sum())


def check_accumulate(bundle, ds, p, batches, tiling, kernel, what="", start=None):
    """One case: the device's sums after the batches equal the oracle's from the
    same start, every rendered pixel moved, rows past H kept their start, every
    launch took the expected fixed-grid kernel.

    Without a given start the case runs from two.  The sentinel (about -1000
    and different in every pixel and slot) shows an unwritten pixel and a write
    to a wrong local index, but a running sum that large takes each addend
    rounded to its own grid, so the order of the additions shows in about one
    value of a thousand (measured on the oracle: a reversed slice order changes
    5 of 7659 sums of the 37x23 cornell frame).  The sentinel scaled by 2^-20
    (exact, so still different everywhere) is small against one sample: there
    the same reversal changes 874."""
    if start is None:
        big = sentinel(p.largeur_image, local_rows(tiling))
        for name, s in (("sentinel", big), ("sentinel * 2^-20", big * 2.0 ** -20)):
            check_accumulate(bundle, ds, p, batches, tiling, kernel, "%s, from the %s" % (what, name), s)
        return
    H = p.hauteur_image
    want = oracle_batches(bundle, p, batches, tiling, start)
    assert_rendered_rows_moved(want, start, tiling, H, what + " (oracle)")
    got, kernels = device_batches(ds, p, batches, tiling, start)
    assert kernels == [kernel] * len(batches), "%s: kernels %r, expected %r" % (what, kernels, kernel)
    assert_rendered_rows_moved(got, start, tiling, H, what)
    assert_same_sums(got, want, what)


def consecutive(sizes_and_chunks, first=0):
    """[(S, spp_chunks)] -> batches at consecutive offsets from `first`."""
    out, off = [], first
    for S, chunks in sizes_and_chunks:
        out.append((off, S, chunks))
        off += S
    return out


def cyclic(H, k, r, G):
    return tipe_rt.cyclic_tiling(H, k, r, G)


def tiling_of(*fields):
    return Tiling(*fields)
