"""What the paired-draw kernels (render_kernel_q<QB=-2> without AO, rt_queue.h)
no longer compute every round, against the oracle bit for bit:

* the winner's sphere test in half-b units (rt_shared_math.h sphere_halfb),
  whose lanes outside the shifted windows run the reference form;
* the head of a task's Philox blocks kept in LDS from the task's hand-out.

Frames of 48x36 or less, 8 to 16 spp.  spp_chunks 1 is the fixed grid (no
task); 4 gives tasks of several samples; spp_chunks = spp makes every sample
a task, so a lane refreshes its head words at every hand-out.  The cyclic
tiling has padding rows: a lane that draws one keeps its old head words
through a round without a task.  The box scaled by 2^20 and by 2^-20 moves
every quantity the windows test by 2^+-40; emitters whose emission * strength
is inexact, zero and subnormal pin shade_with's product.  One non-opaque scene
(QB -1) and one pyramid scene (QB 0) run kernels this form is not compiled into.
"""
import numpy as np
import pytest

import helpers
import tipe_rt
from tipe_rt import scenes

from gpu_driver import PLANES, assert_same, gpu_render, render_and_compare
from kernel_cases import TRANSPARENT, bundle_of

pytestmark = pytest.mark.gpu

W, H, SPP = 32, 24, 8
QS = "render_kernel_q<QB=-2>"


@pytest.mark.parametrize("chunks", [1, 4, SPP])
@pytest.mark.parametrize("bounces", [0, 1, 5, 6, 7, 20])
def test_box_bounces_and_chunking(bounces, chunks):
    p = helpers.params(W, H, SPP, bounces, chunks=chunks)
    kernel = render_and_compare(helpers.cornell(), p)
    if chunks > 1:
        assert kernel == QS


def test_kernel_name_and_larger_frame():
    p = helpers.params(48, 36, 16, 6, chunks=16)
    assert render_and_compare(helpers.cornell(), p) == QS


def test_sky_kernel():
    p = helpers.params(W, H, SPP, 6, chunks=SPP, sky_mode=1)
    assert render_and_compare(bundle_of((), None, True), p) == QS


def test_cyclic_tiling_with_padding_rows():
    """34 rows in 4-row tiles for three ranks: nine tiles, the last with two
    rows, so every rank's band of 12 rows ends in padding."""
    Hc, k, world = 34, 4, 3
    bundle = helpers.cornell()
    p = helpers.params(W, Hc, SPP, 6, chunks=SPP)
    ref = helpers.oracle_render(bundle, p)
    padded = 0
    for r in range(world):
        t = tipe_rt.cyclic_tiling(Hc, k, r, world)
        got, kernel = gpu_render(bundle, p, t, kernel=True)
        assert kernel == QS
        for lt in range(t.n_tiles):
            for y in range(k):
                g = t.row_base + (t.tile_first + lt * t.tile_step) * k + y
                if g >= Hc:
                    padded += 1
                    continue
                for plane, name in zip(got, PLANES):
                    assert_same(plane[lt * k + y][None], ref[name][g][None], "rank %d row %d %s" % (r, g, name))
    assert padded > 0


def scaled_box(s):
    """The README box and its camera with every coordinate and length times s."""
    sph = scenes.cornell_spheres()
    for q in sph:
        q.center = tipe_rt.types.Vec3(*[s * x for x in q.center.e])
        q.radius = s * q.radius
    spec = dict(scenes.README_CAMERA)
    spec["origin"] = tuple(s * x for x in spec["origin"])
    spec["target"] = tuple(s * x for x in spec["target"])
    return helpers.SceneBundle(sph), helpers.camera_of(spec), 3.0 * s


@pytest.mark.parametrize("exp", [20, -20])
def test_far_coordinates(exp):
    bundle, cam, focus = scaled_box(2.0 ** exp)
    p = helpers.params(W, H, SPP, 6, chunks=4, cam=cam, focus=focus)
    assert render_and_compare(bundle, p) == QS


def test_emitters():
    """0.55 * 2.5 and 0.863 * 2.5 (the README light) are inexact already; the
    extra emitters' products are inexact in every channel, zero (es = 0: no
    light, the surface bounces on), and subnormal."""
    m = scenes.material
    extra = [((-0.5, -0.7, -2.2), 0.3, m((0.7, 0.6, 0.5), (0.1, 0.7, 0.3), 1.0 / 3.0)),
             ((0.5, -0.7, -2.6), 0.3, m((0.9, 0.9, 0.9), (1.0, 0.5, 0.25), 0.0)),
             ((0.0, -0.8, -1.6), 0.2, m((0.8, 0.8, 0.8), (0.3, 0.6, 0.9), 1e-310))]
    for _, _, mt in extra[:1] + extra[2:]:
        e = np.array(mt.emissionColor.e[:]) * mt.emissionStrength
        assert (e != 0).all()
    assert (np.array(extra[2][2].emissionColor.e[:]) * 1e-310 < 2.3e-308).all()
    p = helpers.params(W, H, SPP, 6, chunks=4)
    assert render_and_compare(helpers.cornell(extra), p) == QS


def test_unaffected_non_opaque():
    p = helpers.params(W, H, SPP, 6, chunks=4)
    assert render_and_compare(bundle_of(TRANSPARENT, None, False), p) == "render_kernel_q<QB=-1>"


def test_unaffected_pyramid():
    p = helpers.params(W, H, SPP, 6, chunks=4)
    assert render_and_compare(helpers.pyramid_scene(), p) == "render_kernel_q<QB=0>"
