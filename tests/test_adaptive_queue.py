"""What is built on the two accumulate entry points obeys
rt_set_accumulate_queue without code of its own, and gives the same bits.

rt_adaptive_async at (first_half 8, 4 rounds, tolerance 1/64) with AUTO slices
-- every batch has min(32, S) > 1 slices, so with the switch on round 0 takes
render_kernel_q and every later round render_kernel_ql -- must leave the
accumulators A and B and the round counts identical, value for value (NaN
excepted as in accumulate_support.assert_same_sums), to a run with the switch
off, whose kernels tests/test_gpu_accumulate_oracle.py holds to the oracle.  At
least two round counts must occur, so that list launches did run.  The planes
of rt_render_vdenoised at 16 spp are identical as well."""
import numpy as np
import pytest

import helpers
import tipe_rt
from accumulate_support import assert_same_sums
from adaptive_support import device_adaptive
from queue_accumulate_support import accumulate_queue
from tipe_rt.types import RT_SPP_CHUNKS_AUTO

pytestmark = pytest.mark.gpu

W, H, BOUNCES = 48, 36, 5
SCENES = {"cornell": (helpers.cornell, "render_kernel", "render_kernel_list", "QB=-2"),
          "tree": (helpers.tree_scene, "render_kernel<BVH>", "render_kernel_list<BVH>", "QB=3,OP")}


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_adaptive_loop_is_the_same_on_and_off(scene):
    make, fixed, fixed_list, qb = SCENES[scene]
    bundle = make()
    p = helpers.params(W, H, 999, BOUNCES, chunks=RT_SPP_CHUNKS_AUTO)       # nbRayonParPixel is ignored
    ap = tipe_rt.adaptive_params(first_half=8, max_rounds=4, tolerance=1.0 / 64.0)
    ds = tipe_rt.DeviceScene(bundle.scene, 0)
    try:
        A0, B0, rounds0, _ = device_adaptive(ds, p, ap, frame=False)
        assert (tipe_rt.last_render_kernel(), tipe_rt.last_list_kernel()) == (fixed, fixed_list)
        with accumulate_queue():
            A1, B1, rounds1, _ = device_adaptive(ds, p, ap, frame=False)
            kernels = (tipe_rt.last_render_kernel(), tipe_rt.last_list_kernel())
    finally:
        ds.close()
    assert kernels == ("render_kernel_q<%s>" % qb, "render_kernel_ql<%s>" % qb)
    assert len(np.unique(rounds0)) >= 2, np.unique(rounds0, return_counts=True)
    assert rounds0.min() >= 1 and rounds0.max() <= 4
    assert (rounds1 == rounds0).all(), "d_rounds differs at %d pixels" % int((rounds1 != rounds0).sum())
    assert_same_sums(A1, A0, scene + " A")
    assert_same_sums(B1, B0, scene + " B")


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_render_vdenoised_is_the_same_on_and_off(scene):
    make, fixed, _, qb = SCENES[scene]
    bundle = make()
    p = helpers.params(W, H, 16, BOUNCES, chunks=RT_SPP_CHUNKS_AUTO)
    off = tipe_rt.render_vdenoised(bundle.scene, p)
    assert tipe_rt.last_render_kernel() == fixed
    with accumulate_queue():
        on = tipe_rt.render_vdenoised(bundle.scene, p)
        assert tipe_rt.last_render_kernel() == "render_kernel_q<%s>" % qb
    for name, a, b in zip(("canva", "albedo", "normal"), on, off):
        assert_same_sums(a, b, "%s %s" % (scene, name))
    assert off[0].max() > 0
