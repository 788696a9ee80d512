"""Which task-queue instantiation a scene takes, and that each is bit-exact.

r04 splits render_kernel_q by what the scene can reach (DESIGN §4a
"Instantiations"):
  * QB = -2: spheres only, every material opaque -- no triangle scan, no
    alpha-hole or refraction branch compiled in (the C2 bench scene);
  * QB = -1: spheres only, some material transparent or a hole;
  * QB = 0: spheres and brute-force triangles (<= 32, no BVH);
  * QB = 3 with OPQ: the deep-tree kernel when every sphere material, every
    texel and every material index (no 3 or 4, tri_material's overrides)
    is opaque (C4).
The host picks them (rt_launch_plan.cpp plan_render) from the scene upload's
material flags.  main.c:196-234 decides per hit: alpha < 0.0001 is a hole,
alpha <= 0.99 refracts, anything else (NaN included) shades; the opaque
gate is exactly "no material takes either of the first two branches", so a
material at alpha = 0.99 must keep the refraction code and one just above
it must not.  Every render is compared with the oracle bit for bit.
"""
import pytest

import helpers
import tipe_rt
from gpu_driver import assert_stack_bound_holds, render_and_compare
from kernel_cases import ALPHA_KERNEL, OVERRIDE_KERNEL, _nature, one_transparent, override_tree, prm
from tipe_rt import scenes

pytestmark = pytest.mark.gpu


def test_opaque_sphere_scene_takes_qb_minus2():
    assert render_and_compare(helpers.cornell(), prm()) == "render_kernel_q<QB=-2>"


@pytest.mark.parametrize("alpha", [0.5, 0.99, 0.00005, 0.0])
def test_transparent_or_hole_sphere_takes_qb_minus1(alpha):
    assert render_and_compare(one_transparent(alpha), prm()) == ALPHA_KERNEL[alpha]


def test_alpha_just_above_refraction_threshold_is_opaque():
    assert render_and_compare(one_transparent(0.9900001), prm()) == ALPHA_KERNEL[0.9900001]


def test_whole_box_transparent_takes_qb_minus1():
    bundle = helpers.SceneBundle(scenes.cornell_spheres(alpha=0.5))
    assert render_and_compare(bundle, prm()) == "render_kernel_q<QB=-1>"


def test_triangle_scene_takes_qb0():
    assert render_and_compare(helpers.pyramid_scene(), prm()) == "render_kernel_q<QB=0>"


def test_tree_scene_takes_deep_tree_opaque_instantiation():
    """C4: README spheres + the 1320-triangle tree, all opaque."""
    p = helpers.params(40, 30, 6, 8, use_ao=True, chunks=4)
    assert render_and_compare(helpers.tree_scene(), p) == "render_kernel_q<QB=3,OP>"


def test_tree_scene_with_transparent_sphere_keeps_qb3():
    extra = [((0.1, -0.9, -1.8), 0.3, scenes.material((0.8, 0.8, 0.8), alpha=0.5, ior=1.5))]
    bundle = helpers.SceneBundle(scenes.cornell_spheres(extra=extra),
                                 scenes.moved(scenes.load_tree_fixture(), scenes.TREE_MOVE))
    p = helpers.params(40, 30, 6, 8, use_ao=True, chunks=4)
    assert render_and_compare(bundle, p) == "render_kernel_q<QB=3>"


@pytest.mark.parametrize("mat_index", [3, 4])
def test_tree_with_override_material_keeps_qb3(mat_index):
    p = helpers.params(40, 30, 6, 8, use_ao=True, chunks=4)
    assert render_and_compare(override_tree(mat_index), p) == OVERRIDE_KERNEL


@pytest.mark.parametrize("scene", ["tree", "sweep", "mineways", "nature", "main_regime"])
def test_bvh_stack_bound_holds_on_the_gpu(scene):
    """rt_count_async checks every BVH push against the LDS stack of the
    kernel plan_render picks for the tree (rt.h RT_CNT_BVH_STACK_OVER):
    the C4 tree (deep-tree queue kernel, 24 entries), the 100-triangle sweep
    mesh and mineways (606 triangles), over a whole frame with AO."""
    if scene == "tree":
        bundle = helpers.tree_scene()
    elif scene == "mineways":
        bundle = helpers.mineways_scene()
    elif scene in ("nature", "main_regime"):       # 5812 triangles, stack4 22 / main()'s scale
        bundle = helpers.nature_scene() if scene == "nature" else helpers.main_regime_scene()
        p = helpers.params(120, 90, 4, 10, use_ao=True, ao=2.5, chunks=4,
                           cam=helpers.camera_of(scenes.NATURE_CAMERA if scene == "nature" else scenes.MAIN_CAMERA))
        c = assert_stack_bound_holds(bundle, p)
        assert c[tipe_rt.types.RT_CNT_BVH_NODES] > 0
        return
    else:
        sph, mesh = scenes.synthetic_cornell(10, 100)
        bundle = helpers.SceneBundle(sph, mesh)
    p = helpers.params(120, 90, 4, 8, use_ao=True, ao=2.5, chunks=4)
    c = assert_stack_bound_holds(bundle, p)
    assert c[tipe_rt.types.RT_CNT_BVH_NODES] > 0          # the tree was walked


@pytest.mark.parametrize("opaque", [False, True])
def test_tree_with_stack_bound_above_24_keeps_the_queue_kernel(opaque):
    """A tree whose exact stack bound is 26 (> 24, kernel_cases._nature).  The
    non-opaque deep-tree kernel has 32 LDS stack entries (kStackQN; 38 KiB
    per block, still 4 blocks per CU), so it takes such trees -- an opaque
    one too, instead of the 24-entry OPQ kernel -- rather than the fixed
    grid; every push stays inside (RT_CNT_BVH_STACK_OVER == 0), bit for bit
    vs the oracle."""
    bundle = _nature(opaque)
    p = helpers.params(32, 24, 4, 10, chunks=4, cam=helpers.camera_of(scenes.NATURE_CAMERA))
    assert render_and_compare(bundle, p) == "render_kernel_q<QB=3>"
    assert_stack_bound_holds(bundle, p)
