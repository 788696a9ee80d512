"""BVH trees whose 64-byte binary16 form does not exist.

rt_scene_upload packs the tree a second time into 64-byte nodes (binary16
planes, rt_bvh.cpp pack_bvh_h) for the deep-tree queue kernel.  It refuses
when a coordinate lies beyond binary16's range (65504), a leaf index above
65535 or a leaf holds too many triangles.  Then:
  * a deep tree (the queue kernel's QB 3 instantiation, which walks the
    64-byte nodes) renders with the fixed-grid BVH kernel;
  * a shallow tree (QB 4, which walks the 128-byte nodes anyway) keeps the
    task-queue kernel.
Both must stay bit-exact against the oracle (mesh.h:70-94 through
closest_hit main.c:52-92), and rt_last_render_kernel names the path taken.
"""
import numpy as np
import pytest

import helpers
from gpu_driver import render_and_compare
from kernel_cases import FALLBACK, with_far_triangle
from tipe_rt import scenes

pytestmark = pytest.mark.gpu


def fallback_case(name):
    scene, params, kernel = FALLBACK[name]
    assert render_and_compare(scene(), params()) == kernel


def test_deep_tree_without_binary16_nodes_takes_fixed_grid():
    fallback_case("deep_far")


def test_deep_tree_with_binary16_nodes_takes_queue_qb3():
    """Control: the same tree without the far triangle packs, and runs the
    deep-tree queue kernel (its opaque-material instantiation: the tree's
    texels and the README spheres are opaque, test_gpu_instantiations.py)."""
    fallback_case("deep")


def test_shallow_tree_without_binary16_nodes_keeps_queue_qb4():
    fallback_case("shallow_far")


def test_far_triangle_is_invisible():
    """The appended triangle changes no pixel (so the fallback tests compare
    the same picture as the packed tree)."""
    p = helpers.params(24, 18, 2, 6, chunks=2)
    a = helpers.oracle_render(helpers.tree_scene(), p)["canva"]
    b = helpers.oracle_render(helpers.SceneBundle(scenes.cornell_spheres(), with_far_triangle(
        scenes.moved(scenes.load_tree_fixture(), scenes.TREE_MOVE))), p)["canva"]
    assert np.array_equal(a, b)
