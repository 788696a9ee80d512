"""Meshes above 65535 triangles walk a wide BVH on the GPU.

Such a mesh used to get no tree (16-bit stack entries and child indices) and
fell to the every-triangle scan.  rt_scene_upload now builds a wide tree
(rt_bvh.h BvhBuild::wide) and the launch takes render_kernel_q<QB=5> (the
deep-tree queue kernel over 64-byte BvhNodeW nodes with a 24-bit stack) or,
without a task queue or when the wide nodes do not pack, render_kernel<BVH32>
(the fixed grid with uint32 stack entries).  The scene is the README box with
scenes.heightfield_mesh as its floor, so camera rays and bounces hit the
terrain.  Every comparison is bit for bit on canva, albedo, normal and
radiance, against the oracle (which scans every triangle) or against the
GPU's own every-triangle scan (accel = RT_ACCEL_NONE), and every case asserts
the kernel the launch took.  Each scene is uploaded once.
"""
import numpy as np
import pytest

import helpers
import kernel_cases
import tipe_rt
from gpu_driver import Uploaded, assert_same_frame
from kernel_cases import QB5, BVH32
from tipe_rt import scenes
from tipe_rt.types import (Sphere, RT_ACCEL_NONE, RT_CNT_BVH_NODES, RT_CNT_BVH_STACK_OVER, RT_CNT_BVH_TRI_TESTS,
                           RT_CNT_TRI_TESTS)

pytestmark = pytest.mark.gpu


def uploaded(spheres, mesh):
    return Uploaded(helpers.SceneBundle(spheres, mesh))


def against_oracle(up, p, nthreads=8):
    assert_same_frame(up.render(p), helpers.oracle_render(up.bundle, p, nthreads=nthreads))
    return up.kernel


def against_brute_force(up, W, H, spp, bounces, **kw):
    """The BVH render against the same launch with accel = RT_ACCEL_NONE."""
    ref = up.render(helpers.params(W, H, spp, bounces, accel=RT_ACCEL_NONE, **kw))
    assert "BVH" not in up.kernel and "QB=5" not in up.kernel, up.kernel
    assert_same_frame(up.render(helpers.params(W, H, spp, bounces, **kw)), ref)
    return up.kernel


@pytest.fixture(scope="module")
def big():
    """180 000 triangles: node indices pass 16 bits too (90 671 nodes)."""
    up = uploaded(scenes.cornell_spheres(), scenes.heightfield_mesh(300, 1, 0.25, scenes.README_FLOOR))
    yield up
    up.close()


@pytest.fixture(scope="module")
def alpha_mesh():
    """66 248 triangles with a refracting (alpha 0.5) texel and an alpha-0 hole
    (kernel_cases.alpha_mesh: shared with the counter tests)."""
    return kernel_cases.alpha_mesh()


@pytest.fixture(scope="module")
def mid(alpha_mesh):
    up = uploaded(scenes.cornell_spheres(), alpha_mesh)
    yield up
    up.close()


def test_180000_triangles_match_the_oracle(big):
    """16x12, 2 spp, 2 bounces: the oracle's every-triangle scan of this frame
    took 2.8 s on 8 threads when measured (the 24x18 frame of the 66 248-triangle
    case below 2.0 s)."""
    assert against_oracle(big, helpers.params(16, 12, 2, 2, chunks=4)) == QB5


@pytest.mark.parametrize("kw,kernel", [(dict(chunks=4), QB5), (dict(chunks=1), BVH32),
                                       (dict(chunks=4, use_ao=True), QB5)],
                         ids=["queue", "fixed-grid", "queue-ao"])
def test_180000_triangles_match_gpu_brute_force(big, kw, kernel):
    assert against_brute_force(big, 64, 48, 2, 4, **kw) == kernel


def test_alpha_holes_and_refraction_through_the_wide_kernel(mid):
    assert against_oracle(mid, helpers.params(24, 18, 2, 4, chunks=4)) == QB5


def test_far_origins_under_the_sky_sphere(alpha_mesh):
    """main.c:346's radius-1e5 sky, zero-throughput exit off: sky hits go on
    from |o| ~ 1e5 through the wide tree with per-ray margins (ray32<true>)."""
    up = uploaded(scenes.main_spheres(), alpha_mesh)
    with tipe_rt.reference_counts():
        assert against_brute_force(up, 32, 24, 2, 4, chunks=4) == QB5
    up.close()


def test_counters_show_the_tree_culls(big):
    c = big.counts(helpers.params(16, 12, 2, 2, chunks=4))
    assert c[RT_CNT_BVH_STACK_OVER] == 0, c
    assert c[RT_CNT_BVH_NODES] > 0, c
    assert c[RT_CNT_BVH_TRI_TESTS] * 100 < c[RT_CNT_TRI_TESTS], c


@pytest.mark.parametrize("nt,kernel", [(65535, "render_kernel<BVH>"), (65536, BVH32)])
def test_boundary_between_narrow_and_wide(alpha_mesh, nt, kernel):
    """65 535 triangles keep the narrow fixed-grid kernel they took before wide
    trees existed (above 32768 triangles no narrow tree takes the queue
    kernel); one more triangle makes the tree wide."""
    up = uploaded(scenes.cornell_spheres(), helpers.mesh_of(alpha_mesh, nt))
    assert against_brute_force(up, 32, 24, 1, 4) == kernel
    up.close()


def test_leaves_of_three(alpha_mesh, monkeypatch):
    monkeypatch.setenv("RT_BVH_LEAF", "3")               # read by rt_scene_upload's build
    up = uploaded(scenes.cornell_spheres(), alpha_mesh)
    monkeypatch.delenv("RT_BVH_LEAF")
    assert against_brute_force(up, 32, 24, 2, 4, chunks=4) == QB5
    up.close()


def test_scene_beyond_binary16_takes_the_wide_fixed_grid(alpha_mesh):
    """Every coordinate x 1e5: the BvhNodeW form does not pack, so even a
    launch with a task queue walks the 128-byte nodes on the fixed grid."""
    k = 1e5
    tris, qm, mats, tw, th, nm = helpers.mesh_of(alpha_mesh, len(alpha_mesh[0]))
    np.frombuffer(tris, dtype=np.float64).reshape(len(tris), -1)[:, :9] *= k
    sun = (Sphere * 1)(scenes.main_spheres()[0])
    sun[0].center = scenes.Vec3(0.5 * k, 2.8 * k, -1.2 * k)
    sun[0].radius = 0.3 * k
    cam = scenes.README_CAMERA
    camera = helpers.camera_of(dict(cam, origin=tuple(k * x for x in cam["origin"]),
                                    target=tuple(k * x for x in cam["target"])))
    up = uploaded(sun, (tris, qm, mats, tw, th, nm))
    assert against_brute_force(up, 32, 24, 2, 4, chunks=4, cam=camera, focus=3.0 * k) == BVH32
    up.close()
