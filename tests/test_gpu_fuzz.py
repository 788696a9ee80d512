"""Randomised scenes, GPU vs oracle bit for bit (RT_RNG_PHILOX).

Each seed builds a scene the hand-written tests do not: random spheres
(some enclosing the camera, translucent ones with 1e-4 <= alpha <= 0.99,
alpha holes, emitters, mirrors), optionally a random textured mesh with
the reference's hard-coded material overrides (texture.h:71-87, indices
1/3/4), random camera, aperture, focus, AO on/off, spp_chunks, and more
than 32 triangles on odd seeds so the BVH path runs.  Sizes stay small
so the oracle finishes in about a second per scene."""
import pytest

import tipe_rt
from gpu_driver import check_parity, assert_stack_bound_holds
from helpers import random_scene
from tipe_rt import scenes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(64))
def test_random_scene_bitexact(seed):
    bundle, p = random_scene(seed)
    check_parity(bundle, p)


@pytest.mark.parametrize("seed", range(800, 840))
def test_random_far_scene_bitexact(seed):
    """main()'s coordinate regime: every random scene scaled by 50-2000 and
    moved by up to 1000 units, inside a radius-1e5 emissive sky sphere
    (main.c:300-301, 346), so the candidate pass's interval bound
    (Hs = (|o| + L) sqrt(a)) and the BVH padding run at |o|, L ~ 1e3-1e5;
    0-24 bounces; spp_chunks 1-3; bit for bit vs the oracle.  Odd seeds run
    with the zero-throughput exit off, so paths go on after a sky hit and
    BVH walks start at |o| ~ 1e5 (per-ray margins, rt_triangles.h ray32)."""
    bundle, p = random_scene(seed, far=True)
    if seed % 2:
        with tipe_rt.reference_counts():
            check_parity(bundle, p)
    else:
        check_parity(bundle, p)


@pytest.mark.parametrize("seed", range(200, 248))
def test_random_scene_zero_throughput_queue_bitexact(seed):
    """Random scenes whose colours have exact-zero channels (paths end at
    zero throughput), rendered with spp_chunks 2-4 (the queue kernel for
    sphere/brute-force scenes, the BVH kernel on odd seeds), bit for bit
    against the oracle, which never ends a path early."""
    bundle, p = random_scene(seed, zeros=True, chunks=2 + seed % 3)
    check_parity(bundle, p)


@pytest.mark.parametrize("seed", range(100, 124))
def test_random_scene_cuda_semantics_bitexact(seed):
    """rt.h RT_SEM_CUDA on random scenes: each triangle takes its first texel
    as its own material (scenes.with_cuda_materials), sky off."""
    bundle, p = random_scene(seed)
    if bundle.mesh is not None:
        scenes.with_cuda_materials(bundle.mesh)
    p.semantics = tipe_rt.types.RT_SEM_CUDA
    check_parity(bundle, p)


@pytest.mark.parametrize("seed", range(300, 324))
def test_random_bvh_scene_queue_tiny_grid_bitexact(seed, monkeypatch):
    """Random 100-400 triangle meshes (BVH) with random spheres, through the
    BVH task-queue kernel (resumable walks, rt_queue.h render_kernel_q<..,
    QB>) on a 1-3 block grid, so every lane runs many tasks and walks span
    rounds across task switches; 5-6 sample slices at 40-48 spp use the
    tapered slice bounds (rt_chunk_bound).  Bit for bit vs the oracle."""
    monkeypatch.setenv("RT_QUEUE_BLOCKS", str(1 + seed % 3))
    bundle, p = random_scene(seed, zeros=bool(seed % 2), chunks=5 + seed % 2, nt_range=(100, 400),
                             spp=40 + 8 * (seed % 2))
    p.largeur_image, p.hauteur_image = min(p.largeur_image, 20), min(p.hauteur_image, 15)
    check_parity(bundle, p)
    assert_stack_bound_holds(bundle, p)


@pytest.mark.parametrize("seed", range(400, 432))
def test_random_opaque_sphere_scene_queue_bitexact(seed):
    """Opaque sphere-only random scenes (r04's QB -2 queue instantiation: no
    triangle, hole or refraction code) at spp_chunks 2-5, zero-throughput
    colours on odd seeds; the kernel taken is checked, bit for bit vs the
    oracle."""
    bundle, p = random_scene(seed, zeros=bool(seed % 2), chunks=2 + seed % 4, opaque=True, mesh_p=0.0)
    check_parity(bundle, p)
    assert tipe_rt.last_render_kernel() == "render_kernel_q<QB=-2>"


@pytest.mark.parametrize("seed", range(500, 516))
def test_random_opaque_bvh_scene_queue_bitexact(seed, monkeypatch):
    """Opaque random 100-400 triangle scenes through the BVH queue kernel
    (the deep-tree OPQ instantiation where the tree is deep) on a 1-3 block
    grid, bit for bit vs the oracle."""
    monkeypatch.setenv("RT_QUEUE_BLOCKS", str(1 + seed % 3))
    bundle, p = random_scene(seed, zeros=bool(seed % 2), chunks=5 + seed % 2, nt_range=(100, 400),
                             spp=40 + 8 * (seed % 2), opaque=True)
    p.largeur_image, p.hauteur_image = min(p.largeur_image, 20), min(p.hauteur_image, 15)
    check_parity(bundle, p)
    assert_stack_bound_holds(bundle, p)
    # deep trees take the OPQ kernel; shallow ones QB 4; a camera outside the
    # scene bound the brute-force scan (QB 0); an over-deep tree the fixed grid
    assert tipe_rt.last_render_kernel() in ("render_kernel_q<QB=3,OP>", "render_kernel_q<QB=3>", "render_kernel_q<QB=4>",
                                            "render_kernel_q<QB=0>", "render_kernel<BVH>")
