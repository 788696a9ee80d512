"""rt.h RT_SEM_CUDA: main_cuda.cu's integrator (an optional
fidelity mode beside the authoritative main.c path).

CPU tests pin the oracle's restatement of main_cuda.cu on behaviours the
CUDA source fixes without a GPU: the x1.20 emitter display
(main_cuda.cu:89-99), black misses, the albedo/normal of the pre-pass hit,
the t1 >= 0 sphere acceptance (sphere.hu:27-36), the mesh-box cull
(triangle.hu:42-59) and the (i + 0.5 + U) jitter (main_cuda.cu:152-153).
The CUDA build itself (curand XORWOW, __cosf/__sinf) cannot run here, so
the mode's images are pinned to the restatement only ("parity unpinned"
against NVIDIA output).  GPU tests compare the kernel with the
restatement bit for bit."""
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle_ffi
import tipe_rt
from tipe_rt import scenes
from tipe_rt.types import Sphere, Vec3, RT_SEM_CUDA, Material


def emitter_scene():
    """One big emitter sphere filling the view (camera at the origin)."""
    sph = (Sphere * 1)()
    sph[0].center = Vec3(0.0, 0.0, -5.0)
    sph[0].radius = 4.0
    sph[0].mat = scenes.material((0.2, 0.3, 0.4), (1.0, 0.6, 0.2), 4.0, 0.0)
    return helpers.SceneBundle(sph)


def cam_origin():
    return tipe_rt.init_camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0, 4.0 / 3.0)


def test_cuda_emitter_display_is_hsl_x120():
    b = emitter_scene()
    p = helpers.params(8, 6, 2, 3, cam=cam_origin(), semantics=RT_SEM_CUDA)
    ref = helpers.oracle_render(b, p)
    o = oracle_ffi.oracle()
    hsl = o.oracle_rgb_to_hsl(tipe_rt.types.Vec3(1.0, 0.6, 0.2))
    hsl.e[2] *= 1.20
    hsl.e[1] *= 1.20
    want = o.oracle_hsl_to_rgb(hsl)
    want = np.array([want.e[0], want.e[1], want.e[2]])
    # every sample sees the emitter: radiance mean = albedo mean = the display colour
    assert np.allclose(ref["radiance"], want, rtol=0, atol=1e-15)
    assert np.allclose(ref["albedo"], want, rtol=0, atol=1e-15)
    main = helpers.oracle_render(b, helpers.params(8, 6, 2, 3, cam=cam_origin()))
    assert not np.allclose(main["radiance"], want)            # main.c: x1.0


def test_cuda_miss_is_black_and_albedo_is_first_hit():
    # README box seen by the README camera: the open front lets paths escape
    b = helpers.cornell()
    p = helpers.params(16, 12, 4, 5, semantics=RT_SEM_CUDA)
    ref = helpers.oracle_render(b, p)
    assert np.isfinite(ref["radiance"]).all()
    # albedo samples are first-hit diffuse colours (or emitter display colours)
    assert (ref["albedo"] >= 0).all() and (ref["albedo"] <= 1.2 + 1e-12).all()
    # same scene, main.c semantics: a different image (x1.3 brightening etc.)
    main = helpers.oracle_render(b, helpers.params(16, 12, 4, 5))
    assert not np.array_equal(main["radiance"], ref["radiance"])


def test_cuda_hit_sphere_accepts_t1_from_zero():
    """sphere.hu:27-36 accepts t1 >= 0 (sphere.h: 1e-4).  A ray starting on
    the unit sphere and entering it has t1 = 0 exactly: the CUDA path hits
    the sphere again at t = 0, main.c goes on to t2 = 2."""
    o = oracle_ffi.oracle()
    r = tipe_rt.types.Ray(Vec3(0.0, 0.0, 1.0), Vec3(0.0, 0.0, -1.0))
    hc = o.oracle_hit_sphere_cuda(Vec3(0, 0, 0), 1.0, r)
    hm = o.oracle_hit_sphere(Vec3(0, 0, 0), 1.0, r)
    assert hc.didHit and hc.dst == 0.0
    assert hm.didHit and hm.dst == 2.0
    # t2 needs 0.001 in the CUDA path: leaving outward, t2 = 0 is a miss
    r2 = tipe_rt.types.Ray(Vec3(0.0, 0.0, 1.0), Vec3(0.0, 0.0, 1.0))
    assert not o.oracle_hit_sphere_cuda(Vec3(0, 0, 0), 1.0, r2).didHit


def test_cuda_mode_validation():
    b = helpers.sky_scene()
    p = helpers.params(8, 6, 1, 2, semantics=RT_SEM_CUDA, sky_mode=1)
    W, H = 8, 6
    bufs = [np.zeros((H, W, 3)) for _ in range(4)]
    rc = oracle_ffi.oracle().oracle_render_rows(C.byref(b.scene), C.byref(p), H - 1, 0, 1, 0,
                                                *[x.ctypes.data for x in bufs], None)
    assert rc == tipe_rt.types.RT_EINVAL
    p.sky_mode, p.semantics = 0, 7
    rc = oracle_ffi.oracle().oracle_render_rows(C.byref(b.scene), C.byref(p), H - 1, 0, 1, 0,
                                                *[x.ctypes.data for x in bufs], None)
    assert rc == tipe_rt.types.RT_EINVAL


def test_cuda_mesh_box_culls_flat_axis_aligned_mesh():
    """triangle.hu:42-59 requires a positive overlap of the box's slabs: a
    mesh flat in y (zero box thickness) is never tested in the CUDA path, so
    a camera looking down on it sees through it; main.c sees it."""
    from tipe_rt.types import Triangle, UV
    tris = (Triangle * 2)()
    A, B, Cc, D = (-1, -0.5, -1), (1, -0.5, -1), (1, -0.5, -3), (-1, -0.5, -3)
    for t, (p0, p1, p2) in zip(tris, [(A, B, Cc), (A, Cc, D)]):
        t.A, t.B, t.C = Vec3(*p0), Vec3(*p1), Vec3(*p2)
        t.uvA = t.uvB = t.uvC = UV(0.5, 0.5)
        t.mat = scenes.material((1.0, 0.0, 0.0))
    qm = (C.c_int * 2)(0, 0)
    mats = (Material * 1)()
    mats[0] = scenes.material((1.0, 0.0, 0.0))
    light = (Sphere * 1)()
    light[0].center = Vec3(0.0, 3.0, -2.0)
    light[0].radius = 1.0
    light[0].mat = scenes.material((0, 0, 0), (1, 1, 1), 3.0, 0.0)
    b = helpers.SceneBundle(light, (tris, qm, mats, 1, 1, 1))
    cam = tipe_rt.init_camera((0, 1.5, 0.5), (0, -0.5, -2), (0, 1, 0), 50.0, 4.0 / 3.0)
    ref_c = helpers.oracle_render(b, helpers.params(8, 6, 2, 2, cam=cam, semantics=RT_SEM_CUDA))
    ref_m = helpers.oracle_render(b, helpers.params(8, 6, 2, 2, cam=cam))
    # the quad's red albedo shows only in main.c semantics (the triangles are
    # front-facing for this camera: det = -d.N >= 1e-6 with N = AB x AC)
    assert ref_m["albedo"][..., 0].max() > 0.5
    assert ref_c["albedo"][..., 0].max() == 0.0


# ---- GPU: kernel vs restatement ---------------------------------------------
@pytest.mark.gpu
def test_gpu_cuda_mode_cornell_bitexact():
    from gpu_driver import check_parity
    check_parity(helpers.cornell(), helpers.params(40, 30, 8, 5, semantics=RT_SEM_CUDA))


@pytest.mark.gpu
def test_gpu_cuda_mode_ao_and_chunks_bitexact():
    from gpu_driver import check_parity
    check_parity(helpers.cornell(), helpers.params(32, 24, 8, 6, use_ao=True, ao=2.5, chunks=4,
                                                   semantics=RT_SEM_CUDA))


@pytest.mark.gpu
def test_gpu_cuda_mode_pyramid_mesh_bitexact():
    from gpu_driver import check_parity
    mesh = scenes.with_cuda_materials(scenes.pyramid_mesh())
    check_parity(helpers.SceneBundle(scenes.cornell_spheres(), mesh), helpers.params(40, 30, 8, 6,
                                                                                     semantics=RT_SEM_CUDA))


@pytest.mark.gpu
def test_gpu_cuda_mode_tree_bvh_bitexact():
    from gpu_driver import check_parity
    mesh = scenes.with_cuda_materials(scenes.tree_mesh())
    bundle = helpers.SceneBundle(scenes.cornell_spheres(), mesh)
    check_parity(bundle, helpers.params(24, 18, 4, 6, use_ao=True, ao=3.0, semantics=RT_SEM_CUDA))


def _cuda_pyramid():
    return helpers.SceneBundle(scenes.cornell_spheres(), scenes.with_cuda_materials(scenes.pyramid_mesh()))


def _cuda_tree():
    return helpers.SceneBundle(scenes.cornell_spheres(), scenes.with_cuda_materials(scenes.tree_mesh()))


def _cuda_wide():
    import kernel_cases
    mesh = kernel_cases.alpha_mesh()                    # shared: the triangles' own materials go on a copy
    return helpers.SceneBundle(scenes.cornell_spheres(), scenes.with_cuda_materials(helpers.mesh_of(mesh, len(mesh[0]))))


def assert_cuda_counters_match_oracle(bundle, p, bvh, nthreads=1):
    """The nine reference counters (RT_CNT_SAMPLES .. RT_CNT_RNG_DRAWS) of
    render_kernel_cuda<COUNT> against the oracle's tracer_cuda, exactly.
    RT_CNT_TRI_TESTS is main_cuda.cu:40-45's: the triangles are tested only by
    casts that meet the mesh box.  Texture hits are a main.c event
    (tri_uvmapping); CUDA mode has none."""
    from gpu_driver import gpu_counts
    T = tipe_rt.types
    ref = helpers.oracle_render(bundle, p, nthreads=nthreads, counters=True)["counters"]
    got = gpu_counts(bundle, p)
    nine = T.RT_CNT_EXACT_RESCANS
    names = tipe_rt.COUNTER_NAMES
    print(dict(zip(names, got)))
    assert [int(x) for x in got[:nine]] == [int(x) for x in ref[:nine]], (dict(zip(names, got)),
                                                                          dict(zip(names, (int(x) for x in ref))))
    nt = bundle.scene.nbTriangles
    assert got[T.RT_CNT_TEX_HITS] == 0 and got[T.RT_CNT_REFRACT] == 0
    # some casts miss the mesh box and some meet it: the count is neither 0 nor main.c's casts x triangles
    assert 0 < got[T.RT_CNT_TRI_TESTS] < got[T.RT_CNT_CASTS] * nt and got[T.RT_CNT_TRI_TESTS] % nt == 0
    assert got[T.RT_CNT_BVH_TRI_TESTS] <= got[T.RT_CNT_TRI_TESTS]
    assert (got[T.RT_CNT_BVH_NODES] > 0) == bvh and got[T.RT_CNT_BVH_STACK_OVER] == 0


@pytest.mark.gpu
def test_gpu_cuda_mode_counters_match_oracle():
    assert_cuda_counters_match_oracle(_cuda_pyramid(), helpers.params(24, 18, 4, 6, use_ao=True, ao=2.5,
                                                                       semantics=RT_SEM_CUDA), bvh=False)


@pytest.mark.gpu
def test_gpu_cuda_mode_counters_match_oracle_bvh():
    """render_kernel_cuda<COUNT, BVH>: the tree; 21x13 leaves partial waves and blocks."""
    assert_cuda_counters_match_oracle(_cuda_tree(), helpers.params(21, 13, 3, 5, use_ao=True, ao=2.5,
                                                                    semantics=RT_SEM_CUDA), bvh=True)


@pytest.mark.gpu
def test_gpu_cuda_mode_counters_match_oracle_wide():
    """render_kernel_cuda_w<COUNT>: the 66 248-triangle mesh (a wide tree)."""
    assert_cuda_counters_match_oracle(_cuda_wide(), helpers.params(16, 12, 2, 2, semantics=RT_SEM_CUDA), bvh=True,
                                      nthreads=8)
