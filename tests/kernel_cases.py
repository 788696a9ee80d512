"""Scene -> kernel name: which instantiation plan_render (rt_launch_plan.cpp)
picks for a scene, as data.  The GPU tests render each scene and assert
rt_last_render_kernel's name; tests/test_launch_plan.py checks the same
triples on the CPU.  Nothing here touches the device.
"""
import functools

import helpers
from tipe_rt import scenes
from tipe_rt.types import Material

# ---- every render_kernel_q instantiation (tests/test_gpu_queue_variants.py) ----
# one alpha-0.5 sphere in view: keeps the refraction code compiled in
TRANSPARENT = [((0.1, -0.9, -1.8), 0.3, scenes.material((0.8, 0.8, 0.8), alpha=0.5, ior=1.5))]

# variant -> (expected kernel name, extra spheres, mesh or None); without sky
# these are cornell(), cornell() + the sphere, pyramid_scene(), tree_scene(),
# the tree + the sphere, and synthetic_cornell(10, 100)
VARIANTS = {
    "QB-2": ("render_kernel_q<QB=-2>", (), lambda: None),
    "QB-1": ("render_kernel_q<QB=-1>", TRANSPARENT, lambda: None),
    "QB0": ("render_kernel_q<QB=0>", (), scenes.pyramid_mesh),
    "QB3OP": ("render_kernel_q<QB=3,OP>", (), scenes.tree_mesh),
    "QB3": ("render_kernel_q<QB=3>", TRANSPARENT, scenes.tree_mesh),
    "QB4": ("render_kernel_q<QB=4>", (), lambda: scenes.synthetic_cornell(10, 100)[1]),
}


def bundle_of(extra, mesh, sky):
    spheres = scenes.cornell_spheres(extra=extra)
    if not sky:
        return helpers.SceneBundle(spheres, mesh)
    sk = helpers.sky_scene()
    sph = helpers.spheres_plus(spheres, [sk.spheres[len(sk.spheres) - 1]])         # the sky sphere stays last
    return helpers.SceneBundle(sph, mesh, sky=sk.sky)


def variant_params(sky, ao):
    return helpers.params(24, 18, 4, 6, use_ao=ao, ao=2.5, chunks=2, sky_mode=1 if sky else 0)


# ---- opaque gates (tests/test_gpu_instantiations.py) ---------------------------
def one_transparent(alpha):
    """README box plus one extra small sphere of the given alpha in view."""
    extra = [((0.1, -0.9, -1.8), 0.3, scenes.material((0.8, 0.8, 0.8), alpha=alpha, ior=1.5))]
    return helpers.SceneBundle(scenes.cornell_spheres(extra=extra))


P = dict(W=40, H=30, spp=8, bounces=6)


def prm(**kw):
    q = dict(P)
    q.update(kw)
    return helpers.params(q["W"], q["H"], q["spp"], q["bounces"], chunks=4)


# alpha of the extra sphere -> the kernel
ALPHA_KERNEL = {0.5: "render_kernel_q<QB=-1>", 0.99: "render_kernel_q<QB=-1>", 0.00005: "render_kernel_q<QB=-1>",
                0.0: "render_kernel_q<QB=-1>", 0.9900001: "render_kernel_q<QB=-2>"}
OVERRIDE_KERNEL = "render_kernel_q<QB=3>"


def override_tree(mat_index):
    """tri_material's material indices 3 and 4 force alpha 0.1 / 0.6 whatever
    the texel holds: a tree whose first triangles use one of them is not
    opaque.  The texel table gets entries up to that index (copies of
    material 0), so the scene stays valid."""
    tris, qm, mats, tw, th, nm = scenes.moved(scenes.load_tree_fixture(), scenes.TREE_MOVE)
    n_new = max(nm, mat_index + 1)
    mats2 = (Material * (n_new * tw * th))()
    for k in range(n_new * tw * th):
        mats2[k] = mats[k] if k < nm * tw * th else mats[0]
    for k in range(0, len(tris), 7):
        qm[k] = mat_index
    return helpers.SceneBundle(scenes.cornell_spheres(), (tris, qm, mats2, tw, th, n_new))


def _nature(opaque, far_z=4e4):
    """RTX_MAP/nature plus one 0.1-unit triangle at z = far_z, behind the
    camera: the triangles' coordinate bound R_b becomes 4e4, which widens
    every box's padding, and the tree's exact stack bound becomes 26."""
    t2, q2, mats, tw, th, nm = helpers.mesh_plus_triangle(scenes.nature_mesh(), (0.0, 0.0, far_z), (0.1, 0.0, far_z),
                                                          (0.0, 0.1, far_z))
    if opaque:                          # every texel at alpha 1, no material index 3 / 4 override
        for k in range(len(mats)):
            mats[k].alpha = 1.0
        for k in range(len(q2)):
            if q2[k] in (3, 4):
                q2[k] = 0
    return helpers.SceneBundle(scenes.main_spheres(), (t2, q2, mats, tw, th, nm))


# ---- trees without binary16 nodes (tests/test_gpu_bvh_fallback.py) -------------
FAR = 2.0e5      # beyond binary16's 65504, inside the AO / zero-exit gates' 2^20


def with_far_triangle(mesh):
    """The mesh plus one small triangle at z = +FAR (behind the camera,
    outside the README box): it never changes a pixel, but its coordinates
    stop pack_bvh_h."""
    return helpers.mesh_plus_triangle(mesh, (0.0, 0.0, FAR), (1.0, 0.0, FAR), (0.0, 1.0, FAR))


def deep_far_scene():
    return helpers.SceneBundle(scenes.cornell_spheres(),
                               with_far_triangle(scenes.moved(scenes.load_tree_fixture(), scenes.TREE_MOVE)))


def shallow_far_scene():
    sph, mesh = scenes.synthetic_cornell(10, 100)
    return helpers.SceneBundle(sph, with_far_triangle(mesh))


# scene, params, kernel
FALLBACK = {
    "deep_far": (deep_far_scene, lambda: helpers.params(40, 30, 6, 8, use_ao=True, chunks=4), "render_kernel<BVH>"),
    "deep": (helpers.tree_scene, lambda: helpers.params(40, 30, 6, 8, use_ao=True, chunks=4),
             "render_kernel_q<QB=3,OP>"),
    "shallow_far": (shallow_far_scene, lambda: helpers.params(48, 36, 8, 6, chunks=4), "render_kernel_q<QB=4>"),
}

# ---- wide trees (tests/test_gpu_big_mesh.py, test_gpu_counters.py, test_cuda_semantics.py) ----
QB5, BVH32 = "render_kernel_q<QB=5>", "render_kernel<BVH32>"


@functools.lru_cache(maxsize=None)
def alpha_mesh():
    """66 248 triangles (above 65535: a wide tree) with a refracting (alpha
    0.5) texel and an alpha-0 hole, as the README box's floor.  Built once
    per process and shared: callers that change it take a copy
    (helpers.mesh_of)."""
    return scenes.heightfield_mesh(182, 1, 0.25, scenes.README_FLOOR, alpha=0.5)
