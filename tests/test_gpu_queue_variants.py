"""Every render_kernel_q instantiation, once: six (QB, OPQ) values x sky
off/on x AO off/on = 24 kernels (rt_kernels.hip with_queue_variant).

The host maps (qb, opq, sky, ao) to the instantiation in one place; each
case here renders a scene that plan_render sends to one of them, checks
rt_last_render_kernel's name and compares all four planes with the oracle
bit for bit.  The sky halves use sky_scene()'s enclosing sky sphere (the
last sphere, main.c:64-71) and texels with sky_mode 1.
"""
import pytest

import helpers
from tipe_rt import scenes
from tipe_rt.types import Sphere

from test_gpu_bvh_fallback import render_and_compare

pytestmark = pytest.mark.gpu

# one alpha-0.5 sphere in view: keeps the refraction code compiled in
TRANSPARENT = [((0.1, -0.9, -1.8), 0.3, scenes.material((0.8, 0.8, 0.8), alpha=0.5, ior=1.5))]


def tree_mesh():
    return scenes.moved(scenes.load_tree_fixture(), scenes.TREE_MOVE)


def pyramid_mesh():
    return scenes.moved(scenes.load_mesh_fixture("pyramide"), scenes.PYRAMID_MOVE)


# variant -> (expected kernel name, extra spheres, mesh or None); without sky
# these are cornell(), cornell() + the sphere, pyramid_scene(), tree_scene(),
# the tree + the sphere, and synthetic_cornell(10, 100)
VARIANTS = {
    "QB-2": ("render_kernel_q<QB=-2>", (), lambda: None),
    "QB-1": ("render_kernel_q<QB=-1>", TRANSPARENT, lambda: None),
    "QB0": ("render_kernel_q<QB=0>", (), pyramid_mesh),
    "QB3OP": ("render_kernel_q<QB=3,OP>", (), tree_mesh),
    "QB3": ("render_kernel_q<QB=3>", TRANSPARENT, tree_mesh),
    "QB4": ("render_kernel_q<QB=4>", (), lambda: scenes.synthetic_cornell(10, 100)[1]),
}


def bundle_of(extra, mesh, sky):
    spheres = scenes.cornell_spheres(extra=extra)
    if not sky:
        return helpers.SceneBundle(spheres, mesh)
    sk = helpers.sky_scene()
    n = len(spheres)
    sph = (Sphere * (n + 1))()
    for k in range(n):
        sph[k] = spheres[k]
    sph[n] = sk.spheres[len(sk.spheres) - 1]         # the sky sphere stays last
    return helpers.SceneBundle(sph, mesh, sky=sk.sky)


def variant_params(sky, ao):
    return helpers.params(24, 18, 4, 6, use_ao=ao, ao=2.5, chunks=2, sky_mode=1 if sky else 0)


@pytest.mark.parametrize("ao", [False, True], ids=["noao", "ao"])
@pytest.mark.parametrize("sky", [False, True], ids=["nosky", "sky"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_queue_variant(variant, sky, ao):
    name, extra, mesh = VARIANTS[variant]
    bundle = bundle_of(extra, mesh(), sky)
    kernel = render_and_compare(bundle, variant_params(sky, ao))
    assert kernel == name
