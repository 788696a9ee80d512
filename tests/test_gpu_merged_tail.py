"""The sphere candidate pass's merged root tail (rt_spheres.h spheres_closest):
a flagged pair of spheres runs one tail in the wave-casts in which no lane's
line crosses both, two otherwise.  Which pairs the host flags
(rt_scene_prep.cpp order_candidates) is a hint, so every scene here must stay bit
for bit on the oracle with the host's own flags and with every pair flagged
in the caller's order (RT_CAND_MERGE=all), on the queue kernel
(spp_chunks 32) and on the fixed grid (spp_chunks 1; both carry the
flagged-pair loop in sphere scenes); rt_verify_sphere_pass runs the pass
against the plain exact scan on stress rays of each scene.
"""
import numpy as np
import pytest

import helpers
import tipe_rt
from gpu_driver import check_parity
from helpers import stress_rays
from tipe_rt import scenes

pytestmark = pytest.mark.gpu

M = scenes.material
WALLS = [r for r in scenes.README_SPHERES if r[1] == 500]
SMALL = [r for r in scenes.README_SPHERES if r[1] != 500]
CAM_O = np.array(scenes.README_CAMERA["origin"], dtype=np.float64)
AXIS = np.array(scenes.README_CAMERA["target"], dtype=np.float64) - CAM_O
AXIS /= np.linalg.norm(AXIS)


def bundle_of(rows):
    return helpers.SceneBundle(helpers.sphere_array(rows))


def readme_rows(rows, wall_refl=None):
    return [(c, r, M(d, e, es, rf if wall_refl is None or r != 500 else wall_refl)) for c, r, d, e, es, rf in rows]


LIGHT = M((0, 0, 0), (1.0, 0.6, 0.2), 4.0)
RED, GREEN, GREY = M((1, 0, 0)), M((0, 1, 0), refl=0.5), M((0.8, 0.8, 0.8))


def scene_rows(name):
    walls = readme_rows(WALLS)
    lamp = ((-0.5, 1.4, -1.2), 0.5, LIGHT)
    if name == "readme":
        return readme_rows(scenes.README_SPHERES)
    if name == "behind":          # one behind the other on the camera axis: the lanes at the centre cross both
        return walls + [lamp, (CAM_O + 2.0 * AXIS, 0.2, RED), (CAM_O + 3.2 * AXIS, 0.2, GREEN),
                        ((0.6, -0.6, -2.0), 0.2, GREY)]
    if name == "overlap":
        return walls + [lamp, ((0.0, -0.3, -2.0), 0.4, RED), ((0.3, -0.3, -2.1), 0.4, GREEN)]
    if name == "duplicates":      # equal t: the reference keeps the first
        return walls + [lamp, ((0.3, 0.2, -2.5), 0.3, RED), ((0.3, 0.2, -2.5), 0.3, GREEN),
                        ((-0.5, -0.5, -1.5), 0.3, GREY)]
    if name == "radii_1e-12":
        return walls + [lamp, ((-0.4, 0.1, -2.0), 0.25, RED), ((-0.4, 0.1, -2.0), 0.25 + 1e-12, GREEN),
                        ((0.5, -0.5, -1.5), 0.3, GREY)]
    if name == "touching":        # each other and the floor (y = -1)
        return walls + [lamp, ((0.0, -0.5, -1.8), 0.5, M((0.9, 0.9, 0.9), refl=0.9)),
                        ((0.5, -0.5, -1.8), 0.5, M((0.2, 0.8, 0.5)))]
    if name == "camera_inside":   # the second root wins on every ray
        return walls + [lamp, (CAM_O, 0.4, M((0.8, 0.8, 0.8), (1, 1, 1), 0.5)), ((0.0, -0.5, -3.0), 0.3, RED)]
    if name == "odd_count":       # 11 records + the padding
        return readme_rows(scenes.README_SPHERES) + [((-0.3, 0.3, -2.0), 0.3, GREEN)]
    if name == "small_only":      # every pair is flagged
        return readme_rows(SMALL) + [((0.0, 0.2, -2.0), 0.3, GREY)]
    if name == "reflective":      # rs 0.96 walls: lerped, non-unit directions over 6 bounces
        return readme_rows(scenes.README_SPHERES, wall_refl=0.96)
    raise KeyError(name)


SCENES = ["readme", "behind", "overlap", "duplicates", "radii_1e-12", "touching", "camera_inside", "odd_count",
          "small_only", "reflective"]
# the host's own flags on both kernels; every pair flagged on the queue kernel, and on the
# fixed grid for the README box
MODES = [("auto", 1), ("auto", 32), ("all", 32)]


@pytest.mark.parametrize("mode,chunks", MODES + [("all", 1)])
def test_readme_box(mode, chunks, monkeypatch):
    if mode != "auto":
        monkeypatch.setenv("RT_CAND_MERGE", mode)
    check_parity(bundle_of(scene_rows("readme")), helpers.params(32, 24, 8, 6, chunks=chunks))


@pytest.mark.parametrize("mode,chunks", MODES)
@pytest.mark.parametrize("name", SCENES[1:])
def test_merged_tail_scene(name, mode, chunks, monkeypatch):
    if mode != "auto":
        monkeypatch.setenv("RT_CAND_MERGE", mode)
    ref = check_parity(bundle_of(scene_rows(name)), helpers.params(32, 24, 8, 6, chunks=chunks))
    assert ref["canva"].max() > 0


@pytest.mark.parametrize("mode", ["auto", "all"])
@pytest.mark.parametrize("name", SCENES)
def test_verify_sphere_pass(name, mode, monkeypatch):
    if mode != "auto":
        monkeypatch.setenv("RT_CAND_MERGE", mode)
    b = bundle_of(scene_rows(name))
    rays = stress_rays(b.spheres, 300_000, 11)
    # rays along the camera axis and through pairs of centres: lines that cross two spheres
    rng = np.random.default_rng(12)
    C_ = np.array([[s.center.e[0], s.center.e[1], s.center.e[2]] for s in b.spheres])
    i, j = rng.integers(0, len(C_), (2, 50_000))
    o = C_[i] + (C_[i] - C_[j]) * rng.uniform(0.0, 2.0, (50_000, 1)) + rng.normal(0, 1e-3, (50_000, 3))
    through = np.concatenate([o, C_[j] - o + rng.normal(0, 1e-2, (50_000, 3))], axis=1)
    through = through[np.isfinite(through).all(axis=1)]
    fb, bad = tipe_rt.verify_sphere_pass(b.scene, np.concatenate([rays, through]))
    assert bad == 0
    assert fb < len(rays)
