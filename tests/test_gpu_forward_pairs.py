"""Forward pairs of the sphere candidate pass (rt_spheres.h spheres_closest):
two spheres that a ray starting between them moves towards at most one of
share one root tail when no lane of the wave is live for both, a lane's sphere
being dead only when the certificate h > hmin, ca > -cmin proves that its tail
would write a sentinel.  Which pairs the host flags is a hint, so every scene
here must give the same bytes with the host's own flags (RT_CAND_MERGE unset),
with none (off), with every pair of the caller's order an r07 pair (all) and
with every pair a forward pair (fwd-all), and those bytes are the oracle's.
Each mode renders every scene in one fresh child process (this file run as a
script), which also runs rt_verify_sphere_pass on rays built around the
certificate's edges.

The verify case sets must not pass through the exact rescan: under the parent's
flags (off) at most 1 % of each set's rays may take it.  What makes a ray
rescan there: a sphere with |D| < 2^-36 Hs^2 (on a surface: h < 2^-18 Hs), a
winner within M = 2^-26 Hs of a * 1e-4, two candidates within 2M.  So the
surface sets leave at h / Hs from 2^-17.5 up (half of them in [2^-17.5, 2^-14],
around the certificate's hmin = 2^-16 Hs), and only 0.8 % of their rays
carry the cosines below that, down to 1e-12.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tipe-raytracer_amd")]
    import torch  # noqa: F401  (before librt_hip.so, as conftest.py does)

import helpers
import tipe_rt
from gpu_driver import assert_same_frame, gpu_render
from tipe_rt import scenes

pytestmark = pytest.mark.gpu

M = scenes.material
MODES = ["auto", "off", "all", "fwd-all"]
SCENES = ["readme", "outside_near", "outside_far", "below_floor", "overlap500", "three"]
PLANES = ("canva", "albedo", "normal")
W, H, SPP, BOUNCES = 48, 36, 8, 6
LMAX = 1004.0                                    # the README box's max |C| + R (its back wall)


def readme_rows():
    return [(c, r, M(d, e, es, rf)) for c, r, d, e, es, rf in scenes.README_SPHERES]


def scene_of(name):
    """(bundle, camera spec)"""
    cam = dict(scenes.README_CAMERA)
    small = [r for r in readme_rows() if r[1] != 500]
    if name == "readme":
        rows = readme_rows()
    elif name == "outside_near":                 # inside the left wall's sphere, 2 behind its face
        rows = readme_rows()
        cam["origin"] = (-3.0, 0.3, 0.5)
    elif name == "outside_far":                  # beyond the left wall's sphere: h < 0 for both walls
        rows = readme_rows()
        cam["origin"] = (-1100.0, 0.3, 0.5)
    elif name == "below_floor":                  # inside the (diffuse) floor's sphere: its bounces enter the box
        rows = readme_rows()
        cam["origin"] = (0.34, -3.0, 0.5)
    elif name == "overlap500":                   # the camera inside the overlap |x| < 100 of two radius-500 spheres
        rows = [((-400, 0, 0), 500, M((0.8, 0.3, 0.3))), ((400, 0, 0), 500, M((0.3, 0.3, 0.8), refl=0.5))] + small
    elif name == "three":                        # odd count: a padding record
        rows = [((0, -501, 0), 500, M((0.8, 0.8, 0.8))), ((0, 501, 0), 500, M((0.8, 0.8, 0.8), refl=0.9)),
                ((-0.5, 0.2, -2.0), 0.5, M((0, 0, 0), (1.0, 0.6, 0.2), 4.0))]
    else:
        raise KeyError(name)
    return helpers.SceneBundle(helpers.sphere_array(rows)), cam


def params_of(cam):
    return helpers.params(W, H, SPP, BOUNCES, chunks=32, cam=helpers.camera_of(cam))


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def leaving(rng, nrm, rho, hs, R):
    """Unit directions leaving a surface with normal nrm at h = rho * hs (cosine rho * hs / R, at most 1)."""
    cosv = np.minimum(rho * hs / R, 1.0)[:, None]
    tan = unit(np.cross(nrm, rng.normal(size=nrm.shape)))
    return cosv * nrm + np.sqrt(np.maximum(1.0 - cosv * cosv, 0.0)) * tan


def rho_main(rng, m, R, hs):
    """h / Hs: half around the certificate's edge, half up to cosine 1."""
    top = np.log2(R / hs)
    return 2.0 ** np.where(rng.random(m) < 0.5, rng.uniform(-17.5, -14.0, m), rng.uniform(-17.5, top, m))


def verify_sets(spheres):
    """{name: rays (n, 6)} -- about 2e5 rays in all, on the README box."""
    rng = np.random.default_rng(808)
    C_ = np.array([[s.center.e[0], s.center.e[1], s.center.e[2]] for s in spheres])
    R_ = np.array([s.radius for s in spheres])
    m = 50_000
    out = {}
    # origins on a surface, leaving; 0.8 % at the cosines below the grazing band's edge, down to 1e-12
    k = rng.integers(0, len(R_), m)
    nrm = unit(rng.normal(size=(m, 3)))
    o = C_[k] + R_[k, None] * nrm
    hs = np.abs(o).sum(axis=1) + LMAX
    rho = rho_main(rng, m, R_[k], hs)
    low = rng.random(m) < 0.008
    rho = np.where(low, 10.0 ** rng.uniform(-12.0, np.log10(2.0 ** -18.5 * hs / R_[k])) * R_[k] / hs, rho)
    out["surface"] = np.concatenate([o, leaving(rng, nrm, rho, hs, R_[k])], axis=1)
    # origins 1e-9 inside and outside a surface: leaving, and any direction
    k = rng.integers(0, len(R_), m)
    nrm = unit(rng.normal(size=(m, 3)))
    o = C_[k] + (R_[k] + rng.choice([-1e-9, 1e-9], m))[:, None] * nrm
    hs = np.abs(o).sum(axis=1) + LMAX
    d = np.where(rng.random((m, 1)) < 0.7, leaving(rng, nrm, rho_main(rng, m, R_[k], hs), hs, R_[k]),
                 unit(rng.normal(size=(m, 3))))
    out["near_surface"] = np.concatenate([o, d], axis=1)
    # the exact centre between two spheres, directions in the bisecting plane and a little off it
    # (disjoint spheres only: at the centre between two overlapping walls a direction in the bisecting
    # plane leaves both at the same t, two candidates within 2M, which is the rescan's case by design)
    i, j = rng.integers(0, len(R_), (2, 4 * m))
    disjoint = np.linalg.norm(C_[i] - C_[j], axis=1) > R_[i] + R_[j]
    i, j = i[disjoint][:m], j[disjoint][:m]
    o = 0.5 * (C_[i] + C_[j])
    axis = unit(C_[j] - C_[i])
    perp = unit(np.cross(axis, rng.normal(size=axis.shape)))
    off = rng.choice([0.0, 1e-12, 1e-9, 1e-6, 1e-4, 1e-2], len(i))[:, None] * rng.choice([-1.0, 1.0], (len(i), 1))
    out["bisecting"] = np.concatenate([o, perp + off * axis], axis=1)
    # a = |d|^2 from 2^-20 to 2^20, origins inside the box away from every surface
    o = rng.uniform([-0.95, -0.95, -3.9], [0.95, 0.95, 0.4], (2 * m, 3))
    clear = np.all(np.linalg.norm(o[:, None, :] - C_[None, :, :], axis=2) - R_[None, :] > 0.1, axis=1)
    o = o[clear][:m]
    d = unit(rng.normal(size=o.shape)) * 2.0 ** rng.uniform(-10.0, 10.0, (len(o), 1))
    out["scaled"] = np.concatenate([o, d], axis=1)
    return out


def child(mode, path):
    """One mode: every scene's planes and the verify counts of every case set, into path (npz)."""
    if mode != "auto":
        os.environ["RT_CAND_MERGE"] = mode
    else:
        os.environ.pop("RT_CAND_MERGE", None)
    out = {}
    for name in SCENES:
        b, cam = scene_of(name)
        got = gpu_render(b, params_of(cam), radiance=False)
        for plane, arr in zip(PLANES, got):
            out["%s/%s" % (name, plane)] = arr
    b, _ = scene_of("readme")
    for name, rays in verify_sets(b.spheres).items():
        out["verify/" + name] = np.array(tipe_rt.verify_sphere_pass(b.scene, rays) + (len(rays),), dtype=np.int64)
    np.savez(path, **out)


@pytest.fixture(scope="module")
def by_mode(tmp_path_factory):
    d = tmp_path_factory.mktemp("fwd_pairs")
    res = {}
    for mode in MODES:
        path = str(d / ("%s.npz" % mode))
        env = {k: v for k, v in os.environ.items() if k != "RT_CAND_MERGE"}
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, path], capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 0, "mode %s: %s" % (mode, r.stderr[-3000:])
        res[mode] = dict(np.load(path))
    return res


@pytest.fixture(scope="module")
def oracle_planes():
    ref = {}
    for name in SCENES:
        b, cam = scene_of(name)
        ref[name] = helpers.oracle_render(b, params_of(cam))
    return ref


def planes_of(npz, name):
    return [npz["%s/%s" % (name, plane)] for plane in PLANES]


@pytest.mark.parametrize("name", SCENES)
def test_modes_give_the_same_bytes(name, by_mode):
    for mode in MODES[1:]:
        assert_same_frame(planes_of(by_mode[mode], name), planes_of(by_mode["auto"], name),
                          "%s, %s vs auto:" % (name, mode), PLANES, same_bytes=True)


@pytest.mark.parametrize("name", SCENES)
def test_bytes_are_the_oracles(name, by_mode, oracle_planes):
    ref = oracle_planes[name]
    if name == "readme":
        assert ref["canva"].max() > 0
    for mode in MODES:
        assert_same_frame(planes_of(by_mode[mode], name), ref, "%s, %s:" % (name, mode), PLANES, same_bytes=True)


@pytest.mark.parametrize("case", ["surface", "near_surface", "bisecting", "scaled"])
def test_verify_sphere_pass_on_certificate_rays(case, by_mode):
    fb_off, bad_off, n = (int(x) for x in by_mode["off"]["verify/" + case])
    print("%s: %d rays, exact rescans %s" % (case, n, {m: int(by_mode[m]["verify/" + case][0]) for m in MODES}))
    assert n >= 40_000
    assert fb_off <= 0.01 * n, "the case set leans on the exact rescan: %d of %d under the parent's flags" % (fb_off, n)
    for mode in MODES:
        fb, bad, n_mode = (int(x) for x in by_mode[mode]["verify/" + case])
        assert n_mode == n and bad == 0, (case, mode, bad)
        assert fb <= 0.01 * n, (case, mode, fb)


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
