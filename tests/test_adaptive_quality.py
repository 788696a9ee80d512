"""Adaptive sampling's quality at an equal sample budget, measured: on the
64x48 frames and against the 2048-spp truth that test_vdenoise.py uses, the
RMSE of canva / 255 of an adaptive render at the default parameters is set
against uniform renders whose even sample count is the smallest one at or
above the adaptive frame's mean count.  The bar is the uniform frame's own
seed-to-seed spread m = (max - min) / mean of its RMSE over four seeds,
measured in the same run: adaptive <= uniform x (1 + m)."""
import functools

import numpy as np
import pytest

import helpers
import tipe_rt

SIZE = (64, 48)
SEEDS = (7, 8, 9, 10)


def bundle_of(scene):
    return helpers.cornell() if scene == "cornell" else helpers.pyramid_scene()


@functools.lru_cache(maxsize=None)
def converged(scene):
    """The 2048-spp canva at seed 1010."""
    return tipe_rt.render_rows(bundle_of(scene).scene, helpers.params(*SIZE, 2048, 6, seed=1010, chunks=1))[0]


def rmse(canva, truth):
    return float(np.sqrt(np.mean(((canva - truth) / 255.0) ** 2)))


def measure(scene, ap):
    """(adaptive RMSE, mean count, uniform count, uniform RMSEs per seed, share of pixels per round count)."""
    truth = converged(scene)
    bundle = bundle_of(scene)
    canva, _, _, rounds = tipe_rt.render_adaptive(bundle.scene, helpers.params(*SIZE, 1, 6, seed=SEEDS[0]), ap)
    counts = 2 * ap.first_half * 2.0 ** (rounds - 1)
    mean = float(counts.mean())
    S = int(np.ceil(mean / 2.0)) * 2
    uni = [rmse(tipe_rt.render_rows(bundle.scene, helpers.params(*SIZE, S, 6, seed=s, chunks=1))[0], truth)
           for s in SEEDS]
    hist = [float((rounds == k).mean()) for k in range(1, ap.max_rounds + 1)]
    return rmse(canva, truth), mean, S, uni, hist


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "pyramid"])
def test_adaptive_matches_uniform_at_an_equal_budget(scene):
    ap = tipe_rt.adaptive_params()
    got, mean, S, uni, hist = measure(scene, ap)
    u = float(np.mean(uni))
    m = (max(uni) - min(uni)) / u
    print("%s: adaptive RMSE %.5f at a mean of %.2f samples per pixel (rounds %s); uniform at %d spp: %s, mean %.5f, "
          "spread m = %.3f" % (scene, got, mean, ["%.3f" % h for h in hist], S, ["%.5f" % x for x in uni], u, m))
    assert got <= u * (1.0 + m), (got, u, m)
