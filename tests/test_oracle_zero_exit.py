"""The zero-throughput exit (rt.h rt_set_zero_throughput_exit) restated in
the oracle (rt_oracle.h oracle_set_zero_exit), on the CPU.

Inside the host's gates (rt_launch_plan.cpp set_gates: bounded materials,
with AO 0 < AO_intensity <= 1000 and coordinates within 2^20) leaving the
bounce loop at rayColor == (0, 0, 0) changes no plane, byte for byte, and only
removes work; outside them it changes the frame, which is why the gates exist.
tests/test_gpu_counters.py compares rt_count_async with these counters."""
import numpy as np
import pytest

import composition_cases
import helpers
import kernel_cases
import tipe_rt
from tipe_rt.types import (RT_CNT_SAMPLES, RT_CNT_CASTS, RT_CNT_SPHERE_TESTS, RT_CNT_SHADE, RT_CNT_RNG_DRAWS,
                           RT_CNT_EXACT_RESCANS)

PLANES = ("canva", "albedo", "normal", "radiance")


def _p(W=21, H=13, spp=4, bounces=6, **kw):
    kw.setdefault("compat", 0)
    return lambda: helpers.params(W, H, spp, bounces, **kw)


# name -> (scene, params): every kind of path end the exit can meet -- black
# diffuse lights, walls of disjoint colours, AO misses, texels, alpha holes,
# refraction, the sky sphere's emission
SCENES = {
    "box": (helpers.cornell, _p(32, 24, 8, 6)),
    "box_ao": (helpers.cornell, _p(32, 24, 8, 6, use_ao=True)),
    "pyramid_ao": (helpers.pyramid_scene, _p(use_ao=True)),
    "tree_ao": (helpers.tree_scene, _p(use_ao=True)),
    "sky": (helpers.sky_scene, _p(sky_mode=1)),
    "sky_tree": (helpers.sky_tree_scene, _p(sky_mode=1, use_ao=True)),
    "mineways": (helpers.mineways_scene, _p()),
    "alpha_half": (lambda: kernel_cases.one_transparent(0.5), _p()),
    "alpha_zero": (lambda: kernel_cases.one_transparent(0.0), _p()),
}


def both(bundle, p):
    """The same frame without and with the exit, counters included."""
    off = helpers.oracle_render(bundle, p, counters=True)
    on = helpers.oracle_render(bundle, p, counters=True, zero_exit=True)
    return off, on


def assert_exit_is_exact(off, on, what):
    for k in PLANES:
        assert on[k].tobytes() == off[k].tobytes(), "%s: %s differs with the exit on" % (what, k)
    c0, c1 = off["counters"], on["counters"]
    assert c1[RT_CNT_SAMPLES] == c0[RT_CNT_SAMPLES] > 0, what
    for k in (RT_CNT_CASTS, RT_CNT_SPHERE_TESTS, RT_CNT_SHADE, RT_CNT_RNG_DRAWS):
        assert c1[k] <= c0[k], (what, tipe_rt.COUNTER_NAMES[k], c1[k], c0[k])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_exit_changes_no_plane_and_only_removes_work(name):
    build, params = SCENES[name]
    off, on = both(build(), params())
    assert_exit_is_exact(off, on, name)
    print(name, "casts", off["counters"][RT_CNT_CASTS], "->", on["counters"][RT_CNT_CASTS])
    if name == "box":                   # black-diffuse light, green wall then red wall
        assert on["counters"][RT_CNT_CASTS] < off["counters"][RT_CNT_CASTS]


def inside_the_gates(p):
    """set_gates' AO condition on the value the tracer sees (rt.h
    compat_int_truncation); the random scenes' materials and coordinates are
    bounded by construction (helpers.random_scene, composition_cases._random)."""
    ao = float(int(p.AO_intensity)) if p.compat_int_truncation else p.AO_intensity
    return not p.useAO or 0.0 < ao <= 1000.0


RANDOM_PHILOX = [c.name for c in composition_cases.PHILOX_CASES if c.name.startswith("random_")]


@pytest.mark.parametrize("name", RANDOM_PHILOX)
def test_exit_is_exact_on_the_random_philox_cases(name):
    """composition_cases' random scenes (small frames, 0-24 bounces, aperture,
    textures, chunked sums) where the host would take the exit."""
    bundle, p = composition_cases.PHILOX_BY_NAME[name].scene()
    if not inside_the_gates(p):
        # outside the gate nothing is claimed; the run must still be well formed
        on = helpers.oracle_render(bundle, p, counters=True, zero_exit=True)
        assert on["counters"][RT_CNT_SAMPLES] == p.largeur_image * p.hauteur_image * p.nbRayonParPixel
        return
    off, on = both(bundle, p)
    assert_exit_is_exact(off, on, name)


def test_some_random_philox_case_is_inside_the_gates_with_ao():
    ps = [composition_cases.PHILOX_BY_NAME[n].scene()[1] for n in RANDOM_PHILOX]
    assert any(p.useAO and inside_the_gates(p) for p in ps)
    assert any(not p.useAO for p in ps)


def test_unbounded_emission_is_why_the_materials_gate_exists():
    """emissionStrength 1e308 x emission 100 overflows to inf; once rayColor
    is 0 the reference adds inf * 0 = NaN on every later hit of that light,
    and a path that left at rayColor == 0 does not: the frames differ, so the
    host must not take the exit here (SceneFacts::mats_bounded)."""
    spheres = tipe_rt.scenes.cornell_spheres()
    spheres[3].mat.emissionStrength = 1e308
    spheres[3].mat.emissionColor = tipe_rt.types.Vec3(100.0, 100.0, 100.0)
    bundle = helpers.SceneBundle(spheres)
    off, on = both(bundle, helpers.params(16, 12, 4, 6))
    nan_off, nan_on = int(np.isnan(off["radiance"]).sum()), int(np.isnan(on["radiance"]).sum())
    print("NaN radiance values: without the exit", nan_off, "with it", nan_on)
    assert nan_off > 0
    assert on["radiance"].tobytes() != off["radiance"].tobytes()
    assert nan_on != nan_off


@pytest.mark.parametrize("zero_exit", [False, True])
def test_counters_add_up_over_rows(zero_exit):
    """A sample's stream is keyed by its pixel, so the counters of one-row
    renders sum to the whole frame's: what lets a GPU count of any tiling be
    compared with the oracle's rows."""
    bundle = helpers.pyramid_scene()
    p = helpers.params(21, 13, 3, 6, use_ao=True, compat=0, chunks=4)
    whole = helpers.oracle_render(bundle, p, counters=True, zero_exit=zero_exit)["counters"]
    rows = sum(helpers.oracle_render(bundle, p, row_hi=j, row_lo=j, counters=True, zero_exit=zero_exit)["counters"]
               for j in range(13))
    assert list(rows) == list(whole)
    assert whole[RT_CNT_SAMPLES] == 21 * 13 * 3 and whole[RT_CNT_EXACT_RESCANS] == 0


def test_switch_is_off_by_default_and_after_a_call():
    bundle, p = helpers.cornell(), helpers.params(16, 12, 4, 6)
    first = helpers.oracle_render(bundle, p, counters=True)["counters"]
    on = helpers.oracle_render(bundle, p, counters=True, zero_exit=True)["counters"]
    again = helpers.oracle_render(bundle, p, counters=True)["counters"]
    assert list(first) == list(again)
    assert on[RT_CNT_CASTS] < first[RT_CNT_CASTS]


def test_cuda_semantics_ignore_the_switch():
    bundle = helpers.cornell()
    p = helpers.params(16, 12, 4, 6, use_ao=True, semantics=tipe_rt.types.RT_SEM_CUDA)
    off, on = both(bundle, p)
    assert list(on["counters"]) == list(off["counters"])
    for k in PLANES:
        assert on[k].tobytes() == off[k].tobytes()
