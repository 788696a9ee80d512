"""Host side of the forward pairs (rt_scene_prep.cpp pair_forward), CPU only.

After the small-sphere pairs the host looks, among the spheres that are left,
for pairs that a ray starting between them moves towards at most one of: two
disjoint spheres whose centres are nearly opposite (cosine <= -0.9) seen from
the centroid P of all other spheres' centres, with P outside both.  This is a
step of its own (pair_forward) that rt_scene_upload runs on what prepare_scene
gives; the probe test_scene_prep.py builds (tools/probes/scene_prep_check.cpp)
runs both when asked to, and the order and the two flag counts are read back
from its JSON line.
"""
import json
import os
import subprocess

import pytest

from test_scene_prep import checker, scene_text, README, M  # noqa: F401  (checker: the probe fixture)
import test_scene_prep


def run(checker, text, merge=None):
    """prepare_scene and pair_forward, as rt_scene_upload runs them."""
    env = {k: v for k, v in os.environ.items() if k != "RT_CAND_MERGE"}
    if merge:
        env["RT_CAND_MERGE"] = merge
    p = subprocess.run([checker, "64", "fwd"], input=text, capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


NAN = float("nan")
GREY = M((0.8, 0.8, 0.8))
LEFT, FLOOR, RIGHT, BACK, CEILING, MIRROR = 0, 1, 2, 7, 8, 9


def pairs(rec, lo, hi):
    order = rec["cand_orig"]["data"]
    return [tuple(order[k:k + 2]) for k in range(lo, hi, 2)]


def test_readme_box_wall_pairs(checker):
    rec = run(checker, scene_text(README))
    assert (rec["ns_merge"], rec["ns_fwd"]) == (4, 4)
    assert pairs(rec, 0, 4) == [(3, 6), (4, 5)]                       # the two small pairs, as before
    assert pairs(rec, 4, 8) == [(LEFT, RIGHT), (FLOOR, CEILING)]
    assert rec["cand_orig"]["data"][8:] == [BACK, MIRROR]             # unflagged, in the caller's order
    assert sorted(rec["cand_orig"]["data"]) == list(range(10))
    off = run(checker, scene_text(README), merge="off")
    assert rec["sph_cand"]["data"] == [off["sph_cand"]["data"][j] for j in rec["cand_orig"]["data"]]
    assert rec["sph_slot"]["data"] == [off["sph"]["data"][j] for j in rec["cand_orig"]["data"]]
    # the step only permutes the unflagged candidate records of prepare_scene's result
    prep = test_scene_prep.run(checker, scene_text(README))
    assert prep["ns_fwd"] == 0 and prep["cand_orig"]["data"][:4] == rec["cand_orig"]["data"][:4]
    for key in rec:
        if key not in ("ns_fwd", "cand_orig", "sph_cand", "sph_slot", "facts_bits"):
            assert rec[key] == prep[key], key


# Two radius-3 spheres on the x axis with two more on the z axis, whose centroid P = (0, 0.2, 0)
# lies between the first two and off their axis; (2, 3) become a small pair (x = 9/256).
def between(gap):
    return [((-3.0 - gap, 0.0, 0.0), 3.0, GREY), ((3.0 + gap, 0.0, 0.0), 3.0, GREY),
            ((0.0, 0.2, 8.0), 3.0, GREY), ((0.0, 0.2, -8.0), 3.0, GREY)]


def test_disjoint_spheres_around_the_centroid_pair(checker):
    rec = run(checker, scene_text(between(0.01)))
    assert (rec["ns_merge"], rec["ns_fwd"]) == (2, 2)
    assert pairs(rec, 0, 4) == [(2, 3), (0, 1)]


def test_touching_spheres_get_no_forward_pair(checker):
    rec = run(checker, scene_text(between(0.0)))                      # they touch at the origin, P is 0.2 off it
    assert (rec["ns_merge"], rec["ns_fwd"]) == (2, 0)
    assert rec["cand_orig"]["data"] == [2, 3, 0, 1]


def test_nested_spheres_get_no_forward_pair(checker):
    # the radius-4 sphere lies inside the radius-10 one; (2, 3) become a small pair (x = 16/576), and their
    # centroid P = (2.5, 0.1, 0) is between the two centres that are left, inside the large sphere
    rows = [((0.0, 0.0, 0.0), 10.0, GREY), ((5.0, 0.0, 0.0), 4.0, GREY),
            ((2.5, 0.1, 12.0), 4.0, GREY), ((2.5, 0.1, -12.0), 4.0, GREY)]
    rec = run(checker, scene_text(rows))
    assert (rec["ns_merge"], rec["ns_fwd"]) == (2, 0)
    assert rec["cand_orig"]["data"] == [2, 3, 0, 1]
    # ... and overlapping: the same spheres as the disjoint case, pushed into each other
    assert run(checker, scene_text(between(-0.5)))["ns_fwd"] == 0


def test_a_nan_centre_gets_no_pair(checker):
    rows = between(0.01) + [((NAN, 0.0, 0.0), 1.0, GREY)]
    rec = run(checker, scene_text(rows))
    assert (rec["ns_merge"], rec["ns_fwd"]) == (0, 0)
    assert rec["cand_orig"]["data"] == list(range(6))


@pytest.mark.parametrize("mode,want", [("fwd-all", (0, 10)), ("all", (10, 0)), ("off", (0, 0))])
def test_cand_merge_modes(checker, mode, want):
    rec = run(checker, scene_text(README), merge=mode)
    assert (rec["ns_merge"], rec["ns_fwd"]) == want
    assert rec["cand_orig"]["data"] == list(range(10))
