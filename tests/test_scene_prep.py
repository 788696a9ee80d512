"""Host check of the scene preparation (rt_scene_prep.cpp prepare_scene), CPU only.

Everything rt_scene_upload copies to the device is prepared by one pure host
function: the candidate records and their pairing order (pair_candidates),
cand_lmax, the per-triangle precomputation and the affine texel map
(tri_uv_affine), tex0, the BVH reorder and the bounds and flags the launch
gates read.  tools/probes/scene_prep_check.cpp reads a scene as text, calls
prepare_scene and prints the SceneFacts fields and the arrays as one JSON line;
this test builds it with g++ and checks the cases below.  The expected pairing
orders follow the two rules in pair_candidates' comment.  Flagged pairs: among
the spheres of smallest radius, in ascending radius (ties by index), each
unpaired sphere takes the unpaired partner with the smallest
x = (max(R_i, R_j) / d)^2 and the pair is flagged when x <= 1/16.  Forward
pairs, among the spheres that are left: two disjoint spheres whose centres are
nearly opposite (cosine <= -0.9) seen from the centroid P of all other spheres'
centres, with P outside both.  The other spheres follow in the caller's order.
"""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from tipe_rt import scenes
from tipe_rt.types import Triangle, UV, Vec3, Material

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tipe-raytracer_amd", "csrc")
INF = float("inf")
M = scenes.material


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("prep") / "scene_prep_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    "-o", exe, os.path.join(ROOT, "tools", "probes", "scene_prep_check.cpp"),
                    os.path.join(CSRC, "rt_scene_prep.cpp"), os.path.join(CSRC, "rt_bvh.cpp")], check=True)
    return exe


def fmt(*xs):
    return " ".join(float(x).hex() for x in xs)


def mat_text(m):
    return fmt(*m.diffuseColor.e, *m.emissionColor.e, m.emissionStrength, m.reflectionStrength, m.alpha,
               m.materialIndex)


def scene_text(spheres=(), mesh=None, sky=None):
    """spheres: (center, radius, Material) rows; mesh: scenes' mesh tuple; sky: (w, h, materials)."""
    out = ["spheres %d" % len(spheres)]
    out += ["%s %s" % (fmt(*c, r), mat_text(m)) for c, r, m in spheres]
    if mesh is not None:
        tris, qm, mats, tw, th, nm = mesh
        out.append("triangles %d %d %d %d" % (len(tris), tw, th, nm))
        for k, t in enumerate(tris):
            out.append("%s %d %s" % (fmt(*t.A.e, *t.B.e, *t.C.e, t.uvA.u, t.uvA.v, t.uvB.u, t.uvB.v, t.uvC.u, t.uvC.v),
                                     qm[k], mat_text(t.mat)))
        out.append("texels %d" % len(mats))
        out += [mat_text(m) for m in mats]
    if sky is not None:
        out.append("sky %d %d" % sky[:2])
        out += [mat_text(m) for m in sky[2]]
    return "\n".join(out) + "\n"


def run(checker, text, merge=None, limit=64):
    env = {k: v for k, v in os.environ.items() if k != "RT_CAND_MERGE"}
    if merge:
        env["RT_CAND_MERGE"] = merge
    p = subprocess.run([checker, str(limit)], input=text, capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


def rows_of(array):
    return [(tuple(s.center.e), s.radius, s.mat) for s in array]


README = rows_of(scenes.cornell_spheres())
ODD_COUNT = README + [((-0.3, 0.3, -2.0), 0.3, M((0, 1, 0), refl=0.5))]          # test_gpu_merged_tail.py's
SMALL_ONLY = [r for r in README if r[1] != 500] + [((0.0, 0.2, -2.0), 0.3, M((0.8, 0.8, 0.8)))]


def check_order(checker, rows, rec, order, ns_merge, ns_fwd):
    ns, ns_pad = len(rows), (len(rows) + 1) & ~1
    assert (rec["ns"], rec["ns_pad"], rec["ns_merge"], rec["ns_fwd"]) == (ns, ns_pad, ns_merge, ns_fwd)
    assert rec["cand_orig"]["data"] == order and sorted(order) == list(range(ns_pad))
    # sph in the caller's order (r2 = radius^2, the padding's -inf)
    want = [[*c, r * r] for c, r, _ in rows] + [[0.0, 0.0, 0.0, -INF]] * (ns_pad - ns)
    assert rec["sph"]["data"] == want
    assert rec["sph_slot"]["data"] == [want[j] for j in order]
    # the candidate records are the by-sphere records (RT_CAND_MERGE=off keeps them in place), permuted;
    # the pairing changes nothing else
    off = run(checker, scene_text(rows), merge="off")
    by_sphere = off["sph_cand"]["data"]
    assert (off["ns_merge"], off["ns_fwd"]) == (0, 0) and off["cand_orig"]["data"] == list(range(ns_pad))
    assert rec["sph_cand"]["data"] == [by_sphere[j] for j in order]
    assert off["sph_slot"]["data"] == want
    for key in rec:
        if key not in ("ns_merge", "ns_fwd", "cand_orig", "sph_cand", "sph_slot", "facts_bits"):
            assert rec[key] == off[key], key
    for (c, r, _), k in zip(rows, by_sphere):
        assert k[:3] == list(c) and k[3] == pytest.approx(sum(x * x for x in c) - r * r, rel=1e-12, abs=1e-12)
    if ns < ns_pad:
        assert by_sphere[ns] == [0.0, 0.0, 0.0, INF]


def pair_x(rows, i, j):
    d2 = sum((a - b) ** 2 for a, b in zip(rows[i][0], rows[j][0]))
    return max(rows[i][1], rows[j][1]) ** 2 / d2


NAN = float("nan")
GREY = M((0.8, 0.8, 0.8))
LEFT, FLOOR, RIGHT, BACK, CEILING, MIRROR = 0, 1, 2, 7, 8, 9


def pairs(rec, lo, hi):
    order = rec["cand_orig"]["data"]
    return [tuple(order[k:k + 2]) for k in range(lo, hi, 2)]


def test_readme_box_pairs(checker):
    rec = run(checker, scene_text(README))
    check_order(checker, README, rec, [3, 6, 4, 5, 0, 2, 1, 8, 7, 9], 4, 4)
    assert pair_x(README, 3, 6) == pytest.approx(0.0218, abs=5e-5)
    assert pair_x(README, 4, 5) == pytest.approx(0.0269, abs=5e-5)
    assert math.isfinite(rec["cand_lmax"]) and rec["cand_lmax"] >= 1004.0
    assert rec["sph_bound"] == 1004.0 and rec["coord_max"] == 1004.0
    assert rec["mats_bounded"] and rec["sph_opaque"] and rec["nt"] == 0 and rec["bvh_nodes"] == 0


def test_odd_count_shares_the_padding(checker):
    rec = run(checker, scene_text(ODD_COUNT))
    check_order(checker, ODD_COUNT, rec, [10, 5, 3, 6, 4, 9, 0, 11, 1, 8, 2, 7], 8, 2)
    slot = rec["cand_orig"]["data"].index(11)
    assert rec["sph_cand"]["data"][slot][3] == INF and rec["sph"]["data"][11][3] == -INF


def test_small_only_flags_every_pair(checker):
    check_order(checker, SMALL_ONLY, run(checker, scene_text(SMALL_ONLY)), [5, 3, 0, 2, 1, 4], 6, 0)


def test_readme_box_wall_pairs(checker):
    rec = run(checker, scene_text(README))
    assert (rec["ns_merge"], rec["ns_fwd"]) == (4, 4)
    assert pairs(rec, 0, 4) == [(3, 6), (4, 5)]                       # the two small pairs come first
    assert pairs(rec, 4, 8) == [(LEFT, RIGHT), (FLOOR, CEILING)]
    assert rec["cand_orig"]["data"][8:] == [BACK, MIRROR]             # unflagged, in the caller's order
    assert sorted(rec["cand_orig"]["data"]) == list(range(10))
    # against the unpaired run: the records are its records permuted by cand_orig, nothing else differs
    off = run(checker, scene_text(README), merge="off")
    assert rec["sph_cand"]["data"] == [off["sph_cand"]["data"][j] for j in rec["cand_orig"]["data"]]
    assert rec["sph_slot"]["data"] == [off["sph_slot"]["data"][j] for j in rec["cand_orig"]["data"]]
    assert off["sph_slot"]["data"] == off["sph"]["data"]
    for key in rec:
        if key not in ("ns_merge", "ns_fwd", "cand_orig", "sph_cand", "sph_slot", "facts_bits"):
            assert rec[key] == off[key], key


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


def forty_spheres():
    """Six radius-500 walls around 34 small spheres of radius 0.2 to 0.8: more than kMergeScan (32) spheres."""
    state = [20260101]

    def rnd():                                   # a 31-bit LCG: the scene does not depend on a library's stream
        state[0] = (state[0] * 1103515245 + 12345) % (1 << 31)
        return state[0] / float(1 << 31)

    rows, walls = [], 0
    for i in range(40):
        if i % 7 == 3 and walls < 6:
            c = [0.0, 0.0, 0.0]
            c[walls // 2] = 504.0 if walls % 2 else -504.0
            rows.append((tuple(c), 500.0, GREY))
            walls += 1
        else:
            rows.append((tuple(round(8.0 * rnd() - 4.0, 3) for _ in range(3)), (0.2, 0.3, 0.5, 0.8)[int(4 * rnd())], GREY))
    return rows


def test_more_spheres_than_the_scan_looks_at(checker):
    # 34 small spheres, of which the flagged-pair rule scans the 32 smallest: 27 and 29 (radius 0.8) stay
    # unflagged.  The expected order and counts were recorded from the two-step host code this step replaced
    # (prepare_scene, then pair_forward), not from pair_candidates.
    rows = forty_spheres()
    assert len(rows) == 40 and sum(r == 500.0 for _, r, _ in rows) == 6
    rec = run(checker, scene_text(rows))
    check_order(checker, rows, rec,
                [6, 16, 8, 19, 21, 30, 23, 11, 33, 28, 5, 20, 7, 25, 12, 32, 18, 0, 36, 14, 1, 4, 9, 13, 15, 34, 35, 26,
                 37, 22, 3, 10, 17, 24, 31, 38, 2, 39, 27, 29], 30, 8)


@pytest.mark.parametrize("mode,rows", [("all", README), ("off", README), ("all", ODD_COUNT), ("off", ODD_COUNT)])
def test_cand_merge_override_keeps_the_callers_order(checker, mode, rows):
    rec = run(checker, scene_text(rows), merge=mode)
    ns_pad = (len(rows) + 1) & ~1
    assert rec["cand_orig"]["data"] == list(range(ns_pad))
    assert rec["ns_merge"] == (ns_pad if mode == "all" else 0)
    assert rec["ns_fwd"] == 0


@pytest.mark.parametrize("mode,want", [("fwd-all", (0, 10)), ("all", (10, 0)), ("off", (0, 0))])
def test_cand_merge_modes(checker, mode, want):
    rec = run(checker, scene_text(README), merge=mode)
    assert (rec["ns_merge"], rec["ns_fwd"]) == want
    assert rec["cand_orig"]["data"] == list(range(10))


@pytest.mark.parametrize("extra,sph_bound", [
    (((0.3, 0.2, -2.0), INF), INF),
    # std::max drops the NaN term: the other two coordinates give 2.3, below the walls' 1004
    (((float("nan"), 0.2, -2.0), 0.3), 1004.0),
])
def test_non_finite_sphere_switches_the_pass_off(checker, extra, sph_bound):
    rows = README + [(extra[0], extra[1], M((1, 0, 0)))]
    rec = run(checker, scene_text(rows))
    assert rec["ns_merge"] == 0 and rec["ns_fwd"] == 0 and rec["cand_orig"]["data"] == list(range(12))
    assert rec["cand_lmax"] == INF and rec["coord_max"] == INF
    assert rec["sph_bound"] == sph_bound


@pytest.mark.parametrize("n,finite", [(65535, False), (65534, True)])
def test_cand_lmax_by_sphere_count(checker, n, finite):
    line = "%s %s\n" % (fmt(0.0, 0.0, -3.0, 1.0), mat_text(M((1, 1, 1))))
    rec = run(checker, "spheres %d\n" % n + line * n)
    assert rec["ns"] == n and rec["sph_cand"]["n"] == (n + 1) & ~1
    assert math.isfinite(rec["cand_lmax"]) == finite
    if finite:
        assert 4.0 <= rec["cand_lmax"] <= 4.0 * (1 + 1e-9)


def soup(n, seed, uv=True, nm=2, tw=2, th=2):
    rng = np.random.default_rng(seed)
    tris, qm = (Triangle * n)(), []
    for k in range(n):
        a = rng.uniform(-1, 1, 3)
        tris[k].A, tris[k].B, tris[k].C = Vec3(*a), Vec3(*(a + 0.2 * rng.normal(size=3))), Vec3(*(a + 0.2 * rng.normal(size=3)))
        if uv:
            tris[k].uvA, tris[k].uvB, tris[k].uvC = (UV(*rng.uniform(0, 1, 2)) for _ in range(3))
        tris[k].mat = M(tuple(rng.uniform(0, 1, 3)), refl=float(k))
        qm.append(int(rng.integers(0, nm)))
    mats = (Material * (nm * tw * th))()
    for i in range(len(mats)):
        mats[i] = M(tuple(rng.uniform(0.2, 0.9, 3)))
    return tris, qm, mats, tw, th, nm


def check_triangle_rows(rec, mesh, orig):
    tris, qm = mesh[0], mesh[1]
    for k, o in enumerate(orig):
        t = tris[o]
        A, B, Cv = np.array(t.A.e[:]), np.array(t.B.e[:]), np.array(t.C.e[:])
        assert rec["tri"]["data"][k][:9] == [*A, *(B - A), *(Cv - A)]
        x = rec["tri_tex"]["data"][k]
        assert x[:12] == [*B, *Cv, t.uvA.u, t.uvA.v, t.uvB.u, t.uvB.v, t.uvC.u, t.uvC.v] and x[12] == qm[o]
        assert rec["tri_mat"]["data"][k] == [*t.mat.diffuseColor.e, *t.mat.emissionColor.e, t.mat.emissionStrength,
                                             t.mat.reflectionStrength, t.mat.alpha, t.mat.materialIndex]


def test_bvh_reorders_the_triangle_arrays(checker):
    mesh = soup(40, 11)
    rec = run(checker, scene_text(README, mesh))
    assert rec["nt"] == 40 and rec["bvh_nodes"] > 0 and rec["bvh"]["n"] == rec["bvh_nodes"]
    orig = rec["tri_orig"]["data"]
    assert sorted(orig) == list(range(40)) and orig != list(range(40))
    check_triangle_rows(rec, mesh, orig)
    assert rec["tri_uv"]["n"] == 40 and not rec["all_tex0"]
    assert rec["bvh_rbox"] >= 1.0 and rec["r_scene"] >= 1.0 and rec["bvh_stack4"] >= 1


def test_few_triangles_without_uv(checker):
    mesh = soup(5, 12, uv=False, nm=3)
    mesh[1][:] = [0, 1, 2, 5, -1]            # (5 and -1 are outside the table: the index is clamped into it)
    rec = run(checker, scene_text(README, mesh))
    assert rec["bvh_nodes"] == 0 and rec["tri_orig"]["n"] == 0 and rec["bvh"]["n"] == 0 and rec["bvhh"]["n"] == 0
    check_triangle_rows(rec, mesh, range(5))
    assert [x[13] for x in rec["tri_tex"]["data"]] == [0, 4, 8, 11, 0]
    assert rec["all_tex0"] and rec["tri_uv"]["n"] == 0
    assert (rec["tw"], rec["th"], rec["n_texels"]) == (2, 2, 12)


def test_zero_area_triangle_has_no_affine_map(checker):
    mesh = soup(5, 13)
    mesh[0][2].B = mesh[0][2].A
    rec = run(checker, scene_text(README, mesh))
    diam = [x[10] for x in rec["tri_uv"]["data"]]
    assert [d < 0 for d in diam] == [False, False, True, False, False]
    assert [x[13] for x in rec["tri_tex"]["data"]] == [-1] * 5


def test_texel_table_of_2_to_31_is_refused_unread(checker):
    t = Triangle()
    t.B, t.C = Vec3(1, 0, 0), Vec3(0, 1, 0)
    rec = run(checker, scene_text(README, ([t], [0], [M((1, 1, 1))], 65536, 32768, 1)))
    assert rec == {"rc": -4, "error": "2147483648 texels >= 2^31"}


def test_opacity_and_bounded_flags(checker):
    base = run(checker, scene_text(README, soup(5, 14)))
    assert base["sph_opaque"] and base["tri_opaque"] and base["mats_bounded"]
    rec = run(checker, scene_text(README + [((0.0, 0.0, -2.0), 0.2, M((1, 1, 1), alpha=0.5))], soup(5, 14)))
    assert not rec["sph_opaque"] and rec["tri_opaque"] and rec["mats_bounded"]
    mesh = soup(5, 14, nm=4)
    mesh[1][:] = [0, 1, 2, 3, 0]
    rec = run(checker, scene_text(README, mesh))
    assert rec["sph_opaque"] and not rec["tri_opaque"] and rec["mats_bounded"]
    mesh = soup(5, 14)
    mesh[2][3] = M((1e200, 0.5, 0.5))
    rec = run(checker, scene_text(README, mesh))
    assert rec["sph_opaque"] and rec["tri_opaque"] and not rec["mats_bounded"]
