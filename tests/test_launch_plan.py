"""Host check of the launch plan (rt_launch_plan.cpp fill_kparams + plan_render), CPU only.

Which kernel a scene renders with is decided on the host, once per launch:
queue or fixed grid, the queue kernel's (QB, OPQ) instantiation, the BVH stack
that instantiation has, the row bands and their partial-sum bytes.  A scene
that falls to a slower instantiation loses rate silently, so the decision is
checked here without a GPU.  tools/probes/launch_plan_check.cpp prepares a scene
given as text, fills the launch descriptor for each `params` section and prints
the plans; a `facts` section gives the scalars the plan depends on directly, so
every boundary is hit exactly.

The scene cases are the (scene, params, kernel name) triples the GPU tests
assert on the device, from tests/kernel_cases.py.  The scalar cases follow
the rule in plan_render's comment: a narrow tree takes QB 4 (14 stack entries)
when its bound fits, no origin is far and it is shallow or has no 64-byte
nodes; else QB 3 over the 64-byte nodes (32 entries; OPQ, 24, when every
material is opaque, the bound fits and no origin is far); else the fixed grid
(48).  A wide tree takes QB 5 (32) or the fixed grid's wide kernel.

Name and stack of a queue plan come from one table (rt_queue_variants.h), which
the device code sizes its stacks by too; the checker prints it, and every queue
plan any case here gets is compared with its row.
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import composition_cases as cc
import helpers
import kernel_cases as kc
from tipe_rt import scenes
from tipe_rt.types import RT_SEM_CUDA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tipe-raytracer_amd", "csrc")
SRC = [os.path.join(ROOT, "tools", "probes", "launch_plan_check.cpp")] + \
      [os.path.join(CSRC, f) for f in ("rt_scene_prep.cpp", "rt_launch_plan.cpp", "rt_bvh.cpp")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "launch_plan_check")
    subprocess.run(["g++", "-O2"] + FLAGS + ["-o", exe] + SRC, check=True)
    return exe


def rows_text(a):
    return "\n".join(" ".join(map(repr, row)) for row in a.tolist()) + "\n"


def doubles(array, n):
    return np.frombuffer(array, dtype=np.float64).reshape(n, -1)


def scene_text(bundle):
    """A SceneBundle in the checkers' input format (tools/probes/scene_text.h)."""
    out = []
    if bundle.spheres is not None and len(bundle.spheres):
        out.append("spheres %d\n" % len(bundle.spheres) + rows_text(doubles(bundle.spheres, len(bundle.spheres))))
    if bundle.mesh is not None:
        tris, qm, mats, tw, th, nm = bundle.mesh
        n = len(tris)
        t = doubles(tris, n)                               # A B C, mat, uvA uvB uvC
        rows = np.concatenate([t[:, :9], t[:, 19:25], np.asarray(qm[:n], dtype=np.float64)[:, None], t[:, 9:19]],
                              axis=1).tolist()
        out.append("triangles %d %d %d %d\n" % (n, tw, th, nm))
        out.append("\n".join(" ".join(map(repr, r[:15])) + " %d " % r[15] + " ".join(map(repr, r[16:]))
                             for r in rows) + "\n")
        out.append("texels %d\n" % len(mats) + rows_text(doubles(mats, len(mats))))
    if bundle.sky is not None:
        tex, w, h = bundle.sky
        out.append("sky %d %d\n" % (w, h) + rows_text(doubles(tex, w * h)))
    return "".join(out)


def params_text(p=None, **kw):
    """A `params` section from an rt_params (and / or keyword values)."""
    d = {}
    if p is not None:
        d = dict(W=p.largeur_image, H=p.hauteur_image, spp=p.nbRayonParPixel, bounces=p.nbRebondMax,
                 chunks=p.spp_chunks, useAO=p.useAO, AO=p.AO_intensity, compat=p.compat_int_truncation,
                 semantics=p.semantics, accel=p.accel, sky_mode=p.sky_mode, ox=p.cam.origin.e[0],
                 oy=p.cam.origin.e[1], oz=p.cam.origin.e[2], aperture_x=p.ouverture_x, aperture_y=p.ouverture_y)
    d.update(kw)
    return "params " + " ".join("%s %r" % (k, float(v)) for k, v in d.items()) + " end\n"


@functools.lru_cache(maxsize=None)
def variants(checker):
    """The queue kernel's table: [{qb, opq, name, stack}]."""
    p = subprocess.run([checker, "variants"], capture_output=True, text=True, timeout=120, check=True)
    return json.loads(p.stdout)["variants"]


def run(checker, text, env=None):
    e = {k: v for k, v in os.environ.items() if k != "RT_PARTIAL_BUDGET"}
    e.update(env or {})
    p = subprocess.run([checker], input=text, capture_output=True, text=True, timeout=120, env=e)
    assert p.returncode == 0, p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["rc"] == 0, rec
    rows = {(v["qb"], v["opq"]): v for v in variants(checker)}
    for pl in rec["plans"]:                                # every queue plan of every case is its table row
        if pl["queue"]:
            row = rows.get((pl["qb"], pl["opq"]))
            assert row is not None, pl
            assert (pl["name"], pl["stack_cap"]) == (row["name"], row["stack"]), (pl, row)
    return rec["plans"]


def kernels(checker, bundle, params):
    return [pl["name"] for pl in run(checker, scene_text(bundle) + "".join(params_text(p) for p in params))]


def test_queue_variant_table(checker):
    """The seven (QB, OPQ) pairs, their reported names and their stack entries; run() holds every plan to them."""
    table = sorted(variants(checker), key=lambda v: (v["qb"], v["opq"]))
    assert [(v["qb"], v["opq"]) for v in table] == [(-2, 0), (-1, 0), (0, 0), (3, 0), (3, 1), (4, 0), (5, 0)]
    names = [v["name"] for v in table]
    assert names == ["render_kernel_q<QB=%s>" % s for s in ("-2", "-1", "0", "3", "3,OP", "4", "5")]
    assert sorted(names) == sorted([name for name, _, _ in kc.VARIANTS.values()] + [kc.QB5])
    assert [v["stack"] for v in table] == [0, 0, 0, 32, 24, 14, 32]


# ---- scenes -> kernel names, as the GPU tests assert them ------------------------------------------

@pytest.mark.parametrize("sky", [False, True], ids=["nosky", "sky"])
@pytest.mark.parametrize("variant", list(kc.VARIANTS))
def test_queue_variant_scenes(checker, variant, sky):
    name, extra, mesh = kc.VARIANTS[variant]
    bundle = kc.bundle_of(extra, mesh(), sky)
    plans = run(checker, scene_text(bundle) + "".join(params_text(kc.variant_params(sky, ao))
                                                      for ao in (False, True)))
    assert [pl["name"] for pl in plans] == [name, name]
    assert [(pl["sky"], pl["ao"]) for pl in plans] == [(int(sky), 0), (int(sky), 1)]


@pytest.mark.parametrize("alpha", list(kc.ALPHA_KERNEL))
def test_sphere_alpha_thresholds(checker, alpha):
    assert kernels(checker, kc.one_transparent(alpha), [kc.prm()]) == [kc.ALPHA_KERNEL[alpha]]


@pytest.mark.parametrize("mat_index", [3, 4])
def test_override_material_tree(checker, mat_index):
    p = helpers.params(40, 30, 6, 8, use_ao=True, chunks=4)
    assert kernels(checker, kc.override_tree(mat_index), [p]) == [kc.OVERRIDE_KERNEL]


@pytest.mark.parametrize("opaque", [False, True])
def test_tree_with_stack_bound_26(checker, opaque):
    """kernel_cases._nature: above OPQ's 24 entries, within QB 3's 32."""
    p = helpers.params(32, 24, 4, 10, chunks=4, cam=helpers.camera_of(scenes.NATURE_CAMERA))
    pl, = run(checker, scene_text(kc._nature(opaque)) + params_text(p))
    assert (pl["name"], pl["bvh_stack"], pl["stack_cap"]) == ("render_kernel_q<QB=3>", 26, 32)


@pytest.mark.parametrize("name", [c.name for c in cc.PHILOX_CASES if c.kernel is not None])
def test_reference_cases(checker, name):
    bundle, p = cc.PHILOX_BY_NAME[name].scene()
    assert kernels(checker, bundle, [p]) == [cc.PHILOX_BY_NAME[name].kernel]


@pytest.mark.parametrize("name", list(kc.FALLBACK))
def test_trees_without_binary16_nodes(checker, name):
    scene, params, kernel = kc.FALLBACK[name]
    assert kernels(checker, scene(), [params()]) == [kernel]


def test_boundary_between_narrow_and_wide(checker):
    """65 536 triangles of test_bvh_wide.py's height field are the smallest wide tree; one fewer is narrow,
    and above 0x8000 triangles no narrow tree takes the queue kernel (test_gpu_big_mesh.py)."""
    mesh = scenes.heightfield_mesh(182, 1, 0.25, scenes.README_FLOOR)
    ps = [helpers.params(32, 24, 1, 4), helpers.params(32, 24, 4, 4, chunks=4)]
    wide = helpers.SceneBundle(scenes.cornell_spheres(), helpers.mesh_of(mesh, 65536))
    plans = run(checker, scene_text(wide) + "".join(params_text(p) for p in ps))
    assert [pl["name"] for pl in plans] == [kc.BVH32, kc.QB5]
    assert [(pl["wide"], pl["stack_cap"]) for pl in plans] == [(1, 48), (1, 32)]
    assert plans[0]["bvh_stack"] <= 32
    narrow = helpers.SceneBundle(scenes.cornell_spheres(), helpers.mesh_of(mesh, 65535))
    plans = run(checker, scene_text(narrow) + "".join(params_text(p) for p in ps))
    assert [pl["name"] for pl in plans] == ["render_kernel<BVH>"] * 2
    assert [(pl["wide"], pl["stack_cap"], pl["bvh_stack"]) for pl in plans] == [(0, 48, 1 << 30)] * 2


# ---- boundaries, fed as scalars ----------------------------------------------------------------------

# README spheres and an opaque narrow tree that has its 64-byte nodes, inside r_scene; camera at the origin
TREE = dict(ns=10, nt=1320, bvh=1, bvhh=1, bvh_nodes=400, bvh_depth=7, bvh_stack4=20, r_scene=2000.0,
            sph_bound=1004.0, sph_opaque=1, tri_opaque=1)
Q3, Q3OP, Q4, Q5 = ("render_kernel_q<QB=%s>" % s for s in ("3", "3,OP", "4", "5"))
BVH, BVH32, PLAIN, CUDA = "render_kernel<BVH>", "render_kernel<BVH32>", "render_kernel", "render_kernel_cuda"


def plan(checker, facts, env=None, **params):
    text = "facts " + " ".join("%s %r" % (k, float(v)) for k, v in facts.items()) + " end\n"
    pl, = run(checker, text + params_text(**params), env)
    return pl


def tree(**kw):
    return dict(TREE, **kw)


@pytest.mark.parametrize("facts,name,cap", [
    (tree(bvh_depth=4, bvh_stack4=14), Q4, 14),            # shallow: QB 4 up to 14 ...
    (tree(bvh_depth=4, bvh_stack4=15), Q3OP, 24),          # ... then the deep-tree walk
    (tree(bvh_depth=5, bvh_stack4=14), Q3OP, 24),          # deep with 64-byte nodes: never QB 4
    (tree(bvh_stack4=24), Q3OP, 24),
    (tree(bvh_stack4=25), Q3, 32),
    (tree(bvh_stack4=24, tri_opaque=0), Q3, 32),
    (tree(bvh_stack4=24, sph_opaque=0), Q3, 32),
    (tree(bvh_stack4=32), Q3, 32),
    (tree(bvh_stack4=33), BVH, 48),
    (tree(bvh_stack4=48), BVH, 48),
    # an origin beyond r_scene: QB 4 and OPQ have no far-origin margins
    (tree(bvh_depth=4, bvh_stack4=14, sph_bound=1e5), Q3, 32),
    (tree(bvh_stack4=20, sph_bound=1e5), Q3, 32),
    # no 64-byte nodes: QB 4's walk when the bound fits it, else the fixed grid
    (tree(bvhh=0, bvh_stack4=14), Q4, 14),
    (tree(bvhh=0, bvh_stack4=15), BVH, 48),
    (tree(bvhh=0, bvh_stack4=14, sph_bound=1e5), BVH, 48),
    # wide trees
    (tree(bvh_wide=1, bvhh=0, bvhw=1, nt=70000, bvh_nodes=35000, bvh_stack4=32), Q5, 32),
    (tree(bvh_wide=1, bvhh=0, bvhw=1, nt=70000, bvh_nodes=35000, bvh_stack4=33), BVH32, 48),
    (tree(bvh_wide=1, bvhh=0, bvhw=0, nt=70000, bvh_nodes=35000, bvh_stack4=20), BVH32, 48),
    (tree(bvh_wide=1, bvhh=0, bvhw=1, nt=70000, bvh_nodes=35000, bvh_stack4=14, bvh_depth=4), Q5, 32),
    # a narrow tree whose indices do not fit the uint16 stack entries
    (tree(bvh_nodes=0x7fff, nt=0x8000), Q3OP, 24),
    (tree(bvh_nodes=0x8000, nt=0x8000), BVH, 48),
    (tree(bvh_nodes=0x7fff, nt=0x8001), BVH, 48),
    # no BVH
    (dict(ns=10, nt=0, sph_opaque=1), "render_kernel_q<QB=-2>", 0),
    (dict(ns=10, nt=0, sph_opaque=0), "render_kernel_q<QB=-1>", 0),
    (dict(ns=10, nt=5, sph_opaque=1, tri_opaque=1), "render_kernel_q<QB=0>", 0),
])
def test_stack_bounds(checker, facts, name, cap):
    pl = plan(checker, facts, chunks=4)
    assert (pl["name"], pl["stack_cap"], pl["queue"]) == (name, cap, int("_q<" in name))
    if facts.get("bvh") and not facts.get("bvh_wide"):
        sentinel = facts["bvh_nodes"] >= 0x8000 or facts["nt"] > 0x8000
        assert pl["bvh_stack"] == (1 << 30 if sentinel else facts["bvh_stack4"])
    # a count run checks pushes against the same stack, in one band without partials
    cnt = plan(checker, facts, chunks=4, count=1)
    assert (cnt["stack_cap"], cnt["name"], cnt["band_rows"], cnt["partial_bytes"]) == (cap, name, 30, 0)


@pytest.mark.parametrize("facts,kw,name,fixed", [
    (TREE, dict(chunks=1), BVH, dict(bvh=1, wide=0, cuda=0)),
    (dict(ns=10, sph_opaque=1), dict(chunks=1), PLAIN, dict(bvh=0, wide=0, cuda=0)),
    (TREE, dict(chunks=4, semantics=RT_SEM_CUDA), CUDA, dict(bvh=1, wide=0, cuda=1)),
    (dict(ns=10, sph_opaque=1), dict(chunks=4, semantics=RT_SEM_CUDA), CUDA, dict(bvh=0, wide=0, cuda=1)),
    (tree(bvh_wide=1, bvhw=1), dict(chunks=4, semantics=RT_SEM_CUDA), CUDA, dict(bvh=1, wide=1, cuda=1)),
    (TREE, dict(chunks=4, accumulate=1), BVH, dict(bvh=1, wide=0, cuda=0)),
    (dict(ns=10, sph_opaque=1), dict(chunks=4, accumulate=1), PLAIN, dict(bvh=0, wide=0, cuda=0)),
    (TREE, dict(chunks=4, accel=1), "render_kernel_q<QB=0>", dict(bvh=0, wide=0, cuda=0)),     # RT_ACCEL_NONE
])
def test_launches_without_the_queue(checker, facts, kw, name, fixed):
    pl = plan(checker, facts, **kw)
    assert pl["name"] == name and pl["queue"] == int("_q<" in name)
    assert {k: pl[k] for k in fixed} == fixed
    assert pl["stack_cap"] == (48 if fixed["bvh"] else 0)
    chunks = kw["chunks"]
    assert (pl["task_ok"], pl["band_rows"], pl["partial_bytes"]) == \
        (int(chunks > 1), 30, chunks * 40 * 30 * 72 if chunks > 1 else 0)


@pytest.mark.parametrize("cam", [dict(oz=float("nan")), dict(ox=float("inf")), dict(oy=float("-inf"))])
def test_non_finite_camera_gets_no_bvh(checker, cam):
    pl = plan(checker, TREE, chunks=4, **cam)
    assert (pl["bvh"], pl["name"], pl["stack_cap"], pl["bvh_stack"]) == (0, "render_kernel_q<QB=0>", 0, 0)
    assert plan(checker, TREE, chunks=4, oz=3.0)["name"] == Q3OP


def test_tasks_of_a_band_fit_32_bits(checker):
    """The queue numbers a band's chunks * pixels below 2^31.  2^31 - 1 is prime, so with chunks > 1 the
    largest count below the limit is 2^31 - 2 = 2 * 32767 * 32769."""
    env = {"RT_PARTIAL_BUDGET": str(1 << 42)}              # (one band: the budget does not cut it)
    sph = dict(ns=10, sph_opaque=1)
    below = plan(checker, sph, env, chunks=2, spp=4, W=32769, H=32767)
    assert below["band_rows"] * 32769 * below["chunks"] == (1 << 31) - 2
    assert (below["task_ok"], below["queue"], below["name"]) == (1, 1, "render_kernel_q<QB=-2>")
    at = plan(checker, sph, env, chunks=2, spp=4, W=65536, H=16384)
    assert at["band_rows"] * 65536 * at["chunks"] == 1 << 31
    assert (at["task_ok"], at["queue"], at["name"]) == (0, 0, PLAIN)
    assert at["partial_bytes"] == (1 << 31) * 72


@pytest.mark.parametrize("budget,rows,band", [
    (None, 100, 100),                 # 4 GiB: one band
    (1, 100, 16),                     # at least 16 rows
    (11520 * 31, 100, 16),
    (11520 * 32, 100, 32),            # multiples of 16
    (11520 * 47, 100, 32),
    (11520 * 48, 100, 48),
    (11520 * 1000, 100, 100),         # at most local_rows
    (1, 10, 10),
    (-5, 100, 100), (0, 100, 100),    # not a budget: the default
])
def test_partial_budget_bands(checker, budget, rows, band):
    env = None if budget is None else {"RT_PARTIAL_BUDGET": str(budget)}
    pl = plan(checker, dict(ns=10, sph_opaque=1), env, chunks=4, W=40, H=100, rows=rows)
    assert pl["chunks"] == 4 and (pl["band_rows"], pl["partial_bytes"]) == (band, 11520 * band)    # 4 * 40 * 72
    assert (pl["task_ok"], pl["name"]) == (1, "render_kernel_q<QB=-2>")
    cnt = plan(checker, dict(ns=10, sph_opaque=1), env, chunks=4, W=40, H=100, rows=rows, count=1)
    assert (cnt["band_rows"], cnt["partial_bytes"], cnt["task_ok"]) == (rows, 0, 1)
