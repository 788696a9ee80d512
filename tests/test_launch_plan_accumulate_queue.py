"""Host check of the launch plan with rt_set_accumulate_queue's switch
(KParams::acc_queue; the checker's key accumulate_queue), CPU only.

With the switch on, a launch with running sums (accumulate=1) gets the plan a
render launch of the same scene and params gets -- name, (QB, OPQ), stack, row
bands and partial bytes -- wherever that is one of the seven queue pairs; one
sample slice, RT_SEM_CUDA and a tree above every queue stack keep the fixed
grid.  Without the key every plan is what it was.  The cases are
test_launch_plan.py's: its scenes for the pairs, its scalar boundaries."""
import subprocess

import pytest

import kernel_cases as kc
import test_launch_plan as tlp
from tipe_rt.types import RT_SEM_CUDA

SAME = ("name", "queue", "qb", "opq", "sky", "ao", "stack_cap", "task_ok", "band_rows", "partial_bytes", "chunks")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_accq") / "launch_plan_check")
    subprocess.run(["g++", "-O2"] + tlp.FLAGS + ["-o", exe] + tlp.SRC, check=True)
    return exe


def three_plans(checker, head, env=None, **params):
    """(render, accumulate with the switch, accumulate without) of one scene text and params."""
    text = head + tlp.params_text(**params) + tlp.params_text(accumulate=1, accumulate_queue=1, **params) + \
        tlp.params_text(accumulate=1, **params)
    return tlp.run(checker, text, env)


def facts_text(facts):
    return "facts " + " ".join("%s %r" % (k, float(v)) for k, v in facts.items()) + " end\n"


@pytest.mark.parametrize("ao", [False, True], ids=["noao", "ao"])
@pytest.mark.parametrize("sky", [False, True], ids=["nosky", "sky"])
@pytest.mark.parametrize("variant", list(kc.VARIANTS))
def test_the_pairs_of_the_variant_scenes(checker, variant, sky, ao):
    name, extra, mesh = kc.VARIANTS[variant]
    p = kc.variant_params(sky, ao)
    head = tlp.scene_text(kc.bundle_of(extra, mesh(), sky))
    render, on, off = tlp.run(checker, head + tlp.params_text(p) + tlp.params_text(p, accumulate=1, accumulate_queue=1)
                              + tlp.params_text(p, accumulate=1))
    assert (render["name"], render["queue"]) == (name, 1)
    assert {k: on[k] for k in SAME} == {k: render[k] for k in SAME}
    assert off["queue"] == 0 and off["name"] in ("render_kernel", "render_kernel<BVH>")


WIDE = tlp.tree(bvh_wide=1, bvhh=0, bvhw=1, nt=70000, bvh_nodes=35000, bvh_stack4=32)
# facts that reach each of the seven pairs as a render launch (test_launch_plan.test_stack_bounds' rows)
PAIRS = [
    (tlp.tree(bvh_depth=4, bvh_stack4=14), tlp.Q4),
    (tlp.tree(bvh_stack4=24), tlp.Q3OP),
    (tlp.tree(bvh_stack4=25), tlp.Q3),
    (tlp.tree(bvh_stack4=20, sph_bound=1e5), tlp.Q3),
    (WIDE, tlp.Q5),
    (dict(ns=10, nt=0, sph_opaque=1), "render_kernel_q<QB=-2>"),
    (dict(ns=10, nt=0, sph_opaque=0), "render_kernel_q<QB=-1>"),
    (dict(ns=10, nt=5, sph_opaque=1, tri_opaque=1), "render_kernel_q<QB=0>"),
]


@pytest.mark.parametrize("facts,name", PAIRS)
def test_the_seven_pairs_by_their_facts(checker, facts, name):
    render, on, off = three_plans(checker, facts_text(facts), chunks=4)
    assert (render["name"], render["queue"]) == (name, 1)
    assert {k: on[k] for k in SAME} == {k: render[k] for k in SAME}
    assert (off["queue"], off["task_ok"], off["band_rows"], off["partial_bytes"]) == \
        (0, 1, render["band_rows"], render["partial_bytes"])


def test_all_seven_pairs_are_covered(checker):
    assert {name for _, name in PAIRS} == {v["name"] for v in tlp.variants(checker)}


@pytest.mark.parametrize("budget,band", [(11520 * 32, 32), (1, 16), (None, 100)])
def test_row_bands_are_the_render_launch_s(checker, budget, band):
    env = None if budget is None else {"RT_PARTIAL_BUDGET": str(budget)}
    render, on, off = three_plans(checker, facts_text(dict(ns=10, sph_opaque=1)), env, chunks=4, W=40, H=100)
    assert (render["band_rows"], render["partial_bytes"]) == (band, 11520 * band)
    assert {k: on[k] for k in SAME} == {k: render[k] for k in SAME}
    assert (off["name"], off["band_rows"], off["partial_bytes"]) == ("render_kernel", band, 11520 * band)


@pytest.mark.parametrize("facts,kw,name", [
    (tlp.TREE, dict(chunks=1), tlp.BVH),                                  # one slice carries the sums in order
    (dict(ns=10, sph_opaque=1), dict(chunks=1), tlp.PLAIN),
    (tlp.TREE, dict(chunks=4, semantics=RT_SEM_CUDA), tlp.CUDA),
    (dict(ns=10, sph_opaque=1), dict(chunks=4, semantics=RT_SEM_CUDA), tlp.CUDA),
    (tlp.tree(bvh_stack4=33), dict(chunks=4), tlp.BVH),                   # above every queue stack
    (tlp.tree(bvhh=0, bvh_stack4=15), dict(chunks=4), tlp.BVH),           # no walk admits it
    (tlp.tree(bvh_wide=1, bvhh=0, bvhw=1, nt=70000, bvh_nodes=35000, bvh_stack4=33), dict(chunks=4), tlp.BVH32),
    (tlp.tree(bvh_nodes=0x8000, nt=0x8000), dict(chunks=4), tlp.BVH),
])
def test_launches_that_keep_the_fixed_grid(checker, facts, kw, name):
    render, on, off = three_plans(checker, facts_text(facts), **kw)
    for pl in (render, on, off):
        assert (pl["name"], pl["queue"], pl["qb"]) == (name, 0, 0)
    assert on == off


def test_a_band_of_2_31_tasks_keeps_the_fixed_grid(checker):
    env = {"RT_PARTIAL_BUDGET": str(1 << 42)}
    sph = facts_text(dict(ns=10, sph_opaque=1))
    render, on, off = three_plans(checker, sph, env, chunks=2, spp=4, W=65536, H=16384)
    assert [(pl["task_ok"], pl["queue"], pl["name"]) for pl in (render, on, off)] == [(0, 0, tlp.PLAIN)] * 3
    render, on, off = three_plans(checker, sph, env, chunks=2, spp=4, W=32769, H=32767)
    assert [(pl["task_ok"], pl["queue"]) for pl in (render, on, off)] == [(1, 1), (1, 1), (1, 0)]


@pytest.mark.parametrize("facts", [tlp.TREE, dict(ns=10, sph_opaque=1), WIDE])
def test_without_the_key_the_plan_is_unchanged(checker, facts):
    """The switch is read for a launch with running sums only; off (or absent), such a launch is the fixed grid's."""
    head = facts_text(facts)
    plain, keyed_off, render, render_keyed = tlp.run(
        checker, head + tlp.params_text(chunks=4, accumulate=1) + tlp.params_text(chunks=4, accumulate=1, accumulate_queue=0)
        + tlp.params_text(chunks=4) + tlp.params_text(chunks=4, accumulate_queue=1))
    assert plain == keyed_off and plain["queue"] == 0
    assert plain["name"] in (tlp.BVH, tlp.PLAIN, tlp.BVH32)
    assert render == render_keyed and render["queue"] == 1
    cnt, cnt_keyed = tlp.run(checker, head + tlp.params_text(chunks=4, count=1)
                             + tlp.params_text(chunks=4, count=1, accumulate_queue=1))
    assert cnt == cnt_keyed
