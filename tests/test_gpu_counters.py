"""rt_count_async's event totals against the oracle's counters: every
COUNT = true kernel instantiation with the zero-throughput exit on (the mode
every published count uses; reference: rt_oracle.h oracle_set_zero_exit) and
off (the reference's own tracer), the launch shapes the benchmarks count with
(chunks, cyclic row tiles, row bands, repeated calls), the exit's gates, and
what rt.h's definitions imply for the GPU-only diagnostics.  Counters are
integers: every comparison is exact.  Frames: the exit changes no plane."""
import numpy as np
import pytest

import helpers
import kernel_cases
import tipe_rt
from gpu_driver import Uploaded, assert_same_frame, check_parity, gpu_counts, gpu_render
from tipe_rt import scenes
from tipe_rt.types import (RT_CNT_SAMPLES, RT_CNT_CASTS, RT_CNT_SPHERE_TESTS, RT_CNT_SPHERE_DISC, RT_CNT_TRI_TESTS,
                           RT_CNT_SHADE, RT_CNT_TEX_HITS, RT_CNT_REFRACT, RT_CNT_RNG_DRAWS, RT_CNT_EXACT_RESCANS,
                           RT_CNT_BVH_NODES, RT_CNT_BVH_TRI_TESTS, RT_CNT_BVH_LANE_SLOTS, RT_CNT_LEAF_LANE_SLOTS,
                           RT_CNT_CAST_LANE_SLOTS, RT_CNT_SHADE_LANE_SLOTS, RT_CNT_BVH_STACK_OVER, RT_NCOUNTERS,
                           RT_SEM_CUDA, RT_SPP_CHUNKS_AUTO)

pytestmark = pytest.mark.gpu

NINE = RT_CNT_EXACT_RESCANS          # the reference counters: RT_CNT_SAMPLES .. RT_CNT_RNG_DRAWS
assert NINE == 9
BVH_COUNTERS = (RT_CNT_BVH_NODES, RT_CNT_BVH_TRI_TESTS, RT_CNT_BVH_LANE_SLOTS, RT_CNT_LEAF_LANE_SLOTS,
                RT_CNT_BVH_STACK_OVER)
LANE_SLOTS = (RT_CNT_BVH_LANE_SLOTS, RT_CNT_LEAF_LANE_SLOTS, RT_CNT_CAST_LANE_SLOTS, RT_CNT_SHADE_LANE_SLOTS)


def named(c):
    return dict(zip(tipe_rt.COUNTER_NAMES, (int(x) for x in c)))


def assert_nine(got, ref, what):
    """The nine reference counters, exactly."""
    g, r = [int(x) for x in got[:NINE]], [int(x) for x in ref[:NINE]]
    assert g == r, "%s: gpu %r\noracle %r" % (what, named(g), named(r))


def oracle_counts(bundle, p, zero_exit, nthreads=1, rows=None):
    """The oracle's counters of the frame, or summed over the given rows."""
    if rows is None:
        return helpers.oracle_render(bundle, p, nthreads=nthreads, counters=True, zero_exit=zero_exit)["counters"]
    tot = np.zeros(RT_NCOUNTERS, dtype=np.uint64)
    for j in rows:
        tot += helpers.oracle_render(bundle, p, row_hi=j, row_lo=j, counters=True, zero_exit=zero_exit)["counters"]
    return tot


# ---- a. every COUNT instantiation, exit on and off ------------------------------
# 21x13: neither a multiple of the 8x8 wave tile nor of the 16x16 block, two
# blocks wide: partial waves and blocks take part in the kernel's reduction.
def _p(W=21, H=13, spp=4, bounces=6, **kw):
    kw.setdefault("compat", 0)
    return lambda: helpers.params(W, H, spp, bounces, **kw)


def wide_box():
    return helpers.SceneBundle(scenes.cornell_spheres(), kernel_cases.alpha_mesh())


def wide_sky():
    sk = helpers.sky_scene()
    return helpers.SceneBundle(sk.spheres, kernel_cases.alpha_mesh(), sky=sk.sky)


def synthetic():
    return helpers.SceneBundle(*scenes.synthetic_cornell(10, 100))


class Row:
    def __init__(self, build, params, kernel, nonzero, nthreads=1, bites=True):
        self.build, self.params, self.kernel, self.nonzero, self.nthreads = build, params, kernel, nonzero, nthreads
        self.bites = bites           # the exit removes casts on this frame (2 bounces without AO: it cannot)


FLAT, BVH, WIDE = "render_kernel", "render_kernel<BVH>", kernel_cases.BVH32
# nonzero: the events the row is there for (a row cannot pass on zeros)
ROWS = {
    "flat-cornell": Row(helpers.cornell, _p(), FLAT, (RT_CNT_CASTS, RT_CNT_SPHERE_DISC, RT_CNT_SHADE)),
    "flat-pyramid-ao": Row(helpers.pyramid_scene, _p(use_ao=True), FLAT,
                           (RT_CNT_TRI_TESTS, RT_CNT_TEX_HITS, RT_CNT_REFRACT)),
    "flat-alpha-half": Row(lambda: kernel_cases.one_transparent(0.5), _p(), FLAT, (RT_CNT_REFRACT,)),
    "flat-alpha-zero": Row(lambda: kernel_cases.one_transparent(0.0), _p(), FLAT, (RT_CNT_SHADE,)),
    "flat-sky": Row(helpers.sky_scene, _p(sky_mode=1), FLAT, (RT_CNT_CASTS, RT_CNT_SHADE)),
    "bvh-tree-ao": Row(helpers.tree_scene, _p(use_ao=True), BVH, (RT_CNT_TEX_HITS, RT_CNT_BVH_NODES)),
    "bvh-mineways": Row(helpers.mineways_scene, _p(), BVH, (RT_CNT_TEX_HITS, RT_CNT_BVH_TRI_TESTS)),
    "bvh-synthetic": Row(synthetic, _p(spp=3, bounces=5), BVH, (RT_CNT_TRI_TESTS, RT_CNT_BVH_NODES)),
    "bvh-sky-tree-ao": Row(helpers.sky_tree_scene, _p(sky_mode=1, use_ao=True), BVH,
                           (RT_CNT_TEX_HITS, RT_CNT_BVH_NODES)),
    "wide": Row(wide_box, _p(16, 12, 2, 2), WIDE, (RT_CNT_TEX_HITS, RT_CNT_REFRACT, RT_CNT_BVH_TRI_TESTS),
                nthreads=8, bites=False),
    "wide-sky": Row(wide_sky, _p(16, 12, 2, 2, sky_mode=1), WIDE, (RT_CNT_TEX_HITS, RT_CNT_BVH_TRI_TESTS),
                    nthreads=8, bites=False),
    # with AO the second bounce's AO cast is skipped once rayColor is black
    "wide-ao": Row(wide_box, _p(16, 12, 2, 2, use_ao=True), WIDE, (RT_CNT_TEX_HITS, RT_CNT_BVH_TRI_TESTS),
                   nthreads=8),
}


@pytest.fixture(scope="module")
def uploaded():
    """name -> the row's scene on the device, uploaded once for the module."""
    ups = {}

    def get(name):
        if name not in ups:
            ups[name] = Uploaded(ROWS[name].build())
        return ups[name]
    yield get
    for up in ups.values():
        up.close()


@pytest.mark.parametrize("name", list(ROWS))
def test_count_kernels_match_oracle_exit_on_and_off(uploaded, name):
    """GPU counts with the exit on (the default) against the oracle that
    leaves at rayColor == 0, and under reference_counts() against the oracle
    that never does.  The kernel name is that of a render of the same params,
    which plan_render lays out like the count run (spp_chunks 1: fixed grid)."""
    row, up = ROWS[name], uploaded(name)
    p = row.params()
    up.render(p)
    assert up.kernel == row.kernel
    got_on = up.counts(p)
    with tipe_rt.reference_counts():
        got_off = up.counts(p)
    ref_on = oracle_counts(up.bundle, p, True, row.nthreads)
    ref_off = oracle_counts(up.bundle, p, False, row.nthreads)
    print(name, "exit on", named(got_on), "\n  exit off", named(got_off))
    assert_nine(got_on, ref_on, name + ", exit on")
    assert_nine(got_off, ref_off, name + ", exit off")
    for k in row.nonzero:
        assert got_on[k] > 0 and got_off[k] > 0, (tipe_rt.COUNTER_NAMES[k], got_on[k], got_off[k])
    assert (ref_on[RT_CNT_CASTS] < ref_off[RT_CNT_CASTS]) == row.bites


# ---- e. GPU-only diagnostics: what rt.h's definitions imply ----------------------
@pytest.mark.parametrize("exit_on", [True, False], ids=["exit-on", "exit-off"])
@pytest.mark.parametrize("name", list(ROWS))
def test_diagnostic_counters_keep_their_definitions(uploaded, name, exit_on):
    row, up = ROWS[name], uploaded(name)
    p = row.params()
    if exit_on:
        c = up.counts(p)
    else:
        with tipe_rt.reference_counts():
            c = up.counts(p)
    what = (name, named(c))
    for k in LANE_SLOTS:                                  # 64 x wave-level executions
        assert c[k] % 64 == 0, what
    assert c[RT_CNT_CASTS] <= c[RT_CNT_CAST_LANE_SLOTS], what
    assert c[RT_CNT_SHADE_LANE_SLOTS] > 0, what
    assert c[RT_CNT_EXACT_RESCANS] <= c[RT_CNT_CASTS], what
    assert c[RT_CNT_BVH_STACK_OVER] == 0, what
    if row.kernel == FLAT:
        for k in BVH_COUNTERS:
            assert c[k] == 0, what
    else:
        assert 0 < c[RT_CNT_BVH_NODES] <= c[RT_CNT_BVH_LANE_SLOTS], what
        assert 0 < c[RT_CNT_BVH_TRI_TESTS] <= c[RT_CNT_TRI_TESTS], what
        assert c[RT_CNT_LEAF_LANE_SLOTS] > 0, what


# ---- b. the launch shapes the benchmarks count with ------------------------------
W, H = 21, 13


def shapes_params(spp=3, bounces=6, chunks=1):
    return helpers.params(W, H, spp, bounces, use_ao=True, compat=0, chunks=chunks)


@pytest.fixture(scope="module")
def pyramid(uploaded):
    return uploaded("flat-pyramid-ao")


@pytest.fixture(scope="module")
def pyramid_rows(pyramid):
    """The oracle's counters (exit on) of each row of the 21x13 x 3 spp frame."""
    p = shapes_params()
    return [oracle_counts(pyramid.bundle, p, True, rows=[j]) for j in range(H)]


def rows_sum(per_row, rows):
    return sum((per_row[j] for j in rows), np.zeros(RT_NCOUNTERS, dtype=np.uint64))


@pytest.mark.parametrize("chunks", [4, RT_SPP_CHUNKS_AUTO], ids=["chunks4", "auto"])
def test_chunked_count_equals_one_chunk(pyramid, pyramid_rows, chunks):
    """spp 3 under spp_chunks 4 or AUTO: three one-sample slices per pixel
    (the grid's z), counted like the single chunk."""
    assert tipe_rt.types.rt_resolve_spp_chunks(chunks, 3) == 3
    one = pyramid.counts(shapes_params())
    got = pyramid.counts(shapes_params(chunks=chunks))
    assert_nine(got, one, "chunked vs one chunk")
    assert_nine(got, rows_sum(pyramid_rows, range(H)), "chunked vs oracle")
    assert got[RT_CNT_SAMPLES] == W * H * 3


def test_zero_bounces(pyramid):
    """nbRebondMax 0: tracer's loop does not run; only the camera draws happen."""
    p = shapes_params(bounces=0)
    got = pyramid.counts(p)
    assert_nine(got, oracle_counts(pyramid.bundle, p, True), "0 bounces")
    assert got[RT_CNT_SAMPLES] == W * H * 3 and got[RT_CNT_RNG_DRAWS] == 4 * W * H * 3
    assert got[RT_CNT_CASTS] == 0


def cdiv(a, b):
    return -(-a // b)


def tile_rows_of(t):
    """Global rows of an rt_tiling below H (rt.h: rows at or beyond H are padding)."""
    rows = [t.row_base + (t.tile_first + lt * t.tile_step) * t.tile_rows + y
            for lt in range(t.n_tiles) for y in range(t.tile_rows)]
    return [g for g in rows if g < H]


@pytest.mark.parametrize("k,G", [(1, 3), (2, 4)])
def test_cyclic_tiles(pyramid, pyramid_rows, k, G):
    """Rank r of G with cyclic k-row tiles {0, k, r, G, ceil(ceil(H/k)/G)}
    (bench.py's launch): every rank counts its own rows -- the last tile of
    some ranks reaches past row H -- and the ranks add up to the frame."""
    p = shapes_params()
    total = np.zeros(RT_NCOUNTERS, dtype=np.uint64)
    padded = 0
    seen = []
    for r in range(G):
        t = tipe_rt.cyclic_tiling(H, k, r, G)
        assert (t.row_base, t.tile_rows, t.tile_first, t.tile_step, t.n_tiles) == (0, k, r, G, cdiv(cdiv(H, k), G))
        rows = tile_rows_of(t)
        padded += t.n_tiles * t.tile_rows - len(rows)
        seen += rows
        got = pyramid.counts(p, tiling=t)
        assert_nine(got, rows_sum(pyramid_rows, rows), "rank %d of %d, %d-row tiles" % (r, G, k))
        total += np.array(got, dtype=np.uint64)
    assert sorted(seen) == list(range(H)) and padded > 0
    assert_nine(total, pyramid.counts(p), "ranks' sum vs whole frame")


def test_row_band(pyramid, pyramid_rows):
    lo, hi = 4, 9
    got = pyramid.counts(shapes_params(), tiling=tipe_rt.types.Tiling(lo, hi - lo + 1, 0, 1, 1))
    assert_nine(got, rows_sum(pyramid_rows, range(lo, hi + 1)), "rows %d..%d" % (lo, hi))
    assert got[RT_CNT_SAMPLES] == W * (hi - lo + 1) * 3


def test_count_adds_into_the_array(pyramid):
    """rt.h: rt_count_async ADDS its totals: a second call doubles every
    counter, and a pre-filled array keeps its offset."""
    import torch
    p = shapes_params()
    once = pyramid.counts(p)
    d = torch.zeros(RT_NCOUNTERS, dtype=torch.int64, device="cuda:0")
    assert pyramid.counts(p, into=d) == once
    assert pyramid.counts(p, into=d) == [2 * x for x in once]
    fill = [1000 + 7 * k for k in range(RT_NCOUNTERS)]
    d = torch.tensor(fill, dtype=torch.int64, device="cuda:0")
    assert pyramid.counts(p, into=d) == [f + x for f, x in zip(fill, once)]


def test_counters_match_oracle():
    bundle = helpers.pyramid_scene()
    p = helpers.params(32, 24, 8, 6, use_ao=True)
    ref = helpers.oracle_render(bundle, p, counters=True)["counters"]
    with tipe_rt.reference_counts():
        got = np.array(gpu_counts(bundle, p), dtype=np.uint64)
    k = tipe_rt.types.RT_CNT_EXACT_RESCANS           # GPU-only diagnostic
    assert list(got[:k]) == list(ref[:k]), dict(zip(tipe_rt.COUNTER_NAMES, zip(got, ref)))
    assert got[k] <= got[tipe_rt.types.RT_CNT_CASTS] // 1000   # candidate pass almost never ambiguous


@pytest.mark.parametrize("scene,ao", [("cornell", False), ("cornell", True), ("pyramid", True), ("tree", True)])
def test_zero_throughput_exit(scene, ao):
    """Paths end once rayColor == 0 (rt_set_zero_throughput_exit): frames are
    bit-identical with the exit on and off and to the oracle (which never
    exits), and the exit only removes casts."""
    bundle = {"cornell": helpers.cornell, "pyramid": helpers.pyramid_scene, "tree": helpers.tree_scene}[scene]()
    p = helpers.params(32, 24, 8, 6, use_ao=ao, ao=2.5, compat=0)
    check_parity(bundle, p)
    on = gpu_render(bundle, p)
    with tipe_rt.reference_counts():
        off = gpu_render(bundle, p)
        ref_cnt = gpu_counts(bundle, p)
    assert_same_frame(on, off, "exit on vs off:")
    cnt = gpu_counts(bundle, p)
    T = tipe_rt.types
    assert cnt[T.RT_CNT_SAMPLES] == ref_cnt[T.RT_CNT_SAMPLES]
    assert cnt[T.RT_CNT_CASTS] < ref_cnt[T.RT_CNT_CASTS]
    print(scene, "ao" if ao else "", "casts per sample", ref_cnt[T.RT_CNT_CASTS] / ref_cnt[0], "->",
          cnt[T.RT_CNT_CASTS] / cnt[0])


# ---- c. the exit's gates (rt_launch_plan.cpp set_gates) --------------------------
def assert_gated_off(bundle, p):
    """The exit is requested (the default) and the host must refuse it: the
    counts are the reference's, where the oracle's exit would count less."""
    ref = oracle_counts(bundle, p, False)
    assert oracle_counts(bundle, p, True)[RT_CNT_CASTS] < ref[RT_CNT_CASTS]     # the gate decides something here
    assert_nine(gpu_counts(bundle, p), ref, "gated off")


def test_zero_throughput_exit_gated_off():
    """A material beyond the exit's bound (emission strength 1e200 > 2^100:
    the host cannot rule out em overflowing to inf, and inf * 0 is NaN) or
    AO_intensity outside (0, 1000] turns the exit off: the counts are then
    the reference's."""
    spheres = tipe_rt.scenes.cornell_spheres()
    spheres[3].mat.emissionStrength = 1e200
    bundle = helpers.SceneBundle(spheres)
    p = helpers.params(16, 12, 4, 6)
    check_parity(bundle, p)
    assert_gated_off(bundle, p)
    bundle = helpers.cornell()
    p = helpers.params(16, 12, 4, 6, use_ao=True, ao=2000.0, compat=0)
    check_parity(bundle, p)
    assert_gated_off(bundle, p)


def test_zero_throughput_exit_gated_off_by_a_far_coordinate():
    """With AO a coordinate beyond 2^20 turns the exit off (the AO factor's
    bound needs distance/dst <= 1.02): with a small sphere behind the camera
    at z = 3e6 every count must be the reference's; without AO the same scene
    keeps the exit."""
    far = [((0.0, 0.0, 3.0e6), 1.0, scenes.material((0.5, 0.5, 0.5)))]
    bundle = helpers.cornell(extra=far)
    assert_gated_off(bundle, helpers.params(16, 12, 4, 6, use_ao=True, compat=0))
    p = helpers.params(16, 12, 4, 6)
    assert_nine(gpu_counts(bundle, p), oracle_counts(bundle, p, True), "no AO: the exit stays on")


def test_zero_throughput_exit_gated_off_by_cuda_semantics():
    """RT_SEM_CUDA never takes the exit (main_cuda.cu's tracer has its own
    loop): the counts are those of the oracle's tracer_cuda, which has none.
    The main.c oracle of the same scene shows the exit would have counted less."""
    bundle = helpers.cornell()
    p = helpers.params(16, 12, 4, 6, use_ao=True, compat=0, semantics=RT_SEM_CUDA)
    main_c = helpers.params(16, 12, 4, 6, use_ao=True, compat=0)
    assert oracle_counts(bundle, main_c, True)[RT_CNT_CASTS] < oracle_counts(bundle, main_c, False)[RT_CNT_CASTS]
    got = gpu_counts(bundle, p)
    assert_nine(got, oracle_counts(bundle, p, False), "RT_SEM_CUDA, exit requested")
    with tipe_rt.reference_counts():
        assert gpu_counts(bundle, p)[:NINE] == got[:NINE]
