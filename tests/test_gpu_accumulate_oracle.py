"""rt_accumulate_async, rt_accumulate_list_async and rt_adaptive_async against
the CPU oracle's oracle_accumulate (rt.h "progressive rendering" restated in
plain C; tests/test_oracle_accumulate.py ties it to the pinned
oracle_render_rows).

The rule for "equal" is accumulate_support.assert_same_sums: the uint64 bits of
all nine sums of every local pixel, zero signs included, a NaN on both sides
excepted.  No tolerance: both sides perform the same IEEE operations from the
same starting bits.

Every case is a sequence of batches into one accumulator with a different
spp_chunks per batch, starting from adaptive_support.sentinel (finite, non-zero,
different in every pixel and slot), so the first batch already folds onto
running sums, an unwritten pixel shows, and a write to a wrong local index
shows; and once more from that sentinel scaled by 2^-20, where the order of
the additions shows (accumulate_support.check_accumulate says why).  Every case
also asserts that each rendered pixel's sums left their start and that each
launch took the expected fixed-grid kernel."""
import numpy as np
import pytest

import helpers
import tipe_rt
from accumulate_support import (HIGH_OFFSETS, KERNEL, LIST_OFFSETS, SCENES, WORD_BATCH, WORD_FRAMES, Uploads,
                                assert_same_sums, check_accumulate, consecutive, cyclic, global_rows, oracle_batches,
                                tiling_of, whole)
from adaptive_support import (accumulate_list, device_adaptive, glass_cornell, pick, reference_rounds, schedule,
                              sentinel, u64)
from tipe_rt.types import RT_SPP_CHUNKS_AUTO

pytestmark = pytest.mark.gpu

AUTO = RT_SPP_CHUNKS_AUTO
uploaded = Uploads(dict(SCENES, glass=(glass_cornell, {})))


@pytest.fixture(scope="module", autouse=True)
def release_scenes():
    """The uploads live for the module and are released with it."""
    yield
    uploaded.release()


# ---- every fixed-grid instantiation ---------------------------------------------

@pytest.mark.parametrize("scene", sorted(SCENES))
def test_kernel_instantiations(scene):
    """render_kernel<BVH,SKY> and render_kernel_w<SKY>: a strict batch, then a
    sliced one (the wide tree at test_gpu_big_mesh's scale: 2 samples, where
    spp_chunks 3 resolves to 2 slices)."""
    bundle, ds = uploaded(scene)
    wide = scene.startswith("wide")
    W, H, S, B = (16, 12, 2, 2) if wide else (37, 23, 4, 5)
    p = helpers.params(W, H, S, B, **SCENES[scene][1])
    check_accumulate(bundle, ds, p, consecutive([(S, 1), (S, 3)]), whole(H), KERNEL[scene], scene)


@pytest.mark.parametrize("scene", ["cornell", "tree"])
def test_cuda_semantics(scene):
    bundle, ds = uploaded(scene)
    p = helpers.params(37, 23, 4, 5, semantics=1)
    check_accumulate(bundle, ds, p, consecutive([(4, 1), (5, 3)]), whole(23), "render_kernel_cuda", scene)


# ---- the fold and the slice bounds ------------------------------------------------

# (S, spp_chunks): a strict batch; AUTO with 6 samples is 6 one-sample slices;
# 40 samples in 5 slices take the taper with L = 3 (weights 8, 8, 4, 2, 1)
FOLD = [(5, 1), (6, AUTO), (40, 5)]
VARIANTS = {"plain": {}, "ao": dict(use_ao=True, compat=0, ao=2.5), "aperture": dict(compat=0, aperture=(0.1, 0.05))}


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_fold_and_slice_bounds(variant, order):
    bundle, ds = uploaded("cornell")
    p = helpers.params(29, 19, 1, 5, **VARIANTS[variant])
    batches = consecutive(FOLD if order == "forward" else FOLD[::-1])
    check_accumulate(bundle, ds, p, batches, whole(19), "render_kernel", "%s %s" % (variant, order))


def test_no_bounces():
    """B = 0: the bounce loop does not run, so every sample is radiance, albedo
    and normal (0, 0, 0) and adds +0.0 to every sum.  From a start of -0.0 a
    written sum shows as +0.0 (-0.0 + 0.0), an unwritten one keeps its sign."""
    bundle, ds = uploaded("cornell")
    p = helpers.params(29, 19, 1, 0)
    check_accumulate(bundle, ds, p, consecutive(FOLD), whole(19), "render_kernel", "B = 0",
                     start=np.full((19, 29, 9), -0.0))


@pytest.mark.parametrize("W,H", [(1, 1), (1, 7), (9, 1), (2, 3)])
def test_tiny_frames(W, H):
    """With W or H of 1 the reference's camera divides by W - 1 or H - 1 = 0
    (main.c:265-266): every ray is non-finite, misses, and adds +0.0 -- on the
    device as in the oracle.  Those frames start from -0.0, so that a written
    sum shows (as +0.0); 2x3 is the smallest frame with finite rays and starts
    from the sentinel."""
    bundle, ds = uploaded("cornell")
    p = helpers.params(W, H, 1, 5)
    start = np.full((H, W, 9), -0.0) if min(W, H) == 1 else None
    check_accumulate(bundle, ds, p, consecutive(FOLD), whole(H), "render_kernel", "%dx%d" % (W, H), start=start)


# ---- the Philox sample word ---------------------------------------------------------

@pytest.mark.parametrize("offset", HIGH_OFFSETS, ids=["2^31-2", "2^32-4", "2^16-2"])
@pytest.mark.parametrize("scene", ["cornell", "tree"])
def test_sample_word(scene, offset):
    """A batch of 4 samples that crosses bit 31, ends exactly at 2^32, crosses
    bit 16; strict, then in 2 slices, onto the same accumulator.
    test_oracle_accumulate.test_the_high_offsets_can_show_a_cut_sample_word
    shows on the oracle that a word cut to 31 or 16 bits changes every pixel."""
    bundle, ds = uploaded(scene)
    W, H, B = WORD_FRAMES[scene]
    p = helpers.params(W, H, WORD_BATCH, B)
    check_accumulate(bundle, ds, p, [(offset, WORD_BATCH, 1), (offset, WORD_BATCH, 2)], whole(H), KERNEL[scene],
                     "%s at %d" % (scene, offset))


# ---- tilings ----------------------------------------------------------------------------

TW, TH = 37, 23
TILINGS = {"rows 5-17": lambda: tiling_of(5, 13, 0, 1, 1)}
for _k, _G in ((1, 2), (3, 4), (16, 2)):
    for _r in range(_G):
        TILINGS["k=%d G=%d r=%d" % (_k, _G, _r)] = (lambda k=_k, G=_G, r=_r: cyclic(TH, k, r, G))
PAST_H = {"k=1 G=2 r=1", "k=3 G=4 r=3", "k=16 G=2 r=1"}              # their last tile passes H
assert {n for n, make in TILINGS.items() if (global_rows(make()) >= TH).any()} == PAST_H


@pytest.mark.parametrize("name", list(TILINGS))
@pytest.mark.parametrize("scene", ["cornell", "tree"])
def test_tilings(scene, name):
    """The local frame layout li = ly*W + x under a sub-band and under cyclic
    tiles; the last tile of the ranks in PAST_H passes H, and those local rows
    keep the sentinel's bits (check_accumulate)."""
    bundle, ds = uploaded(scene)
    p = helpers.params(TW, TH, 4, 5)
    check_accumulate(bundle, ds, p, consecutive([(4, 1), (5, 3)], first=3), TILINGS[name](), KERNEL[scene],
                     "%s %s" % (scene, name))


# ---- row bands of the partial sums --------------------------------------------------------

@pytest.mark.parametrize("name", ["whole frame", "k=3 G=2 r=0", "k=3 G=2 r=1"])
def test_row_bands(name, monkeypatch):
    """A partial-sum budget of 16 rows (test_spp_chunks_row_bands's): the 53
    rows take 4 bands, a rank's 27 local rows 2, so combine_kernel folds onto
    the running sums with band_y0 > 0."""
    H = 53
    monkeypatch.setenv("RT_PARTIAL_BUDGET", str(16 * 37 * 4 * 72))
    bundle, ds = uploaded("cornell")
    p = helpers.params(37, H, 4, 5)
    t = whole(H) if name == "whole frame" else cyclic(H, 3, int(name[-1]), 2)
    check_accumulate(bundle, ds, p, consecutive([(4, 4), (3, 1), (6, 4)]), t, "render_kernel", name)


# ---- listed pixels ---------------------------------------------------------------------------

def lists_for(W, H):
    every = np.arange(W * H)
    yy, xx = np.divmod(every, W)
    rng = np.random.default_rng(W * 1000 + H)
    return {"checkerboard": every[(xx + yy) % 2 == 0],
            "65 entries": np.sort(rng.choice(W * H, 65, replace=False))}


@pytest.mark.parametrize("offset", LIST_OFFSETS, ids=["2^31-2", "2^32-4"])
@pytest.mark.parametrize("scene", sorted(WORD_FRAMES))
def test_listed_pixels_equal_the_oracle(scene, offset):
    """rt_accumulate_list_async against the oracle itself (test_adaptive_list
    compares it with rt_accumulate_async): a strict batch and one in 3 slices
    at a high offset; a listed pixel holds oracle_accumulate's sums of the
    whole-frame tiling, any other pixel the sentinel.  (The list kernels do
    not report through rt_last_render_kernel.)"""
    bundle, ds = uploaded(scene)
    W, H, B = WORD_FRAMES[scene]
    # the two starts of check_accumulate: what is not listed shows on the first, the order of the fold on the second
    for chunks, start in ((1, sentinel(W, H)), (3, sentinel(W, H)), (3, sentinel(W, H) * 2.0 ** -20)):
        p = helpers.params(W, H, WORD_BATCH, B, chunks=chunks)
        want = oracle_batches(bundle, p, [(offset, WORD_BATCH, chunks)], whole(H), start)
        assert (u64(want) != u64(start)).any(axis=2).all()
        for name, entries in lists_for(W, H).items():
            what = "%s P=%d %s from %g" % (scene, chunks, name, start[0, 0, 0])
            got = accumulate_list(ds, p, (offset,), start, entries)
            listed = np.zeros(W * H, dtype=bool)
            listed[entries] = True
            listed = listed.reshape(H, W)
            assert_same_sums(got[listed][None], want[listed][None], what)
            bad = u64(got)[~listed] != u64(start)[~listed]
            assert not bad.any(), "%s: %d values of unlisted pixels were written" % (what, bad.sum())


# ---- the adaptive loop -----------------------------------------------------------------------------

def test_adaptive_loop_equals_the_oracle():
    """rt_adaptive_async's A and B against accumulators built by
    oracle_accumulate along adaptive_support.schedule, each pixel taken from its
    own round count by the restated selection pass.  The tolerance is chosen as
    test_adaptive chooses it: the first of 2^(-e/2) at which every round count
    holds at least 5 % of the reference's pixels."""
    W, H, bounces = 40, 30, 5
    first_half, max_rounds = 4, 3
    bundle, ds = uploaded("glass")
    p = helpers.params(W, H, 999, bounces)                          # nbRayonParPixel is ignored
    acc = [np.zeros((H, W, 9)), np.zeros((H, W, 9))]
    per_round = []
    for o, b, _ in schedule(first_half, max_rounds):
        acc = [oracle_batches(bundle, p, [(o + k * b, b, 1)], whole(H), acc[k]) for k in range(2)]
        per_round.append((acc[0], acc[1]))
    for tol in [2.0 ** (-e / 2.0) for e in range(25)]:
        rounds = reference_rounds(per_round, first_half, tol)
        shares = [float((rounds == k).mean()) for k in range(1, max_rounds + 1)]
        if min(shares) >= 0.05:
            break
    assert min(shares) >= 0.05, shares
    ap = tipe_rt.adaptive_params(first_half=first_half, max_rounds=max_rounds, tolerance=tol)
    A, B, got_rounds, _ = device_adaptive(ds, p, ap, frame=False)
    assert tipe_rt.last_render_kernel() == "render_kernel"               # round 0's rt_accumulate_async launches
    assert (got_rounds == rounds).all(), "d_rounds differs at %d pixels" % int((got_rounds != rounds).sum())
    assert_same_sums(A, pick(per_round, rounds, 0), "A")
    assert_same_sums(B, pick(per_round, rounds, 1), "B")
    assert (A[..., 6:9] != 0).any(axis=2).all()                          # every pixel received samples
