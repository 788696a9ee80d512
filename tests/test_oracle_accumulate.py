"""oracle_accumulate (the CPU restatement of rt_accumulate_async, rt.h
"progressive rendering") tied to the pinned oracle_render_rows: batches equal
the one-shot frame, a chunked batch equals the chunked frame, every tiling's
local rows equal the whole frame's global rows, the thread count changes
nothing, bad arguments are refused -- and the high sample offsets the GPU
tests use are able to show a cut sample word.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle_ffi
from accumulate_support import (HIGH_OFFSETS, LIST_OFFSETS, SCENES, WORD_BATCH, WORD_FRAMES, consecutive, cyclic,
                                global_rows, local_rows, oracle_accumulate, oracle_batches, tiling_of,
                                truncated_batches, whole)
from adaptive_support import sentinel, u64
from tipe_rt.types import RT_EINVAL, RT_RNG_GLIBC, Vec3

W, H, BOUNCES = 12, 9, 5
BUNDLES = {}


def bundle_of(name):
    if name not in BUNDLES:
        BUNDLES[name] = SCENES[name][0]()
    return BUNDLES[name]


def resolved(sums, S):
    """The four planes of running sums: write_color_canva and sum / S (main.c:275-279)."""
    lib = oracle_ffi.oracle()
    canva = np.empty(sums.shape[:2] + (3,))
    for j in range(sums.shape[0]):
        for i in range(sums.shape[1]):
            c = lib.oracle_write_color_canva(Vec3(*sums[j, i, 0:3]), S)
            canva[j, i] = (c.e[0], c.e[1], c.e[2])
    return dict(canva=canva, albedo=sums[..., 3:6] / S, normal=sums[..., 6:9] / S, radiance=sums[..., 0:3] / S)


@pytest.mark.parametrize("scene", ["cornell", "pyramid"])
@pytest.mark.parametrize("batches", [[12], [5, 7], [1, 1, 10]])
def test_batches_equal_the_one_shot_frame(scene, batches):
    bundle = bundle_of(scene)
    p = helpers.params(W, H, 12, BOUNCES)
    ref = helpers.oracle_render(bundle, p)
    sums = oracle_batches(bundle, p, consecutive([(n, 1) for n in batches]), whole(H), np.zeros((H, W, 9)))
    got = resolved(sums, 12)
    assert ref["radiance"].any()
    for name in ("canva", "albedo", "normal", "radiance"):
        assert (u64(got[name]) == u64(ref[name])).all(), name


@pytest.mark.parametrize("scene", ["cornell", "pyramid"])
@pytest.mark.parametrize("chunks", [3, 6])
def test_a_chunked_batch_equals_the_chunked_frame(scene, chunks):
    """S = 48: P = 3 has equal slices, P = 6 the taper with L = 3.  By value
    (==), not by bits: the frame starts its total as tot = part_0, the
    accumulator as 0.0 + part_0, which differ in the sign of a zero whenever
    part_0 is -0.0.  (Each part_c is itself 0.0 + sample + ..., which is never
    -0.0, so here the bits agree too; the rule for this test is the value.)"""
    bundle = bundle_of(scene)
    S = 48
    p = helpers.params(W, H, S, BOUNCES, chunks=chunks)
    ref = helpers.oracle_render(bundle, p)
    got = resolved(oracle_batches(bundle, p, [(0, S, chunks)], whole(H), np.zeros((H, W, 9))), S)
    for name in ("canva", "albedo", "normal", "radiance"):
        assert (got[name] == ref[name]).all(), name
    # the grouping is a different fold from the strict one: the check above is not vacuous
    strict = helpers.oracle_render(bundle, helpers.params(W, H, S, BOUNCES, chunks=1))
    assert (strict["radiance"] != ref["radiance"]).any()


TILINGS = [("sub-band", lambda: tiling_of(2, 5, 0, 1, 1))] + \
          [("cyclic k=2 G=3 r=%d" % r, lambda r=r: cyclic(H, 2, r, 3)) for r in range(3)] + \
          [("cyclic k=1 G=2 r=%d" % r, lambda r=r: cyclic(H, 1, r, 2)) for r in range(2)]


@pytest.mark.parametrize("scene", ["cornell", "pyramid"])
@pytest.mark.parametrize("chunks", [1, 3])
def test_local_rows_equal_the_whole_frames_global_rows(scene, chunks):
    bundle = bundle_of(scene)
    p = helpers.params(W, H, 4, BOUNCES)
    batches = [(7, 4, chunks), (11, 3, 1)]
    frame_start = sentinel(W, H)
    full = oracle_batches(bundle, p, batches, whole(H), frame_start)
    assert (u64(full) != u64(frame_start)).any(axis=2).all()
    past_h = 0
    for name, make in TILINGS:
        t = make()
        # each local row starts from its global row's start, so both calls fold from the same bits;
        # a row past H starts from a pattern of its own
        start = sentinel(W, local_rows(t)) * 3.0
        for ly, g in enumerate(global_rows(t)):
            if g < H:
                start[ly] = frame_start[g]
        got = oracle_batches(bundle, p, batches, t, start)
        for ly, g in enumerate(global_rows(t)):
            if g >= H:
                past_h += 1
                assert (u64(got[ly]) == u64(start[ly])).all(), (name, ly)
            else:
                assert (u64(got[ly]) == u64(full[g])).all(), (name, ly, g)
    assert past_h > 0                                        # (G = 3, k = 2, H = 9): 5 tiles, rank 2 has a padding tile


@pytest.mark.parametrize("scene", ["cornell", "pyramid"])
def test_thread_count_changes_nothing(scene):
    bundle = bundle_of(scene)
    p = helpers.params(W, H, 5, BOUNCES)
    for t in (whole(H), cyclic(H, 2, 2, 3)):
        start = sentinel(W, local_rows(t))
        a = oracle_batches(bundle, p, [(3, 5, 3)], t, start, nthreads=1)
        b = oracle_batches(bundle, p, [(3, 5, 3)], t, start, nthreads=4)
        assert a.tobytes() == b.tobytes()
        assert a.tobytes() != start.tobytes()


def test_refusals():
    bundle = bundle_of("cornell")
    good = helpers.params(W, H, 4, BOUNCES)
    lib = oracle_ffi.oracle()
    sums = np.zeros((H, W, 9))
    before = sums.tobytes()

    def run(p=good, off=0, t=None, s=sums):
        t = t if t is not None else whole(H)
        return oracle_accumulate(bundle, p, off, t, s)

    assert run() == 0 and sums.tobytes() != before
    before = sums.tobytes()
    assert lib.oracle_accumulate(C.byref(bundle.scene), C.byref(good), 0, None, 1, sums.ctypes.data) == RT_EINVAL
    assert lib.oracle_accumulate(C.byref(bundle.scene), C.byref(good), 0, C.byref(whole(H)), 1, None) == RT_EINVAL
    assert lib.oracle_accumulate(None, C.byref(good), 0, C.byref(whole(H)), 1, sums.ctypes.data) == RT_EINVAL
    for fields in ((0, 0, 0, 1, 1), (0, H, 0, 0, 1), (0, H, 0, 1, 0), (0, -1, 0, 1, 1), (-1, H, 0, 1, 1),
                   (0, H, -1, 1, 1)):
        assert lib.oracle_accumulate(C.byref(bundle.scene), C.byref(good), 0, C.byref(tiling_of(*fields)), 1,
                                     sums.ctypes.data) == RT_EINVAL, fields
    assert run(off=-1) == RT_EINVAL
    assert run(off=(1 << 32) - 3) == RT_EINVAL               # [2^32 - 3, 2^32 + 1)
    assert run(off=1 << 32) == RT_EINVAL
    assert run(p=helpers.params(W, H, 4, BOUNCES, rng=RT_RNG_GLIBC)) == RT_EINVAL
    assert run(p=helpers.params(W, H, 0, BOUNCES)) == RT_EINVAL          # validate()'s own
    assert run(p=helpers.params(W, H, 4, -1)) == RT_EINVAL
    assert run(p=helpers.params(W, H, 4, BOUNCES, semantics=1, sky_mode=1)) == RT_EINVAL
    assert sums.tobytes() == before                          # a refused call writes nothing
    assert run(off=(1 << 32) - 4) == 0                       # ends exactly at 2^32


@pytest.mark.parametrize("scene", sorted(WORD_FRAMES))
def test_the_high_offsets_can_show_a_cut_sample_word(scene):
    """A condition on the inputs of the GPU tests, checked on the reference
    alone.  A kernel that cut the sample word (offset + x) to 31 or to 16 bits
    would draw the streams of the samples (offset + x) mod 2^31 or mod 2^16;
    for every high offset X whose batch such a cut changes at all, the oracle's
    sums of the cut samples differ from its sums at X in every pixel of the
    frame the GPU test renders, so the cut cannot pass there.  (2^31 - 2 and
    2^16 - 2 lie below 2^31, so a 31-bit cut changes only the samples past the
    crossing of the first and nothing of the second; each width is changed by
    at least one offset, asserted below.)"""
    bundle = bundle_of(scene)
    Wf, Hf, bounces = WORD_FRAMES[scene]
    p = helpers.params(Wf, Hf, WORD_BATCH, bounces, **SCENES[scene][1])
    start = np.zeros((Hf, Wf, 9))
    touched = set()
    for X in (LIST_OFFSETS if scene == "wide" else HIGH_OFFSETS):    # the wide tree runs the list offsets only
        true = [(X, WORD_BATCH, 1)]
        at_x = oracle_batches(bundle, p, true, whole(Hf), start)
        for bits in (31, 16):
            cut = truncated_batches(X, WORD_BATCH, bits)
            if cut == true:
                continue
            touched.add(bits)
            other = oracle_batches(bundle, p, cut, whole(Hf), start)
            differs = (u64(other) != u64(at_x)).any(axis=2)
            assert differs.all(), "offset %d cut to %d bits: %d pixels tie" % (X, bits, (~differs).sum())
    assert touched == {31, 16}
    assert truncated_batches((1 << 31) - 2, 4, 31) == [((1 << 31) - 2, 2, 1), (0, 2, 1)]
    assert truncated_batches((1 << 32) - 4, 4, 31) == [((1 << 31) - 4, 4, 1)]
    assert truncated_batches((1 << 16) - 2, 4, 31) == [((1 << 16) - 2, 4, 1)]
