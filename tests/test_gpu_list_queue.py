"""rt_accumulate_list_async on the task-queue list kernel render_kernel_ql
(rt_set_accumulate_queue on) against the CPU oracle's oracle_accumulate.

A listed pixel holds the oracle's sums of the whole-frame tiling, bit for bit
(accumulate_support.assert_same_sums); any other pixel keeps its start.  Both of
check_accumulate's starts run: the sentinel, where an unlisted pixel that was
written shows, and the sentinel scaled by 2^-20, where the order of the fold
shows.  The batch is accumulate_support's 4 samples at LIST_OFFSETS (across bit
31 of the Philox sample word; ending at 2^32), in 3 slices and in AUTO's 4.

The list room is the frame (list_cap 273 = 21x13; the wide tree's frame is
16x12 = 192).  Counts: none, one, one short of and one past a wave, one past a
block of 256, the whole frame, and a count word above list_cap, which the
kernel clamps.  Every list of two or more entries ends with one index that is
not a pixel (W * H + 3): a task without work, which must write nothing.  The
oracle's frame of a (pair, slices, offset, start) is computed once."""
import functools

import numpy as np
import pytest

import tipe_rt
from accumulate_support import LIST_OFFSETS, WORD_BATCH, assert_same_sums, oracle_batches, whole
from adaptive_support import accumulate_list, sentinel, u64
from queue_accumulate_support import FEATURED, PAIRS, PairUploads, accumulate_queue, frame_of, list_name, params_of
from tipe_rt.types import RT_SPP_CHUNKS_AUTO

pytestmark = pytest.mark.gpu

AUTO = RT_SPP_CHUNKS_AUTO
SLICES = (3, AUTO)
SCALES = (1.0, 2.0 ** -20)
uploaded = PairUploads()


@pytest.fixture(scope="module", autouse=True)
def release_scenes():
    yield
    uploaded.release()
    assert tipe_rt.set_accumulate_queue(False) is False


def counts_of(npx):
    return [c for c in (0, 1, 63, 65, 257) if c < npx] + [npx]


def entries_of(npx, count):
    """`count` ascending entries: pixels, the last one (of two or more) an index beyond the frame."""
    rng = np.random.default_rng(1000 * npx + count)
    e = np.sort(rng.choice(npx, count, replace=False)).astype(np.int64)
    if count >= 2:
        e[-1] = npx + 3
    return e


@functools.lru_cache(maxsize=None)
def oracle_frame(pair, sky, ao, chunks, offset, scale):
    bundle, _ = uploaded(pair, sky)
    W, H, _ = frame_of(pair)
    p = params_of(pair, WORD_BATCH, sky, ao, chunks=chunks)
    start = sentinel(W, H) * scale
    want = oracle_batches(bundle, p, [(offset, WORD_BATCH, chunks)], whole(H), start)
    assert (u64(want) != u64(start)).any(axis=2).all()
    want.setflags(write=False)
    return want


def check_lists(pair, sky=False, ao=False, counts=None, what=""):
    bundle, ds = uploaded(pair, sky)
    W, H, _ = frame_of(pair)
    npx = W * H
    for chunks in SLICES:
        p = params_of(pair, WORD_BATCH, sky, ao, chunks=chunks)
        for offset in LIST_OFFSETS:
            for scale in SCALES:
                start = sentinel(W, H) * scale
                want = oracle_frame(pair, sky, ao, chunks, offset, scale)
                for count in counts if counts is not None else counts_of(npx):
                    entries = entries_of(npx, count)
                    # once more with a count word above list_cap: the launch clamps it to the room
                    for word in (None, npx + 1000) if count == npx else (None,):
                        tag = "%s %s P=%d at %d from %g: %d entries, count word %r" % (
                            pair, what, chunks, offset, start[0, 0, 0], count, word)
                        with accumulate_queue():
                            got = accumulate_list(ds, p, (offset,), start, entries, count=word)
                            kernel = tipe_rt.last_list_kernel()
                        assert kernel == list_name(pair), "%s: %s" % (tag, kernel)
                        listed = np.zeros(npx, dtype=bool)
                        listed[entries[entries < npx]] = True
                        listed = listed.reshape(H, W)
                        assert listed.sum() == max(count - (count >= 2), 0)
                        assert_same_sums(got[listed][None], want[listed][None], tag)
                        bad = u64(got)[~listed] != u64(start)[~listed]
                        assert not bad.any(), "%s: %d values of unlisted pixels were written" % (tag, bad.sum())


CASES = [(pair, False, False) for pair in PAIRS] + \
        [(pair, sky, ao) for pair in FEATURED for sky, ao in ((True, False), (False, True), (True, True))]


@pytest.mark.parametrize("pair,sky,ao", CASES, ids=["%s%s%s" % (c[0], "-sky" * c[1], "-ao" * c[2]) for c in CASES])
def test_every_pair(pair, sky, ao):
    check_lists(pair, sky, ao)


@pytest.mark.parametrize("pair", ["QB-2", "QB3", "QB4"])
def test_two_bands(pair, monkeypatch):
    """RT_LIST_BAND=256: the 273 entries of room take bands [0, 256) and [256, 273); the second band's
    prologue finds 17, 1 or no entries of its own."""
    monkeypatch.setenv("RT_LIST_BAND", "256")
    check_lists(pair, counts=(0, 65, 256, 257, 273), what="RT_LIST_BAND=256")


@pytest.mark.parametrize("pair", ["QB-2", "QB3OP"])
def test_two_blocks_take_every_task(pair, monkeypatch):
    monkeypatch.setenv("RT_QUEUE_BLOCKS", "2")
    check_lists(pair, counts=(65, 273), what="RT_QUEUE_BLOCKS=2")


def test_none_before_a_thread_s_first_list_launch():
    """rt_last_list_kernel is per thread, as rt_last_render_kernel: a fresh thread has launched no list."""
    import threading
    out = []
    th = threading.Thread(target=lambda: out.append(tipe_rt.last_list_kernel()))
    th.start()
    th.join()
    assert out == ["none"]


def test_one_slice_and_the_switch_off_report_a_fixed_list_kernel():
    for pair, fixed in (("QB-2", "render_kernel_list"), ("QB3OP", "render_kernel_list<BVH>"),
                        ("QB5", "render_kernel_list_w")):
        _, ds = uploaded(pair)
        w, h, _ = frame_of(pair)
        with accumulate_queue():
            accumulate_list(ds, params_of(pair, WORD_BATCH, chunks=1), (0,), sentinel(w, h), entries_of(w * h, 65))
            assert tipe_rt.last_list_kernel() == fixed                   # P = 1 carries the sums: fixed grid
            accumulate_list(ds, params_of(pair, WORD_BATCH, chunks=3), (0,), sentinel(w, h), entries_of(w * h, 65))
            assert tipe_rt.last_list_kernel() == list_name(pair)
        accumulate_list(ds, params_of(pair, WORD_BATCH, chunks=3), (0,), sentinel(w, h), entries_of(w * h, 65))
        assert tipe_rt.last_list_kernel() == fixed                       # the switch is off again
    # list launches never report through rt_last_render_kernel
    _, ds = uploaded("QB-2")
    W, H, _ = frame_of("QB-2")
    before = tipe_rt.last_render_kernel()
    with accumulate_queue():
        accumulate_list(ds, params_of("QB-2", WORD_BATCH, chunks=3), (0,), sentinel(W, H), entries_of(W * H, 65))
    assert tipe_rt.last_render_kernel() == before
