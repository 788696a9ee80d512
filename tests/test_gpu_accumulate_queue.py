"""rt_accumulate_async on the task-queue kernel (rt_set_accumulate_queue on)
against the CPU oracle's oracle_accumulate.

The contract is bits (accumulate_support.assert_same_sums): a slice partial
starts at +0.0 and takes its samples in order on either kernel, and
combine_kernel adds the partials to the running sums in slice order, so every
sum equals the oracle's uint64 for uint64.  No tolerance.

Every case runs one sequence of sliced batches into one accumulator that starts
from the sentinel scaled by 2^-20 (different in every pixel and slot, and small
against one sample, so a wrong fold order shows: accumulate_support
.check_accumulate): 8 samples in 3 slices, 6 more in AUTO's 6, then 4 samples
that cross bit 31 of the Philox sample word and 4 that end exactly at 2^32.
Each launch must report the pair's queue kernel; the guards around the
accumulator must stay untouched (accumulate_support.device_batches).  The
oracle's sums of a (scene, params, tiling) are computed once and shared by the
cases that only change how the device runs them."""
import functools

import pytest

import tipe_rt
from accumulate_support import (assert_rendered_rows_moved, assert_same_sums, cyclic, device_batches, global_rows,
                                local_rows, oracle_batches, tiling_of, whole)
from adaptive_support import sentinel
from queue_accumulate_support import FEATURED, PAIRS, PairUploads, accumulate_queue, params_of, queue_name
from tipe_rt.types import RT_SPP_CHUNKS_AUTO

pytestmark = pytest.mark.gpu

AUTO = RT_SPP_CHUNKS_AUTO
BATCHES = ((0, 8, 3), (8, 6, AUTO), ((1 << 31) - 2, 4, 2), ((1 << 32) - 4, 4, AUTO))
uploaded = PairUploads()


@pytest.fixture(scope="module", autouse=True)
def release_scenes():
    yield
    uploaded.release()
    assert tipe_rt.set_accumulate_queue(False) is False          # every test left the switch at its default


def start_of(p, tiling):
    return sentinel(p.largeur_image, local_rows(tiling)) * 2.0 ** -20


@functools.lru_cache(maxsize=None)
def oracle_sums(pair, sky, ao, H, tiling_fields):
    """The oracle's sums after BATCHES (read-only: shared between tests)."""
    bundle, _ = uploaded(pair, sky)
    p = params_of(pair, 1, sky, ao, H=H)
    t = tiling_of(*tiling_fields)
    start = start_of(p, t)
    want = oracle_batches(bundle, p, BATCHES, t, start)
    assert_rendered_rows_moved(want, start, t, p.hauteur_image, "oracle")
    want.setflags(write=False)
    return want


def fields(t):
    return (t.row_base, t.tile_rows, t.tile_first, t.tile_step, t.n_tiles)


def check(pair, sky=False, ao=False, H=None, tiling=None, what=""):
    """BATCHES on the device with the switch on: the pair's queue kernel in every launch, the oracle's bits."""
    bundle, ds = uploaded(pair, sky)
    p = params_of(pair, 1, sky, ao, H=H)
    t = tiling if tiling is not None else whole(p.hauteur_image)
    want = oracle_sums(pair, sky, ao, p.hauteur_image, fields(t))
    start = start_of(p, t)
    with accumulate_queue():
        got, kernels = device_batches(ds, p, BATCHES, t, start)
    what = "%s sky=%d ao=%d %s" % (pair, sky, ao, what)
    assert kernels == [queue_name(pair)] * len(BATCHES), "%s: kernels %r" % (what, kernels)
    assert_rendered_rows_moved(got, start, t, p.hauteur_image, what)
    assert_same_sums(got, want, what)


CASES = [(pair, False, False) for pair in PAIRS] + \
        [(pair, sky, ao) for pair in FEATURED for sky, ao in ((True, False), (False, True), (True, True))]


@pytest.mark.parametrize("pair,sky,ao", CASES, ids=["%s%s%s" % (c[0], "-sky" * c[1], "-ao" * c[2]) for c in CASES])
def test_every_pair(pair, sky, ao):
    check(pair, sky, ao)


@pytest.mark.parametrize("pair", list(PAIRS))
def test_two_blocks_take_every_task(pair, monkeypatch):
    """RT_QUEUE_BLOCKS=2: eight waves share the band's tasks, so every lane takes many, one after the other."""
    monkeypatch.setenv("RT_QUEUE_BLOCKS", "2")
    check(pair, what="RT_QUEUE_BLOCKS=2")


@pytest.mark.parametrize("pair", list(PAIRS))
def test_zero_throughput_exit_off(pair):
    """The exit changes the work, never a sum: the same oracle bits."""
    prev = tipe_rt.set_zero_throughput_exit(False)
    try:
        check(pair, what="zero exit off")
    finally:
        tipe_rt.set_zero_throughput_exit(prev)


@pytest.mark.parametrize("pair", FEATURED)
def test_row_bands(pair, monkeypatch):
    """A partial budget of 16 rows of 21 pixels in 2 slices: every batch of the
    21x40 frame (2 to 6 slices) takes bands of 16 rows, three of them, so
    decode_task and combine_kernel run with band_y0 > 0 and a last band of 8."""
    monkeypatch.setenv("RT_PARTIAL_BUDGET", str(16 * 21 * 2 * 72))
    check(pair, H=40, what="3 bands")


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("pair", FEATURED)
def test_cyclic_tiles_with_padding_rows(pair, rank):
    """13 rows in tiles of 3 over 2 ranks, three tiles each: rank 0 holds tiles
    0, 2, 4, whose last passes H by two rows; rank 1 holds tiles 1, 3, 5, whose
    last lies past H altogether.  Those rows are tasks without work and keep
    their start (assert_rendered_rows_moved)."""
    t = cyclic(13, 3, rank, 2)
    assert int((global_rows(t) >= 13).sum()) == (2, 3)[rank]
    check(pair, tiling=t, what="k=3 G=2 r=%d" % rank)


@pytest.mark.parametrize("pair", FEATURED)
def test_sub_band(pair):
    check(pair, tiling=tiling_of(3, 7, 0, 1, 1), what="rows 3-9")


def test_the_switch_defaults_to_off_and_returns_the_previous_setting():
    assert tipe_rt.set_accumulate_queue(True) is False
    try:
        assert tipe_rt.set_accumulate_queue(True) is True
        assert tipe_rt.lib().rt_set_accumulate_queue(7) == 1         # any non-zero value is "on"
        assert tipe_rt.lib().rt_set_accumulate_queue(0) == 1
        assert tipe_rt.lib().rt_set_accumulate_queue(0) == 0
    finally:
        tipe_rt.set_accumulate_queue(False)


def test_off_and_one_slice_keep_the_fixed_grid():
    """Switch off: today's kernel.  Switch on with one slice: the fixed grid carries the sums in sample order."""
    bundle, ds = uploaded("QB-2")
    p = params_of("QB-2", 1)
    t = whole(p.hauteur_image)
    start = start_of(p, t)
    _, off = device_batches(ds, p, BATCHES[:2], t, start)
    assert off == ["render_kernel"] * 2
    with accumulate_queue():
        _, one = device_batches(ds, p, [(0, 4, 1)], t, start)
    assert one == ["render_kernel"]
