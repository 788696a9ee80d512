"""rt_count_async's event totals against the oracle's counters, and the
zero-throughput exit they make visible: paths that end once rayColor == 0
change no plane and only remove casts."""
import numpy as np
import pytest

import helpers
import tipe_rt
from gpu_driver import assert_same_frame, check_parity, gpu_counts, gpu_render

pytestmark = pytest.mark.gpu


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
    ref = helpers.oracle_render(bundle, p, counters=True)["counters"]
    cnt = gpu_counts(bundle, p)
    assert cnt[tipe_rt.types.RT_CNT_CASTS] == ref[tipe_rt.types.RT_CNT_CASTS]
    bundle = helpers.cornell()
    p = helpers.params(16, 12, 4, 6, use_ao=True, ao=2000.0, compat=0)
    check_parity(bundle, p)
    ref = helpers.oracle_render(bundle, p, counters=True)["counters"]
    cnt = gpu_counts(bundle, p)
    assert cnt[tipe_rt.types.RT_CNT_CASTS] == ref[tipe_rt.types.RT_CNT_CASTS]
