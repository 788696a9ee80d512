"""sqrt_rcp_near1 / div_core0 (rt_device_math.h), the sampler's normalize
without v_rsq_f64, checked on the CPU against IEEE sqrt and division.

tests/near1_check.py cuts the functions' own source text out of the header and
compiles it with gcc, so the check runs the code the kernel runs.  This test
covers every double within 2^-30 of 1 (where sqrt(x) is closest to rounding
midpoints), a strided sweep of the whole domain [1 - 2^-18, 1 + 2^-18] and,
for every tested x, a pseudo-random numerator through div_core0 (plus +-0).
tools/archive/check_near1.sh runs all 5.2e10 doubles of the domain (about 4
minutes on 8 cores)."""
from near1_check import build, run


def test_near1_exhaustive_around_one(tmp_path):
    exe = build(tmp_path)
    n = run(exe, 1.0 - 2.0 ** -30, 1.0 + 2.0 ** -30, 1)
    assert n == 2 ** 23 + 2 ** 22 + 1


def test_near1_strided_whole_domain(tmp_path):
    exe = build(tmp_path)
    n = run(exe, 1.0 - 2.0 ** -18, 1.0 + 2.0 ** -18, 1009)
    assert n > 5 * 10 ** 7
