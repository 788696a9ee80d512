"""CPU checks of rt_shared_math.h, the arithmetic the paired-draw kernels
(render_kernel_q<QB=-2> without AO) run in place of per-round work:

* sphere_halfb, hit_sphere in half-b units, against the oracle's hit_sphere
  (sphere.h:13-47 as oracle/rt_oracle.c states it): didHit and dst bit for bit
  on a million random rays and spheres and on edge cases, and "not fast",
  never another t, outside the shifted windows;
* philox_head and the block started from it against the full Philox4x32-10
  (this header's and the oracle's), word for word.

tools/probes/round_trims_check.cpp includes the header as it stands, so the
check runs the code the kernel runs (with IEEE sqrt and division where the
kernel has its exact cores, which the GPU suite compares with the oracle).
"""
import os
import subprocess

import pytest

import oracle_ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tipe-raytracer_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not os.path.exists(oracle_ffi.ORACLE_SO):
        oracle_ffi.build_oracle()
    exe = str(tmp_path_factory.mktemp("trims") / "round_trims_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    "-o", exe, os.path.join(ROOT, "tools", "probes", "round_trims_check.cpp"),
                    oracle_ffi.ORACLE_SO, "-Wl,-rpath," + oracle_ffi.ORACLE_DIR], check=True)
    return exe


def counts(checker, *args):
    p = subprocess.run([checker, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    words = p.stdout.strip().splitlines()[-1].split()
    assert words[0] == args[0]
    return dict(zip(words[1::2], map(int, words[2::2])))


def test_halfb_equals_the_reference_formula(checker):
    c = counts(checker, "halfb", 10 ** 6, 20261)
    assert c["bad"] == 0
    assert c["random_fast"] >= 10 ** 6 - 10      # the random and edge cases all lie inside the windows
    assert c["hits"] > 10 ** 5
    # the sweep beyond the windows: some of it answered, the rest reported as not fast
    assert c["notfast"] > 10 ** 4 and c["fast"] - c["random_fast"] > 10 ** 4
    assert c["fast"] + c["notfast"] == c["n"]


def test_philox_head_equals_the_full_block(checker):
    c = counts(checker, "philox", 10 ** 5, 20262)
    assert c == {"n": 10 ** 5, "bad": 0}
