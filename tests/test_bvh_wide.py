"""Host check of wide BVHs (rt_bvh.cpp), CPU only.

A mesh of more than 65535 triangles gets a wide tree: node or triangle indices
beyond 16 bits, walked with wider stack entries and, in the queue kernel, from
64-byte BvhNodeW nodes whose children are two 32-bit bases plus the count
nibbles (rt_bvh.h).  tools/probes/bvh_wide_check.cpp builds the tree of one
mesh with g++ (rt_bvh.cpp is plain C++) and checks what the kernels rely on:
the children decoded by the kernel's prefix sums equal the BvhNode4's, every
binary16 box contains its float box, the leaf order is a permutation, and
bvh_step's push rule stays within the stack bound.  Every case here needs a
tree that build_bvh refused before wide trees existed.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from tipe_rt import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tools", "probes", "bvh_wide_check.cpp"),
       os.path.join(ROOT, "tipe-raytracer_amd", "csrc", "rt_bvh.cpp")]
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tipe-raytracer_amd", "csrc")]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bvhw") / "bvh_wide_check")
    subprocess.run(["g++", "-O2", "-std=c++17"] + INC + ["-o", exe] + SRC, check=True)
    return exe


def text_of(rows):
    return "\n".join(" ".join(map(repr, row)) for row in np.asarray(rows, dtype=np.float64).tolist()) + "\n"


def heightfield_rows(n):
    tris = scenes.heightfield_mesh(n, 1, 0.25, scenes.README_FLOOR)[0]
    return np.frombuffer(tris, dtype=np.float64).reshape(len(tris), -1)[:, :9].copy()


@pytest.fixture(scope="module")
def hf182():
    rows = heightfield_rows(182)
    return rows, text_of(rows)


def run(exe, text, rays=2000, env=None):
    p = subprocess.run([exe, str(rays)], input=text, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def assert_wide_tree_is_sound(rec, nt):
    assert rec["bvh"] and rec["nt"] == nt, rec
    assert rec["wide"] and rec["packed"], rec
    assert rec["child_mismatch"] == 0 and rec["box_fail"] == 0 and rec["order_valid"], rec
    assert rec["max_leaf_triangle"] == nt - 1, rec
    assert rec["all_hit_peak"] <= rec["stack4"] and rec["ray_peak"] <= rec["stack4"], rec


def test_66248_triangles_triangle_indices_beyond_16_bits(checker, hf182):
    rec = run(checker, hf182[1])
    assert_wide_tree_is_sound(rec, 66248)
    assert rec["max_leaf_triangle"] > 65535 >= rec["max_internal_child"], rec
    assert (rec["nodes"], rec["depth4"], rec["stack4"]) == (32293, 9, 25), rec


def test_180000_triangles_node_indices_beyond_16_bits(checker):
    rec = run(checker, text_of(heightfield_rows(300)))
    assert_wide_tree_is_sound(rec, 180000)
    assert rec["nodes"] > 65536 and rec["max_internal_child"] > 65535, rec
    assert (rec["nodes"], rec["depth4"], rec["stack4"]) == (90671, 9, 27), rec


def test_leaves_of_four_exercise_the_leaf_count_prefix_sums(checker, hf182):
    rec = run(checker, hf182[1], env={"RT_BVH_LEAF": "4"})
    assert_wide_tree_is_sound(rec, 66248)
    assert rec["nodes"] < 32293 // 2, rec                # leaves hold several triangles


def test_soup_beyond_binary16_is_wide_but_does_not_pack(checker):
    """Coordinates ~1e5: the 64-byte form refuses, the tree renders on the fixed grid."""
    rng = np.random.default_rng(3)
    n = 66000
    c = 1e5 * rng.uniform(-1, 1, (n, 3))
    rows = np.concatenate([c, c + 2e3 * rng.normal(size=(n, 3)), c + 2e3 * rng.normal(size=(n, 3))], axis=1)
    rec = run(checker, text_of(rows), rays=200)
    assert rec["bvh"] and rec["wide"] and not rec["packed"], rec
    assert rec["order_valid"] and rec["all_hit_peak"] <= rec["stack4"] and rec["ray_peak"] <= rec["stack4"], rec


@pytest.mark.parametrize("nt,wide", [(65535, False), (65536, True)])
def test_boundary_between_narrow_and_wide(checker, hf182, nt, wide):
    rec = run(checker, text_of(hf182[0][:nt]), rays=200)
    assert rec["bvh"] and rec["nt"] == nt and rec["wide"] == wide, rec
    assert rec["order_valid"] and rec["all_hit_peak"] <= rec["stack4"], rec
    if wide:
        assert rec["packed"] and rec["child_mismatch"] == 0 and rec["box_fail"] == 0, rec


def test_probe_under_address_and_undefined_sanitizers(tmp_path, hf182):
    """The stand-alone host program itself, built with the sanitizers."""
    exe = str(tmp_path / "bvh_wide_check_san")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                   + INC + ["-o", exe] + SRC, check=True)
    rec = run(exe, hf182[1], rays=200)
    assert_wide_tree_is_sound(rec, 66248)
