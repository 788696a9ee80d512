"""rt_accumulate_list_async (rt.h "adaptive sampling", layer 1): samples for
listed pixels only.  A listed pixel must hold, bit for bit, what the same two
rt_accumulate_async calls give it on a copy of the accumulator; a pixel that is
not listed must keep its sentinel bits.  Six kernel instantiations (no tree,
narrow tree, wide tree; sky off / on), spp_chunks 1, 3 and AUTO, several entry
bands, partial waves and blocks, a count beyond list_cap."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import tipe_rt
from accumulate_support import SCENES
from adaptive_support import accumulate_dense, accumulate_list, sentinel, u64
from tipe_rt.types import RT_EINVAL, RT_EUNSUPPORTED, RT_SPP_CHUNKS_AUTO

_UPLOADED = {}


def uploaded(name):
    """(bundle, device scene) of a scene, uploaded once for the module."""
    if name not in _UPLOADED:
        bundle = SCENES[name][0]()
        _UPLOADED[name] = (bundle, tipe_rt.DeviceScene(bundle.scene, 0))
    return _UPLOADED[name]


@pytest.fixture(scope="module", autouse=True)
def release_scenes():
    """The uploads live for the module and are released with it."""
    yield
    for name in SCENES:
        if name in _UPLOADED:
            _UPLOADED.pop(name)[1].close()


def lists_for(W, H):
    """{name: (entries, count, list_cap)} over a W x H frame."""
    npx = W * H
    every = np.arange(npx)
    yy, xx = np.divmod(every, W)
    out = {
        "empty": ([], 0, npx),
        "last pixel": ([npx - 1], 1, npx),
        "every pixel": (every, npx, npx),
        "checkerboard": (every[(xx + yy) % 2 == 0], None, npx),
        "count beyond list_cap": (every[::2][:min(150, npx // 2)], None, 40),
    }
    rng = np.random.default_rng(W * 1000 + H)
    for n in (65, 257):                          # a partial wave, a partial block
        if n < npx:
            out["%d entries" % n] = (np.sort(rng.choice(npx, n, replace=False)), None, npx)
    return out


# (scene, W, H, batch size, spp_chunks, RT_LIST_BAND): W is no multiple of 16 in most; AUTO with a
# batch of 6 samples is P = 6; a band of 256 entries gives the 37x23 and 40x30 frames 4 and 5 bands
CASES = [("cornell", 40, 30, 4, 1, None),
         ("cornell", 37, 23, 5, 3, None),
         ("cornell", 40, 30, 6, RT_SPP_CHUNKS_AUTO, "256"),
         ("pyramid", 37, 23, 4, 1, None),
         ("pyramid", 37, 23, 4, 3, "256"),
         ("tree", 37, 23, 4, 1, None),
         ("tree", 40, 30, 6, RT_SPP_CHUNKS_AUTO, None),
         ("sky", 37, 23, 4, 1, None),
         ("sky", 37, 23, 4, 3, None),
         ("sky_tree", 37, 23, 4, 3, None),
         ("wide", 16, 12, 4, 1, None),
         ("wide", 16, 12, 4, 3, None),
         ("wide_sky", 16, 12, 4, 3, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("scene,W,H,S,chunks,band", CASES,
                         ids=["%s-%dx%d-S%d-P%s-band%s" % c for c in CASES])
def test_listed_pixels_equal_the_dense_accumulate(scene, W, H, S, chunks, band, monkeypatch):
    bundle, ds = uploaded(scene)
    p = helpers.params(W, H, S, 5, chunks=chunks, **SCENES[scene][1])
    if band:
        monkeypatch.setenv("RT_LIST_BAND", band)
    start = sentinel(W, H)
    offsets = (0, 3 * S)
    want = accumulate_dense(ds, p, offsets, start)         # computed once, shared by every list below
    assert (u64(want) != u64(start)).any(axis=2).all()     # every pixel's sums moved
    for name, (entries, count, cap) in lists_for(W, H).items():
        got = accumulate_list(ds, p, offsets, start, entries, count=count, cap=cap)
        listed = np.zeros(W * H, dtype=bool)
        listed[np.asarray(entries, dtype=np.int64)[:cap]] = True
        listed = listed.reshape(H, W)
        bad = u64(got)[listed] != u64(want)[listed]
        assert not bad.any(), "%s: %d listed values differ from rt_accumulate_async" % (name, bad.sum())
        bad = u64(got)[~listed] != u64(start)[~listed]
        assert not bad.any(), "%s: %d values of unlisted pixels were written" % (name, bad.sum())


@pytest.mark.gpu
def test_an_index_outside_the_frame_is_skipped():
    """Device data is not validated, but an entry that is no pixel writes nothing."""
    bundle, ds = uploaded("cornell")
    W, H = 24, 10
    p = helpers.params(W, H, 3, 4, chunks=3)
    start = sentinel(W, H)
    got = accumulate_list(ds, p, (0,), start, [5, W * H, W * H + 7], cap=W * H)
    want = accumulate_dense(ds, p, (0,), start)
    assert (u64(got)[0, 5] == u64(want)[0, 5]).all()
    keep = np.ones((H, W), dtype=bool)
    keep[0, 5] = False
    assert (u64(got)[keep] == u64(start)[keep]).all()


def test_validation_fails_before_any_device_work():
    """Refused arguments are reported with a message before the scene or any
    device pointer is used (they are not real: nothing may dereference them)."""
    L = tipe_rt.lib()
    fake = 0x10000
    W, H = 8, 6

    def run(scene=fake, p=None, off=0, lst=fake, cnt=fake, cap=W * H, sums=fake, **kw):
        p = p if p is not None else helpers.params(W, H, 4, 3, **kw)
        return L.rt_accumulate_list_async(scene, C.byref(p), off, lst, cnt, cap, sums, None)

    def refused(rc, code=RT_EINVAL):
        assert rc == code, rc
        assert L.rt_last_error()

    refused(run(scene=None))
    refused(run(lst=None))
    refused(run(cnt=None))
    refused(run(sums=None))
    refused(run(cap=0))
    refused(run(cap=W * H + 1))
    refused(run(off=-1))
    refused(run(off=(1 << 32) - 3))
    refused(run(semantics=1), RT_EUNSUPPORTED)
    refused(L.rt_accumulate_list_async(fake, None, 0, fake, fake, 4, fake, None))
    bad = helpers.params(W, H, 0, 3)
    refused(run(p=bad))


LIST_PLAN_CPP = r"""
#include <cstdio>
#include <cstdlib>
#include "rt_launch_plan.h"
int main(int argc, char** argv) {
  for (int i = 1; i + 1 < argc; i += 2) {
    const rt::ListPlan pl = rt::plan_list(std::atoi(argv[i]), (unsigned)std::strtoul(argv[i + 1], nullptr, 10));
    std::printf("%u %zu\n", pl.band, pl.partial_bytes);
  }
  return 0;
}
"""


def test_band_and_partials_follow_the_list(tmp_path, monkeypatch):
    """plan_list (host only): the partial buffer of a chunked list launch is what
    list_cap entries need, in whole blocks of 256, and at most 512 MiB; a
    1200x900 frame at P = 32 takes five bands; RT_LIST_BAND only shrinks a band."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "tipe-raytracer_amd", "csrc")
    src = tmp_path / "list_plan.cpp"
    src.write_text(LIST_PLAN_CPP)
    exe = str(tmp_path / "list_plan")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(root, "include"), "-I" + csrc,
                    "-o", exe, str(src)] + [os.path.join(csrc, f) for f in
                                            ("rt_launch_plan.cpp", "rt_scene_prep.cpp", "rt_bvh.cpp")], check=True)

    def plan(*pairs, env=None):
        e = dict(os.environ)
        e.pop("RT_LIST_BAND", None)
        e.update(env or {})
        out = subprocess.run([exe] + [str(v) for pair in pairs for v in pair], capture_output=True, text=True,
                             check=True, env=e).stdout.split()
        return [(int(out[i]), int(out[i + 1])) for i in range(0, len(out), 2)]

    cap = 512 << 20
    got = plan((1, 1200), (3, 192), (3, 1200), (6, 1200), (32, 1080000), (8, 1080000), (1000, 1 << 20), (3, 1),
               (2, (1 << 32) - 1))
    assert got[0] == (1200, 0)                               # one chunk: one band, no partials
    assert got[1] == (256, 3 * 256 * 72)                     # a 16x12 frame: 54 KiB, not the budget
    assert got[2] == (1280, 3 * 1280 * 72) and got[3] == (1280, 6 * 1280 * 72)
    assert got[4] == (232960, 32 * 232960 * 72) and -(-1080000 // 232960) == 5
    assert got[5] == (931840, 8 * 931840 * 72)
    assert got[7] == (256, 3 * 256 * 72)
    for (band, nbytes), (P, n) in zip(got[1:], ((3, 192), (3, 1200), (6, 1200), (32, 1080000), (8, 1080000),
                                                (1000, 1 << 20), (3, 1), (2, (1 << 32) - 1))):
        assert band % 256 == 0 and band >= 256 and nbytes == band * P * 72 and nbytes <= cap
        assert band <= (n + 255) // 256 * 256
    assert plan((3, 1200), (32, 1080000), (3, 100), env={"RT_LIST_BAND": "300"}) == [
        (512, 3 * 512 * 72), (512, 32 * 512 * 72), (256, 3 * 256 * 72)]
    assert plan((32, 1080000), env={"RT_LIST_BAND": "100000000"}) == [got[4]]


def test_entry_points_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", tipe_rt.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    new = {"rt_accumulate_list_async", "rt_adaptive_select_async", "rt_adaptive_workspace_bytes",
           "rt_adaptive_params_init", "rt_adaptive_async", "rt_resolve_adaptive_async", "rt_render_adaptive"}
    assert new <= syms and new <= set(tipe_rt.EXPORTED_SYMBOLS)
    for name in ("accumulate_list_async", "adaptive_select_async", "adaptive_async", "resolve_adaptive_async",
                 "render_adaptive", "adaptive_params"):
        assert callable(getattr(tipe_rt, name))
