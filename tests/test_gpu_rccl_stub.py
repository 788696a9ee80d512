"""The RCCL gather of rt_render_gather_async with more than one rank, on one
GPU: the stand-in library of tests/stubs (built by the Makefile's default
target, loaded through RT_RCCL_LIB) does ncclGather with stream copies and
accepts a device list that repeats device 0, so the rank-major staging, the
assemble offsets and the ranks' streams of the G > 1 path run here.  The real
library keeps refusing such a list (test_gpu_multidevice.py).

The library is loaded once per process, so each case is a fresh child process
(rccl_stub_child.py) under its own time limit, one at a time: the wide path
and the packed canva, canva only and all four planes, each bit for bit
against one device.
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tipe-raytracer_amd", "librt_rccl_stub.so")
CHILD = os.path.join(ROOT, "tests", "rccl_stub_child.py")


def test_stub_exports_the_marker_and_rccl_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", STUB], capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"ncclCommInitAll", "ncclCommDestroy", "ncclGather", "ncclGroupStart", "ncclGroupEnd",
            "ncclGetErrorString", "ncclGetVersion", "rt_rccl_stub_marker"} <= syms


@pytest.mark.parametrize("G,W,H,tile_rows", [(2, 7, 9, 2),      # 5 tiles: ranks hold 3 and 2, the last tile one row
                                             (3, 5, 7, 2),      # 4 tiles: rank 0 holds 2, the others 1 and padding
                                             (8, 33, 9, 1)])    # 9 tiles: rank 0 holds 2, the others 1 and padding
def test_rccl_gather_many_ranks_on_one_gpu(G, W, H, tile_rows):
    assert H % (G * tile_rows), "the case is meant to leave padding rows"
    env = dict(os.environ, RT_RCCL_LIB=STUB)
    r = subprocess.run([sys.executable, CHILD, str(G), str(W), str(H), str(tile_rows)], capture_output=True, text=True,
                       timeout=240, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "DONE 4", r.stdout[-2000:]
    ok = [ln for ln in lines if ln.startswith("OK ")]
    assert len(ok) == 4 and sum("packed=1" in ln for ln in ok) == 2
    assert all(("canva 4 B/px" in ln) == ("packed=1" in ln) for ln in ok)
