"""Child process of test_gpu_rccl_stub.py: rt_render_gather_async over the
RCCL path with G ranks on device 0, the stand-in library of tests/stubs in
RCCL's place (RT_RCCL_LIB, read once per process: hence a process of its own).

    python rccl_stub_child.py G W H tile_rows

Flag off and on, canva only and all four planes, each bit for bit against one
device's rt_render_async frame.  Prints one "OK ..." line per case and
"DONE n"; any mismatch ends the process with its message.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tipe-raytracer_amd")]

import torch  # noqa: E402,F401  (before librt_hip.so: one HIP runtime in the process)

import helpers  # noqa: E402
import tipe_rt  # noqa: E402
from gpu_driver import device_planes, gpu_render  # noqa: E402
from packed_canva_support import same_bits  # noqa: E402
from tipe_rt.types import RT_GATHER_PACKED_CANVA, RT_GATHER_RCCL  # noqa: E402


def main():
    G, W, H, tile_rows = (int(a) for a in sys.argv[1:5])
    stub = os.environ["RT_RCCL_LIB"]
    lib = tipe_rt.lib()
    bundle = helpers.cornell()
    p = helpers.params(W, H, 4, 4, chunks=2)
    ref = gpu_render(bundle, p)
    tipe_rt.check(lib.rt_init(G, (C.c_int * G)(*([0] * G))))
    st = torch.cuda.current_stream().cuda_stream
    done = 0
    for nplanes in (1, 4):
        results = {}
        for flag in (0, RT_GATHER_PACKED_CANVA):
            p.gather = RT_GATHER_RCCL | flag
            for rep in range(2):                   # the second call reuses communicators, streams and pool memory
                planes = device_planes(H, W, fill=-3.0)
                ptrs = [planes[k].data_ptr() if k < nplanes else None for k in range(4)]
                tipe_rt.render_gather_async(bundle.scene, p, tile_rows, *ptrs, stream=st)
                torch.cuda.synchronize()
                got = [t.cpu().numpy() for t in planes]
                tr = tipe_rt.last_gather_transport()
                assert tr.startswith("rccl: ncclGather") and stub in tr and "%d ranks" % G in tr, tr
                assert tr.endswith(", canva 4 B/px") == bool(flag), tr
                for k in range(4):
                    if k < nplanes:
                        same_bits(got[k], ref[k])
                    else:
                        assert (got[k] == -3.0).all(), k
            results[flag] = got
            print("OK G=%d %dx%d tile_rows=%d planes=%d packed=%d: %s" % (G, W, H, tile_rows, nplanes, bool(flag), tr))
            done += 1
        for k in range(nplanes):                  # the other planes equal the flag-off result
            same_bits(results[RT_GATHER_PACKED_CANVA][k], results[0][k])
    lib.rt_shutdown()
    print("DONE %d" % done)


if __name__ == "__main__":
    main()
