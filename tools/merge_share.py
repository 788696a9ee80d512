"""How often the sphere candidate pass's flagged pairs ran one root tail
(rt_spheres.h spheres_closest), per wave-cast of a render_kernel_q frame.

    bash tools/build_variants.sh merge "-DRT_DIAG_MERGE=1"
    RT_HIP_LIB=tools/variants/merge.so python tools/merge_share.py [c2,c3] [spp]

The diagnostic build counts, per wave, the flagged pairs that took the merged
form and those that fell back to two tails, and writes both into the wave's
RT_QUEUE_TRACE record (in place of rounds and tasks), and the same two counts
of the forward pairs (in place of the two clocks): the four counters are
rt_spheres.h's DiagMerge slots, and the record's words 2, 3, 0 and 1 are
DM_FLAGGED_ONE, DM_FLAGGED_TWO, DM_FORWARD_ONE and DM_FORWARD_TWO.  The pairs
are the host's (rt_scene_prep.cpp pair_candidates).  One JSON line per scene."""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tipe-raytracer_amd"))
import torch  # noqa: E402
import tipe_rt  # noqa: E402
from tipe_rt import scenes  # noqa: E402


def run(kind, spp):
    fd, path = tempfile.mkstemp(prefix="merge_share_%s_" % kind, suffix=".bin")
    os.close(fd)
    sph = scenes.cornell_spheres()
    sc = tipe_rt.make_scene(sph) if kind == "c2" else tipe_rt.make_scene(sph, *scenes.pyramid_mesh())
    spec = scenes.README_CAMERA
    cam = tipe_rt.init_camera(**{k: spec[k] for k in ("origin", "target", "up", "vfov", "ratio")})
    p = tipe_rt.make_params(1200, 900, spp, 6, cam, focus=3.0, seed=1010, chunks=32)
    ds = tipe_rt.DeviceScene(sc, 0)
    out = torch.empty((3, 900, 1200, 3), dtype=torch.float64, device="cuda:0")
    os.environ["RT_QUEUE_TRACE"] = path
    tipe_rt.render_async(ds, p, tipe_rt.band_tiling(0, 899), out[0].data_ptr(), out[1].data_ptr(),
                         out[2].data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del os.environ["RT_QUEUE_TRACE"]
    d = np.fromfile(path, dtype=np.uint64).reshape(-1, 4)
    w = d[::64].astype(np.float64)               # the counts are wave-uniform: lane 0 of each wave
    one, two = float(w[:, 2].sum()), float(w[:, 3].sum())
    f_one, f_two = float(w[:, 0].sum()), float(w[:, 1].sum())
    os.remove(path)
    return {"scene": kind, "spp": spp, "kernel": tipe_rt.last_render_kernel(), "flagged_pair_casts": one + two,
            "one_tail": one, "two_tails": two, "merged_share": round(one / max(one + two, 1.0), 4),
            "forward_pair_casts": f_one + f_two, "forward_one_tail": f_one, "forward_two_tails": f_two,
            "forward_merged_share": round(f_one / max(f_one + f_two, 1.0), 4)}


if __name__ == "__main__":
    kinds = (sys.argv[1] if len(sys.argv) > 1 else "c2,c3").split(",")
    spp = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    for k in kinds:
        print(json.dumps(run(k, spp)), flush=True)
