"""What adaptive sampling's test files share: the float32 restatement of
rt.h's selection pass (the thing rt_adaptive_select_async is specified by), the
schedule of rt_adaptive_async, each pixel's round count and sums by them, the
device drivers and the glass scene.  The references are the parent's
rt_accumulate_async / rt_resolve_async and NumPy, never the new code."""
import ctypes as C

import numpy as np

import helpers
import tipe_rt
from gpu_driver import device_planes
from tipe_rt import scenes
from vdenoise_support import BLUR_G, D, F, lum2, shifted

FLOOR = F(2.0 ** -8)


# ---- rt.h in float32 -----------------------------------------------------------

def measure(A, B, n):
    """The planes v and y of accumulators A, B (H, W, 9) holding n samples each."""
    rap = D(1.0) / D(n)
    mA, mB = (rap * A[..., 0:3]).astype(F), (rap * B[..., 0:3]).astype(F)
    half = F(0.5)
    c, d = half * (mA + mB), half * (mA - mB)
    y = (F(0.25) * c[..., 0] + F(0.5) * c[..., 1]) + F(0.25) * c[..., 2]
    return lum2(d), y


def blur(v):
    """vb: the 3x3 blur of the v plane, taps inside the image only."""
    H, W = v.shape
    bn, bd = np.zeros((H, W), dtype=F), np.zeros((H, W), dtype=F)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            pq = shifted(H, W, dy, dx)
            if pq is None:
                continue
            P, Q = pq
            gg = BLUR_G[dy + 1] * BLUR_G[dx + 1]
            bn[P] = bn[P] + gg * v[Q]
            bd[P] = bd[P] + gg
    return bn / bd


def threshold(y, tolerance):
    """((4.0f * (tolerance*tolerance)) * (y + 0x1p-8f))"""
    t = F(tolerance)
    return (F(4.0) * (t * t)) * (y + FLOOR)


class Select:
    """The state rt_adaptive_select_async keeps between calls (the v and y
    planes, as a 0xFF-filled workspace starts them: NaN) and one call of it."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.v = np.full((H, W), np.nan, dtype=F)
        self.y = np.full((H, W), np.nan, dtype=F)

    def __call__(self, A, B, n, tolerance, rnd, active, rounds):
        """active: ascending pixel indices (ignored when rnd == 0); rounds: (H, W)
        int32, updated in place.  Returns the new list (uint32, ascending)."""
        W, H = self.W, self.H
        act = np.ones(W * H, dtype=bool)
        if rnd != 0:
            act[:] = False
            act[np.asarray(active, dtype=np.int64)] = True
        act = act.reshape(H, W)
        v, y = measure(A, B, n)
        self.v[act], self.y[act] = v[act], y[act]
        with np.errstate(invalid="ignore"):
            vb = blur(self.v)
            settled = vb <= threshold(self.y, tolerance)
        assert vb.dtype == F and threshold(self.y, tolerance).dtype == F
        rounds[act] = rnd + 1
        return np.flatnonzero(act & ~settled).astype(np.uint32)


def schedule(first_half, max_rounds):
    """[(o_r, b_r, n_r)]: round r adds [o_r, o_r + b_r) to A and the next b_r
    samples to B; n_r samples per accumulator afterwards."""
    out = []
    for r in range(max_rounds):
        n = first_half << r
        out.append((0, n, n) if r == 0 else (n, n // 2, n))
    return out


# ---- rt_adaptive_async's reference, pixel by pixel -----------------------------------

def reference_rounds(per_round, first_half, tolerance):
    """Each pixel's round count by the restatement: (H, W) int32."""
    R = len(per_round)
    H, W = per_round[0][0].shape[:2]
    state = Select(W, H)
    rounds = np.zeros((H, W), dtype=np.int32)
    active = None
    for r in range(R - 1):
        A, B = per_round[r]                      # an active pixel holds its (r + 1)-round sums
        active = state(A, B, first_half << r, tolerance, r, active, rounds)
    if R == 1:
        rounds[:] = 1
    else:
        rounds.reshape(-1)[active.astype(np.int64)] = R
    return rounds


def pick(per_round, rounds, which):
    """Pixel p from the accumulators of its own round count."""
    out = np.empty_like(per_round[0][which])
    for k in range(1, len(per_round) + 1):
        out[rounds == k] = per_round[k - 1][which][rounds == k]
    return out


# ---- device drivers -------------------------------------------------------------

def sentinel(W, H):
    """A per-pixel pattern no sample sum gives: -(1000 + pixel + slot / 16)."""
    px = np.arange(W * H, dtype=D).reshape(H, W, 1)
    return -(1000.0 + px + np.arange(9, dtype=D) / 16.0)


def u64(x):
    return np.ascontiguousarray(x).view(np.uint64)


def device_list(entries, room):
    """(d_list of `room` entries, d_count) int32 tensors on cuda:0; beyond the
    entries the list holds an index no frame has."""
    import torch
    host = np.full(room, 0x7fffffff, dtype=np.int32)
    host[:len(entries)] = np.asarray(entries, dtype=np.int64)
    return torch.from_numpy(host).to("cuda:0"), torch.tensor([len(entries), -1, -1, -1], dtype=torch.int32,
                                                             device="cuda:0")


def accumulate_list(ds, p, offsets, start, entries, count=None, cap=None):
    """rt_accumulate_list_async at each offset into a copy of `start` (H, W, 9): the host array afterwards."""
    import torch
    W, H = p.largeur_image, p.hauteur_image
    st = torch.cuda.current_stream().cuda_stream
    sums = torch.from_numpy(np.ascontiguousarray(start)).to("cuda:0")
    d_list, d_count = device_list(entries, W * H)
    if count is not None:
        d_count[0] = count
    for off in offsets:
        tipe_rt.accumulate_list_async(ds, p, off, d_list.data_ptr(), d_count.data_ptr(),
                                      cap if cap is not None else W * H, sums.data_ptr(), st)
    torch.cuda.synchronize()
    return sums.cpu().numpy()


def accumulate_dense(ds, p, offsets, start):
    """The reference: rt_accumulate_async over the whole frame at each offset into a copy of `start`."""
    import torch
    H = p.hauteur_image
    st = torch.cuda.current_stream().cuda_stream
    sums = torch.from_numpy(np.ascontiguousarray(start)).to("cuda:0")
    for off in offsets:
        tipe_rt.accumulate_async(ds, p, off, tipe_rt.band_tiling(0, H - 1), sums.data_ptr(), st)
    torch.cuda.synchronize()
    return sums.cpu().numpy()


def enqueue_select(A, B, n, tolerance, rnd, entries, stream, ws=None, rounds=None):
    """Uploads and calls rt_adaptive_select_async, all on `stream`, and waits
    for nothing.  ws: a uint8 device tensor (default: a fresh one of exactly the
    required size filled with 0xFF bytes).  Returns the device tensors."""
    import torch
    H, W = A.shape[:2]
    with torch.cuda.stream(stream):
        dA, dB = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (A, B))
        nbytes = tipe_rt.lib().rt_adaptive_workspace_bytes(W, H)
        if ws is None:
            ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda:0")
        if rounds is None:
            rounds = torch.full((H, W), -7, dtype=torch.int32, device="cuda:0")
        d_list, d_count = device_list(entries, W * H)
    tipe_rt.adaptive_select_async(W, H, dA.data_ptr(), dB.data_ptr(), n, tolerance, rnd, d_list.data_ptr(),
                                  d_count.data_ptr(), rounds.data_ptr(), ws.data_ptr(), nbytes,
                                  stream=stream.cuda_stream)
    return dict(list=d_list, count=d_count, rounds=rounds, ws=ws, _keep=(dA, dB))


def device_select(A, B, n, tolerance, rnd, entries=(), **kw):
    """One call on torch's current stream: (list, rounds, out) with the host list and round counts."""
    import torch
    out = enqueue_select(A, B, n, tolerance, rnd, entries, torch.cuda.current_stream(), **kw)
    torch.cuda.synchronize()
    count = int(out["count"][0])
    return out["list"].cpu().numpy()[:count].astype(np.uint32), out["rounds"].cpu().numpy(), out


def check_select(A, B, n, tolerance, rnd, entries=(), state=None):
    """The device against the restatement: list, count and round counts."""
    H, W = A.shape[:2]
    state = state if state is not None else Select(W, H)
    want_rounds = np.full((H, W), -7, dtype=np.int32)
    want = state(A, B, n, tolerance, rnd, entries, want_rounds)
    got, got_rounds, _ = device_select(A, B, n, tolerance, rnd, entries)
    assert len(got) == len(want), "count %d, restatement %d" % (len(got), len(want))
    assert (got == want).all(), "list differs first at entry %d" % int(np.argmax(got != want))
    assert (got_rounds == want_rounds).all(), "d_rounds differs at %d pixels" % int((got_rounds != want_rounds).sum())
    return want


def sizeof_adaptive_params(tmp_path):
    """sizeof(rt_adaptive_params) from a compiled program."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "rt/rt.h"\nint main(void) { printf("%zu\\n", sizeof(rt_adaptive_params)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), "-o", str(exe), str(src)], check=True)
    return int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout), C.sizeof(
        tipe_rt.types.AdaptiveParams)


def device_adaptive(ds, p, ap, frame=True):
    """rt_adaptive_async on torch's current stream: (A, B, rounds, planes) as host arrays."""
    import torch
    W, H = p.largeur_image, p.hauteur_image
    st = torch.cuda.current_stream().cuda_stream
    acc = torch.full((2, H, W, 9), float("nan"), dtype=torch.float64, device="cuda:0")    # zeroed by the call
    rounds = torch.full((H, W), -7, dtype=torch.int32, device="cuda:0")
    nbytes = tipe_rt.lib().rt_adaptive_workspace_bytes(W, H)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda:0")
    planes = device_planes(H, W)
    tipe_rt.adaptive_async(ds, p, ap, acc[0].data_ptr(), acc[1].data_ptr(), rounds.data_ptr(), ws.data_ptr(), nbytes,
                           *([t.data_ptr() for t in planes] if frame else []), stream=st)
    torch.cuda.synchronize()
    host = acc.cpu().numpy()
    return host[0], host[1], rounds.cpu().numpy(), [t.cpu().numpy() for t in planes]


GLASS = scenes.material((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 0.0, 0.0, 0.3, 1.5)


def glass_cornell():
    return helpers.cornell(extra=[((-0.3, -0.55, -1.9), 0.4, GLASS)])
