"""rt_adaptive_select_async (rt.h "adaptive sampling", layer 2): the settled
test and the ordered compaction, against the float32 restatement of rt.h's text
in adaptive_support.  d_rounds, d_list and *d_count must equal it exactly, on
synthetic accumulators as vdenoise_support.sums makes them; the workspace
starts as 0xFF bytes, so nothing is read before it is written."""
import ctypes as C
import math

import numpy as np
import pytest

import tipe_rt
from adaptive_support import (Select, blur, check_select, device_select, enqueue_select, measure,
                              sizeof_adaptive_params, threshold)
from tipe_rt import types as T
from vdenoise_support import D, F, sums


def test_restatement_on_a_hand_computed_3x3_case():
    """n = 1, d = (2^-2, 2^-2, 2^-2) at the centre only, every mean colour 1 - 2^-8 (so y + 2^-8 = 1).
    v is 2^-4 at the centre and 0 elsewhere; its blur is 2^-4 times the
    normalised tap: centre (1/4)/1, edge-adjacent (1/8)/(3/4), corner (1/16)/(9/16)."""
    Y = 1.0 - 2.0 ** -8
    A = np.zeros((3, 3, 9))
    B = np.zeros((3, 3, 9))
    A[..., 0:3] = Y
    B[..., 0:3] = Y
    A[1, 1, 0:3] = Y + 0.25
    B[1, 1, 0:3] = Y - 0.25
    v, y = measure(A, B, 1)
    assert (y == F(Y)).all() and v[1, 1] == F(2.0 ** -4) and v.sum() == F(2.0 ** -4)
    vb = blur(v)
    want = np.array([[1 / 9, 1 / 6, 1 / 9], [1 / 6, 1 / 4, 1 / 6], [1 / 9, 1 / 6, 1 / 9]]) * 2.0 ** -4
    assert (vb == (want.astype(F))).all() or np.abs(vb.astype(D) - want).max() < 2.0 ** -28
    assert vb[1, 1] == F(2.0 ** -6) and vb[0, 1] == F(2.0 ** -7) / F(0.75)
    # tolerance t: threshold 4 t^2; t = 2^-4 gives 2^-6: the centre is exactly on it and settles,
    # as do the others; t = 2^-5 gives 2^-8: centre 2^-6, sides 2^-7/0.75 and corners 2^-4/9 all run on
    assert threshold(y, 2.0 ** -4)[0, 0] == F(2.0 ** -6)
    rounds = np.zeros((3, 3), dtype=np.int32)
    assert len(Select(3, 3)(A, B, 1, 2.0 ** -4, 0, None, rounds)) == 0 and (rounds == 1).all()
    assert list(Select(3, 3)(A, B, 1, 2.0 ** -5, 0, None, rounds)) == list(range(9))
    # t^2 = 2^-9 is no square of a float; t = 0.05: threshold 0.01 leaves the centre (0.0156) and the
    # sides (0.0104) running and settles the corners (0.0069)
    assert list(Select(3, 3)(A, B, 1, 0.05, 0, None, rounds)) == [1, 3, 4, 5, 7]
    # a later round touches its active pixels only
    st = Select(3, 3)
    st(A, B, 1, 0.05, 0, None, rounds)
    kept = st(A, A, 2, 0.05, 3, [4, 7], rounds)              # identical halves: v = 0 at 4 and 7
    assert rounds[1, 1] == 4 and rounds[2, 1] == 4 and rounds[0, 0] == 1
    assert st.v[1, 1] == 0 and st.v[2, 1] == 0 and list(kept) == []


def test_struct_size_matches_the_header(tmp_path):
    c_size, py_size = sizeof_adaptive_params(tmp_path)
    assert c_size == py_size == 12
    p = tipe_rt.adaptive_params()
    assert (p.first_half, p.max_rounds, p.tolerance) == (8, 5, 1.0 / 64.0)


def test_workspace_size():
    wsb = tipe_rt.lib().rt_adaptive_workspace_bytes
    assert wsb(0, 5) == 0 and wsb(5, -1) == 0 and wsb(32769, 32768) == 0
    assert wsb(1, 1) > 0 and wsb(1, 1) % 16 == 0
    # the v, y and keep planes, and the loop's list
    assert wsb(1200, 900) >= 1200 * 900 * 4 * 4 and wsb(1200, 900) < 1200 * 900 * 4 * 5
    assert wsb(32768, 32768) > wsb(1200, 900) > wsb(67, 35)


def test_validation_fails_before_any_device_work():
    L = tipe_rt.lib()
    W, H = 8, 6
    fake = 0x10000
    nbytes = L.rt_adaptive_workspace_bytes(W, H)

    def refused(rc):
        assert rc == T.RT_EINVAL, rc
        assert L.rt_last_error()

    def run(W=W, H=H, a=fake, b=fake, n=4, tol=0.1, rnd=0, lst=fake, cnt=fake, rounds=fake, ws=fake, nbytes=nbytes):
        return L.rt_adaptive_select_async(W, H, a, b, n, tol, rnd, lst, cnt, rounds, ws, nbytes, None)

    for kw in (dict(W=0), dict(H=0), dict(W=-3), dict(W=32769, H=32768, nbytes=1 << 62), dict(a=None), dict(b=None),
               dict(lst=None), dict(cnt=None), dict(rounds=None), dict(ws=None), dict(n=0), dict(n=-2), dict(rnd=-1),
               dict(rnd=16), dict(nbytes=nbytes - 1), dict(nbytes=0), dict(ws=fake + 4), dict(ws=fake + 8)):
        refused(run(**kw))
    for tol in (math.nan, math.inf, -math.inf, 0.0, -0.5, float(np.nextafter(F(2.0 ** -12), F(0))),
                float(np.nextafter(F(1.0), F(2.0))), 2.0):
        refused(run(tol=tol))
    # resolve
    frame = T.Frame(fake, fake, fake, fake)

    def res(W=W, H=H, a=fake, b=fake, rounds=fake, fh=4, fr=frame):
        return L.rt_resolve_adaptive_async(W, H, a, b, rounds, fh, None if fr is None else C.byref(fr), None)

    for kw in (dict(W=0), dict(H=-1), dict(a=None), dict(b=None), dict(rounds=None), dict(fh=0), dict(fr=None),
               dict(fr=T.Frame(None, fake, fake, fake))):
        refused(res(**kw))


# ---- on the GPU ------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1, 1), (1, 40), (40, 1), (257, 3), (37, 23)])
def test_round_0_equals_the_restatement(W, H):
    """Every pixel active; a tolerance that settles some pixels and not others
    (asserted on the restatement, except on the single pixel)."""
    A, B = sums(W, H, 3, seed=500 + W)
    kept = check_select(A, B, 3, 0.25, 0)
    if W * H > 1:
        assert 0 < len(kept) < W * H, len(kept)


@pytest.mark.gpu
def test_a_frame_of_many_blocks_reaches_the_scan_across_waves_and_its_carry():
    """600x500 is 1172 block counts: the scan's sums across its 16 waves (more
    than 64 counts) and its running carry into a second step of 1024 counts;
    then a later round on the survivors, whose list spans both steps."""
    W, H = 600, 500
    A, B = sums(W, H, 3, seed=640)
    state = Select(W, H)
    kept = check_select(A, B, 3, 0.25, 0, state=state)
    assert 0 < len(kept) < W * H and kept[-1] >= 1024 * 256      # kept entries behind the scan's first step
    A2, B2 = sums(W, H, 6, seed=641)
    rounds = np.full((H, W), -7, dtype=np.int32)
    # the device call starts from a fresh workspace: give it the same planes by replaying round 0 there
    got0, _, dev = device_select(A, B, 3, 0.25, 0)
    assert (got0 == kept).all()
    state(A, B, 3, 0.25, 0, None, rounds)
    want = state(A2, B2, 6, 0.25, 1, kept, rounds)
    got, got_rounds, _ = device_select(A2, B2, 6, 0.25, 1, kept, ws=dev["ws"], rounds=dev["rounds"])
    assert len(got) == len(want) and (got == want).all() and (got_rounds == rounds).all()
    assert 0 < len(want) < len(kept)


@pytest.mark.gpu
def test_a_later_round_with_a_sparse_list_keeps_the_other_pixels():
    """Round 0, then round 2 on its survivors with new sums: the planes of the
    workspace persist (an inactive neighbour's v is the one of round 0), the
    round counts of inactive pixels stay, and the list shrinks in order."""
    W, H = 67, 35
    A, B = sums(W, H, 2, seed=601)
    state = Select(W, H)
    rounds = np.full((H, W), -7, dtype=np.int32)
    want0 = state(A, B, 2, 0.25, 0, None, rounds)
    got0, got_rounds, dev = device_select(A, B, 2, 0.25, 0)
    assert (got0 == want0).all() and (got_rounds == rounds).all() and 0 < len(want0) < W * H
    A2, B2 = sums(W, H, 4, seed=602)
    want1 = state(A2, B2, 4, 0.25, 2, want0, rounds)
    got1, got_rounds, _ = device_select(A2, B2, 4, 0.25, 2, want0, ws=dev["ws"], rounds=dev["rounds"])
    assert len(got1) == len(want1) and (got1 == want1).all()
    assert (got_rounds == rounds).all() and set(np.unique(rounds)) == {1, 3}
    assert 0 < len(want1) < len(want0)


@pytest.mark.gpu
def test_all_settled_and_none_settled():
    W, H = 37, 23
    A, B = sums(W, H, 3, seed=610)
    assert len(check_select(A, B, 3, 1.0, 0)) == 0                   # vb <= 4 (y + 2^-8) everywhere
    assert len(check_select(A, B, 3, 2.0 ** -12, 0)) == W * H


@pytest.mark.gpu
def test_pixels_exactly_on_the_threshold_settle():
    """Every mean colour is Y = 1 - 2^-8, so y + 2^-8 = 1 and, with tolerance
    2^-3, the right-hand side is 2^-4 in float32.  d = 2^-2 in every channel
    gives v = 2^-4 = vb (a constant plane blurs to itself exactly): on the
    threshold, settled.  One pixel's d is 2^-2 (1 + 2^-10): its v, and the vb of
    its 3x3 neighbourhood, is above; those run on."""
    W, H = 9, 5
    Y, d = 1.0 - 2.0 ** -8, 0.25
    A = np.zeros((H, W, 9))
    B = np.zeros((H, W, 9))
    A[..., 0:3], B[..., 0:3] = Y + d, Y - d
    v, y = measure(A, B, 1)
    assert (blur(v) == threshold(y, 0.125)).all() and (threshold(y, 0.125) == F(2.0 ** -4)).all()
    assert len(check_select(A, B, 1, 0.125, 0)) == 0
    d1 = 0.25 * (1 + 2.0 ** -10)
    A[2, 4, 0:3], B[2, 4, 0:3] = Y + d1, Y - d1
    kept = check_select(A, B, 1, 0.125, 0)
    assert sorted(kept) == sorted(j * W + i for j in (1, 2, 3) for i in (3, 4, 5))


@pytest.mark.gpu
def test_a_nan_sum_runs_on():
    """A NaN compares false: the pixel and the neighbours its v reaches are kept."""
    W, H = 12, 7
    A, B = sums(W, H, 3, seed=620)
    A[3, 5, 1] = np.nan
    kept = set(check_select(A, B, 3, 1.0, 0))
    assert kept == {j * W + i for j in (2, 3, 4) for i in (4, 5, 6)}


@pytest.mark.gpu
def test_call_runs_on_the_callers_stream_behind_other_work():
    """A side stream with a long fill queued in front; one synchronisation at the end."""
    import torch
    st = torch.cuda.Stream()
    W, H = 130, 70
    A, B = sums(W, H, 3, seed=630)
    rounds = np.full((H, W), -7, dtype=np.int32)
    want = Select(W, H)(A, B, 3, 0.25, 0, None, rounds)
    with torch.cuda.stream(st):
        busy = torch.zeros(1 << 26, dtype=torch.float32, device="cuda:0")
        for _ in range(4):
            busy += 1.0
    out = enqueue_select(A, B, 3, 0.25, 0, (), st)
    st.synchronize()
    n = int(out["count"][0])
    assert n == len(want) and (out["list"].cpu().numpy()[:n].astype(np.uint32) == want).all()
    assert (out["rounds"].cpu().numpy() == rounds).all()
    assert float(busy[0]) == 4.0
