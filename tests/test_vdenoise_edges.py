"""The variance-guided denoiser where seeded noise on a few frame sizes does
not reach: frame edges on and around the 64 x 4 tile, the second trip of the
grid-stride kernels, no pass at all, sigmas at both ends of their range, a
frame without variance (L at its floor) with flat patches and a hard edge, and
the rt_vdenoise_async contract of rt.h (caller's stream, private workspace,
optional planes).

Every GPU comparison is bit for bit against the restatement in
vdenoise_support.py, which test_vdenoise.py's CPU tests guard.

Which pass kernel a case runs (tiled for steps 1..16, plain for 32..128):

    case                           passes   tiled steps   plain steps
    63/64/65 x 3/4/5               3        1, 2, 4       -
    1024x683                       2        1, 2          -
    67x35                          0        -             -
    67x35, sigma ends              5        1..16         -
    96x24, identical halves        5        1..16         -
    130x70, caller's stream        6        1..16         32
"""
import numpy as np
import pytest

import tipe_rt
from vdenoise_support import D, DEFAULTS, means, restate, case, enqueue, device_vdenoise, assert_planes, check_case


@pytest.mark.gpu
@pytest.mark.parametrize("H", [3, 4, 5])
@pytest.mark.parametrize("W", [63, 64, 65])
def test_tile_edges(W, H):
    """On, one short of and one past the 64 x 4 tile, steps 1..4."""
    check_case(W, H, (1, 3, 8)[(W + H) % 3], 200 + 10 * W + H, 3)


@pytest.mark.gpu
def test_grid_stride_second_trip():
    """1024 x 683 = 699 392 pixels: above the 2048 x 256 threads of the per-pixel grid-stride kernels."""
    assert 1024 * 683 > 2048 * 256
    check_case(1024, 683, 3, 300, 2)


@pytest.mark.gpu
def test_zero_iterations_resolves_the_mean():
    check_case(67, 35, 8, 301, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("sigmas", [(2.0 ** -8, 2.0 ** -8, 2.0 ** -8), (2.0 ** 8, 2.0 ** 8, 2.0 ** 8),
                                    (2.0 ** -8, 2.0 ** 8, 0.3), (2.0 ** 8, 2.0 ** -8, 2.0 ** 8)])
def test_sigmas_at_both_ends(sigmas):
    check_case(67, 35, 3, 302, 5, sigmas)


def flat_with_an_edge(W=96, H=24, n=8):
    """Identical halves (v = 0 everywhere, so L is its floor 2^-26): flat
    8 x 8 patches of radiance, albedo and normal, and a hard vertical edge in
    the radiance at x = W/2."""
    rng = np.random.default_rng(303)
    grow = lambda X: np.repeat(np.repeat(X, 8, axis=0), 8, axis=1)  # noqa: E731
    S = np.concatenate([grow(rng.integers(0, 5, (H // 8, W // 8, 3)).astype(D)),
                        grow(rng.integers(0, 3, (H // 8, W // 8, 3)) / 2.0),
                        grow(rng.integers(-1, 2, (H // 8, W // 8, 3)).astype(D))], axis=2)
    S[:, W // 2:, :3] += 100.0
    return S * n, n


@pytest.mark.gpu
def test_identical_halves_filter_at_the_variance_floor():
    S, n = flat_with_an_edge()
    want = restate(S, S.copy(), n, **dict(DEFAULTS, iterations=5))
    assert (means(S, S, n)[1] == 0).all()
    mid = S.shape[1] // 2
    edge = want["radiance"][:, mid:, :].min() - want["radiance"][:, :mid, :].max()
    assert edge > 90.0                                   # the floor keeps the edge: nothing bleeds across it
    assert_planes(device_vdenoise(S, S.copy(), n, iterations=5), want)


@pytest.mark.gpu
def test_call_runs_on_the_callers_stream_behind_other_work():
    """A non-default stream with a long fill queued in front; one call with
    every plane, one with canva only; a single synchronisation at the end."""
    import torch
    st = torch.cuda.Stream()
    A, B, want = case(130, 70, 3, 304, 6)
    with torch.cuda.stream(st):
        busy = torch.zeros(1 << 26, dtype=torch.float32, device="cuda:0")
        for _ in range(4):
            busy += 1.0
    full = enqueue(A, B, 3, st, iterations=6)
    only = enqueue(A, B, 3, st, planes=("canva",), iterations=6)
    torch.cuda.synchronize()
    assert_planes(full, want)
    assert_planes(only, want)
    assert set(only) == {"canva", "_keep"} and float(busy[0]) == 4.0


GUARD = 4096


@pytest.mark.gpu
def test_workspace_is_private_exact_and_poisoned():
    """The workspace is exactly rt_vdenoise_workspace_bytes long, 16-byte (not
    32-byte) aligned inside a larger buffer, and holds NaNs before the call:
    the result does not depend on them, the bytes around it stay, and the
    accumulators are read-only."""
    import torch
    A, B, want = case(130, 70, 3, 304, 6)
    nbytes = tipe_rt.lib().rt_vdenoise_workspace_bytes(130, 70)
    lo = GUARD + 16
    outer = torch.full((lo + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda:0")
    ws = outer[lo:lo + nbytes]
    assert ws.data_ptr() % 32 == 16 and ws.numel() == nbytes
    got = enqueue(A, B, 3, torch.cuda.current_stream(), ws=ws, iterations=6)
    torch.cuda.synchronize()
    assert_planes(got, want)
    assert (outer[:lo] == 0xFF).all().item() and (outer[lo + nbytes:] == 0xFF).all().item()
    assert (got["_keep"][0].cpu().numpy() == A).all() and (got["_keep"][1].cpu().numpy() == B).all()
