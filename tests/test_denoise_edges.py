"""The built-in denoiser where uniform noise on two frame sizes does not reach:
every instantiation of the pass kernels, frame edges on and around the 64 x 4
tile, the second trip of the grid-stride kernels, exact ties and truncation
edges, binary32 subnormals, and the rt_denoise_async / rt_denoise_host
contract of rt.h (caller's stream, private workspace, threads).

Every GPU comparison is bit for bit against the restatement in
denoise_support.py, which test_denoise_atrous.py's CPU tests guard.

Which pass kernel a case runs (launch_pass: tiled for steps 1..16, plain for
32..128, <ALB, NRM> from the planes given):

    case                                     tiled <A,N>   plain <A,N>
    64x4, 65x5, 128x33, 63x64     5 it.      <1,1>         -
    1x97, 97x1                    7 it.      <1,1>         <1,1>  steps 32, 64
    260x9                         8 it.      <1,1>         <1,1>  steps 32..128
    130x70, normal only           6 it.      <0,1>         <0,1>  step 32
    130x70, albedo only           6 it.      <1,0>         <1,0>  step 32
    130x70, no guide plane        6 it.      <0,0>         <0,0>  step 32
    1024x683                      1 it.      <1,1>         -
    patchwork 128x128         2, 5 it.       <1,1>         -
    subnormal, negative 67x35     3 it.      <1,1>         -
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import helpers
import tipe_rt
from gpu_driver import device_planes
from denoise_support import F, DEFAULTS, restate, params_of, frames, reference_pack

BIG = (1024, 683)          # 2 098 176 floats: just above the 8192 x 256 threads of the grid-stride kernels


# ---- frames ----------------------------------------------------------------------

def patchwork(P=8, G=16, seed=0):
    """G x G flat patches of P x P pixels: canva a permutation of the levels
    0..255 (grey), albedo from {0, 1/3, 2/3, 1} x 1.3 and normals from
    {-1, 0, 1} per channel.  Exact ties (d2 == 0), zero normals, saturated 0
    and 255 and albedo above 1, as a rendered frame has them."""
    assert G * G <= 256
    rng = np.random.default_rng(seed)
    grow = lambda X: np.repeat(np.repeat(X, P, axis=0), P, axis=1)  # noqa: E731
    level = rng.permutation(256)[:G * G].reshape(G, G, 1).astype(np.float64)
    canva = grow(np.repeat(level, 3, axis=2))
    albedo = grow(rng.integers(0, 4, (G, G, 3)) / 3.0 * 1.3)
    normal = grow(rng.integers(-1, 2, (G, G, 3)).astype(np.float64))
    return canva, albedo, normal


def scaled(fr, factor):
    """The frame with its canva plane multiplied by factor."""
    return fr[0] * factor, fr[1], fr[2]


@functools.lru_cache(maxsize=None)
def noise(W, H, seed):
    return frames(H=H, W=W, seed=seed)


def dropped(fr, use_albedo=True, use_normal=True):
    return fr[0], fr[1] if use_albedo else None, fr[2] if use_normal else None


@functools.lru_cache(maxsize=None)
def noise_case(W, H, seed, iterations, use_albedo=True, use_normal=True):
    """(frame, restated c, restated canva) of a noise frame at the default sigmas; shared, never written."""
    fr = dropped(noise(W, H, seed), use_albedo, use_normal)
    return (fr,) + restate(*fr, **dict(DEFAULTS, iterations=iterations))


SMALL = (67, 35, 51, 5)    # W, H, seed, iterations: the two frames of the contract tests
LARGE = (130, 70, 52, 6)


# ---- device plumbing -------------------------------------------------------------

def ws_bytes(W, H):
    return tipe_rt.lib().rt_denoise_workspace_bytes(W, H)


def enqueue(fr, stream, ws=None, color3=True, **kw):
    """Uploads the frame and calls rt_denoise_async, all on `stream`, and waits
    for nothing.  ws: a uint8 device tensor (default: a fresh one of exactly the
    required size).  Returns (color3_out or None, [canva, albedo, normal]) on the device."""
    import torch
    H, W = fr[0].shape[:2]
    with torch.cuda.stream(stream):
        t = [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in fr]
        if ws is None:
            ws = torch.empty(ws_bytes(W, H), dtype=torch.uint8, device="cuda:0")
        c3 = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0") if color3 else None
    tipe_rt.denoise_async(W, H, *[None if x is None else x.data_ptr() for x in t], params_of(**kw), ws.data_ptr(),
                          ws.numel(), None if c3 is None else c3.data_ptr(), stream.cuda_stream)
    return c3, t, ws


def assert_result(got, fr, want_c, want_canva):
    """got = enqueue's tensors after a synchronisation."""
    c3, t = got[0], got[1]
    if c3 is not None:
        c = c3.cpu().numpy()
        bad = c.view(np.uint32) != want_c.view(np.uint32)
        assert not bad.any(), "%d of %d floats differ, first at (y, x, ch) %s" % (bad.sum(), bad.size,
                                                                                   tuple(np.argwhere(bad)[0]))
    assert (t[0].cpu().numpy() == want_canva).all()
    for plane, x in zip(t[1:], fr[1:]):             # the guide planes are read-only
        assert plane is None or (plane.cpu().numpy() == x).all()


def check(fr, **kw):
    """One call on torch's current stream against the restatement; returns (c, canva) restated."""
    import torch
    want = restate(*fr, **dict(DEFAULTS, **kw))
    got = enqueue(fr, torch.cuda.current_stream(), **kw)
    torch.cuda.synchronize()
    assert_result(got, fr, *want)
    return want


# ---- shapes and instantiations ---------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("W,H,iterations", [(64, 4, 5), (65, 5, 5), (128, 33, 5), (63, 64, 5),   # the tile: on, past, short
                                            (1, 97, 7), (97, 1, 7),      # only the centre dx / dy tap exists
                                            (260, 9, 8)])                # step 128: x +- 256 is inside
def test_tile_edges_and_thin_frames(W, H, iterations):
    check(noise(W, H, 60 + iterations), iterations=iterations)


@pytest.mark.gpu
@pytest.mark.parametrize("use_albedo,use_normal", [(False, True), (True, False), (False, False)])
def test_null_planes_through_both_pass_kernels(use_albedo, use_normal):
    """Steps 1..32: the tiled kernel up to its largest tile (albedo at LDS plane
    3 when there is no normal) and the plain kernel, without a guide plane."""
    import torch
    fr, want_c, want_canva = noise_case(*LARGE, use_albedo=use_albedo, use_normal=use_normal)
    got = enqueue(fr, torch.cuda.current_stream(), iterations=LARGE[3])
    torch.cuda.synchronize()
    assert_result(got, fr, want_c, want_canva)


@pytest.mark.gpu
def test_grid_stride_second_trip_of_prepare_and_finish():
    assert BIG[0] * BIG[1] * 3 > 8192 * 256
    check(noise(*BIG, 70), iterations=1)


@pytest.mark.gpu
def test_grid_stride_second_trip_of_pack():
    import torch
    W, H = BIG
    fr = noise(W, H, 70)
    planes = [torch.from_numpy(x).to("cuda:0") for x in fr]
    outs = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    frame = tipe_rt.types.Frame(*[t.data_ptr() for t in planes], None)
    tipe_rt.check(tipe_rt.lib().rt_denoise_pack_async(W, H, C.byref(frame), *[o.data_ptr() for o in outs],
                                                      torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for g, w in zip(outs, reference_pack(*fr)):
        assert (g.cpu().numpy().view(np.uint32) == w.view(np.uint32)).all()


# ---- ties, truncation edges, float mode -----------------------------------------

def one_level_share(fr, want_canva):
    return float((np.abs(want_canva - fr[0]) == 1.0).mean())


def test_patchwork_sits_on_the_truncation_edge():
    """What makes patchwork worth filtering (restatement alone, no GPU): at 2
    iterations at least a quarter of the outputs are the input moved by exactly
    one level, i.e. c * 255 lies next to an integer."""
    fr = patchwork(seed=80)
    assert sorted(np.unique(fr[0])) == list(range(256)) and (fr[0][..., 0] == fr[0][..., 2]).all()
    assert fr[1].max() == 1.3 and fr[1].min() == 0.0 and (fr[2] == 0).all(-1).any()
    assert (fr[0][:8, :8] == fr[0][0, 0]).all() and (fr[1][8:16, -8:] == fr[1][8, -1]).all()
    assert one_level_share(fr, restate(*fr, **dict(DEFAULTS, iterations=2))[1]) >= 0.25


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(iterations=2), dict(iterations=5), dict(iterations=2, sigma_color=2.0 ** -8)],
                         ids=["2-iterations", "5-iterations", "sigma_color-2^-8"])
def test_patchwork_ties_and_truncation_edges(kw):
    fr = patchwork(seed=80)
    _, want_canva = check(fr, **kw)
    if kw == dict(iterations=2):
        assert one_level_share(fr, want_canva) >= 0.25


@pytest.mark.gpu
def test_subnormal_colours_are_kept():
    """Every c is a binary32 subnormal, in and out: a kernel that flushes them returns zeros."""
    fr = scaled(noise(67, 35, 81), 2.0 ** -130)
    want_c, want_canva = restate(*fr, **dict(DEFAULTS, iterations=3))
    tiny = float(np.finfo(F).tiny)
    assert ((want_c != 0) & (np.abs(want_c) < tiny)).all() and (want_canva == 0).all()
    check(fr, iterations=3)


@pytest.mark.gpu
def test_negative_colours_truncate_toward_zero():
    fr = scaled(noise(67, 35, 82), -2.0 ** 20)
    want_c, want_canva = check(fr, iterations=3)
    assert want_c.min() * 255.0 > -2.0 ** 31 and (want_canva <= 0).all()      # (int) is defined
    assert (want_canva != np.floor(want_c * F(255.0))).any()                  # and is not floor


# ---- the rt_denoise_async contract -----------------------------------------------

GUARD = 4096


@pytest.mark.gpu
@pytest.mark.parametrize("case,color3", [(SMALL, True), (LARGE, True), (SMALL, False)],
                         ids=["67x35", "130x70", "67x35-no-color3"])
def test_workspace_is_private_exact_and_poisoned(case, color3):
    """The workspace is exactly rt_denoise_workspace_bytes long, 16-byte (not
    32-byte) aligned inside a larger buffer, and holds NaNs before the call:
    the result does not depend on them and the bytes around it stay."""
    import torch
    fr, want_c, want_canva = noise_case(*case)
    W, H = case[:2]
    n = ws_bytes(W, H)
    lo = GUARD + 16
    outer = torch.full((lo + n + GUARD,), 0xFF, dtype=torch.uint8, device="cuda:0")
    ws = outer[lo:lo + n]
    assert ws.data_ptr() % 32 == 16 and ws.numel() == n
    got = enqueue(fr, torch.cuda.current_stream(), ws=ws, color3=color3, iterations=case[3])
    torch.cuda.synchronize()
    assert_result(got, fr, want_c, want_canva)
    assert (outer[:lo] == 0xFF).all().item() and (outer[lo + n:] == 0xFF).all().item()


@pytest.mark.gpu
def test_calls_run_on_the_callers_streams():
    """Two streams, a frame size and a workspace each, calls enqueued
    alternately, every round on a fresh copy of its input; one
    synchronisation at the very end."""
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    cases = [SMALL, LARGE]
    spaces, got = [], [[], []]
    for st, case in zip(streams, cases):
        with torch.cuda.stream(st):
            spaces.append(torch.empty(ws_bytes(*case[:2]), dtype=torch.uint8, device="cuda:0"))
    for _ in range(3):
        for k in (0, 1):
            got[k].append(enqueue(noise_case(*cases[k])[0], streams[k], ws=spaces[k], iterations=cases[k][3]))
    torch.cuda.synchronize()
    for k in (0, 1):
        for g in got[k]:
            assert_result(g, *noise_case(*cases[k]))


@pytest.mark.gpu
def test_one_workspace_serves_frames_of_different_sizes():
    """large, small, large on one stream and one workspace, nothing waited for in between."""
    import torch
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ws = torch.empty(ws_bytes(*LARGE[:2]), dtype=torch.uint8, device="cuda:0")
    order = [LARGE, SMALL, LARGE]
    got = [enqueue(noise_case(*case)[0], st, ws=ws, iterations=case[3]) for case in order]
    torch.cuda.synchronize()
    for g, case in zip(got, order):
        assert_result(g, *noise_case(*case))


@pytest.mark.gpu
def test_render_then_denoise_stays_on_the_device():
    import torch
    bundle = helpers.cornell()
    W, H = 24, 18
    p = helpers.params(W, H, 2, 4)
    plain = tipe_rt.render_rows(bundle.scene, p)
    want = restate(*plain, **DEFAULTS)[1]
    assert (want != plain[0]).any()
    ds = tipe_rt.DeviceScene(bundle.scene, 0)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        planes = device_planes(H, W, n=3)
        ws = torch.empty(ws_bytes(W, H), dtype=torch.uint8, device="cuda:0")
    tipe_rt.render_async(ds, p, tipe_rt.band_tiling(0, H - 1), *[t.data_ptr() for t in planes], stream=st.cuda_stream)
    tipe_rt.denoise_async(W, H, *[t.data_ptr() for t in planes], params_of(), ws.data_ptr(), ws.numel(), None,
                          st.cuda_stream)
    torch.cuda.synchronize()
    ds.close()
    canva, albedo, normal = [t.cpu().numpy() for t in planes]
    assert (canva == want).all()
    assert (albedo == plain[1]).all() and (normal == plain[2]).all()


# ---- host path and hook ------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("use_albedo,use_normal", [(True, False), (False, True)], ids=["albedo-only", "normal-only"])
def test_host_path_with_one_guide_plane(use_albedo, use_normal):
    fr = dropped(noise(67, 35, 90), use_albedo, use_normal)
    before = [None if x is None else x.copy() for x in fr]
    assert (tipe_rt.denoise(*fr) == restate(*fr, **DEFAULTS)[1]).all()
    assert all(x is None or (x == b).all() for x, b in zip(fr, before))


@pytest.mark.gpu
def test_host_path_from_four_threads():
    """rt_denoise_host shares the drop-ins' stream pool, which serves
    pthreads: four threads (ctypes releases the GIL), a frame size each,
    three calls each."""
    sizes = [(9, 7), (33, 20), (67, 35), (130, 70)]
    its = (2, 4, 6)
    work = [(noise(W, H, 91 + k), [x.copy() for x in noise(W, H, 91 + k)]) for k, (W, H) in enumerate(sizes)]
    results, errors = [[] for _ in sizes], []

    def run(k):
        try:
            for it in its:
                results[k].append(tipe_rt.denoise(*work[k][0], params=params_of(iterations=it)))
        except Exception as e:          # reported after the join
            errors.append((k, e))

    tipe_rt.lib()                       # loaded before the threads start
    threads = [threading.Thread(target=run, args=(k,)) for k in range(len(sizes))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k, (fr, before) in enumerate(work):
        assert len(results[k]) == len(its)
        for it, got in zip(its, results[k]):
            assert (got == restate(*fr, **dict(DEFAULTS, iterations=it))[1]).all(), (sizes[k], it)
        assert all((x == b).all() for x, b in zip(fr, before))


@pytest.mark.gpu
@pytest.mark.parametrize("missing", ["albedo", "normal"])
def test_hook_needs_both_guide_planes(missing):
    """rt_render_rows runs the hook only on a frame with albedo and normal: denoiser()'s arguments."""
    bundle = helpers.cornell()
    p = helpers.params(24, 18, 2, 4)
    plain = tipe_rt.render_rows(bundle.scene, p)
    assert (restate(*plain, **DEFAULTS)[1] != plain[0]).any()
    try:
        tipe_rt.set_denoise_atrous(True)
        got = tipe_rt.render_rows(bundle.scene, p, **{missing: False})
    finally:
        tipe_rt.set_denoise_atrous(False)
    assert not tipe_rt.lib().rt_get_denoise_hook()
    assert (got[0] == plain[0]).all()
    assert got[1 if missing == "albedo" else 2] is None
