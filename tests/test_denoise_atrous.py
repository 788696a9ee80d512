"""The built-in denoiser (rt.h "built-in denoiser"): an edge-avoiding a-trous
wavelet filter of the library's own -- not OIDN -- behind the denoise hook.

rt.h specifies the filter operation by operation in IEEE binary32, so the
NumPy float32 restatement in tests/denoise_support.py (written from that text,
not from the kernel) must equal the GPU bit for bit.  Parameter defaults, the workspace size and
argument validation run without a GPU; everything that filters is gpu-marked."""
import ctypes as C
import math

import numpy as np
import pytest

import helpers
import tipe_rt
from tipe_rt import types as T
from denoise_support import F, TAP_H, DEFAULTS, restate, params_of, device_denoise, frames


def restate_scalar(canva, albedo, normal, iterations=4, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.25):
    """rt.h's filter once more, one pixel and one tap at a time on np.float32
    scalars in the header's tap order: no slicing, so it shares nothing with
    restate's P/Q bookkeeping.  Returns what restate returns."""
    H, W = canva.shape[:2]
    one = F(1.0)

    def scalars(X, div=None):
        return [[[F(X[j, i, ch]) if div is None else F(X[j, i, ch]) / div for ch in range(3)] for i in range(W)]
                for j in range(H)]

    def d2(X, qy, qx, py, px):
        D = [X[qy][qx][ch] - X[py][px][ch] for ch in range(3)]
        return (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]

    c = scalars(canva, F(255.0))
    a = None if albedo is None else scalars(albedo)
    n = None if normal is None else scalars(normal)
    h = [F(1.0) / F(16.0), F(1.0) / F(4.0), F(3.0) / F(8.0), F(1.0) / F(4.0), F(1.0) / F(16.0)]
    sn, sa = F(sigma_normal), F(sigma_albedo)
    for i in range(iterations):
        s = 1 << i
        sc = F(sigma_color) * F(2.0 ** -i)
        out = [[None] * W for _ in range(H)]
        for y in range(H):
            for x in range(W):
                acc, ws = [F(0.0), F(0.0), F(0.0)], F(0.0)
                for dy in range(-2, 3):
                    qy = y + s * dy
                    if qy < 0 or qy >= H:
                        continue
                    for dx in range(-2, 3):
                        qx = x + s * dx
                        if qx < 0 or qx >= W:
                            continue
                        w = (h[dy + 2] * h[dx + 2]) * (one / (one + d2(c, qy, qx, y, x) / (sc * sc)))
                        if n is not None:
                            w = w * (one / (one + d2(n, qy, qx, y, x) / (sn * sn)))
                        if a is not None:
                            w = w * (one / (one + d2(a, qy, qx, y, x) / (sa * sa)))
                        assert type(w) is F
                        acc = [acc[ch] + w * c[qy][qx][ch] for ch in range(3)]
                        ws = ws + w
                out[y][x] = [acc[ch] / ws for ch in range(3)]
        c = out
    c = np.array(c, dtype=F)
    return c, np.trunc(c * F(255.0)).astype(np.int64).astype(np.float64)


def evaluate_f64(canva, albedo, normal, iterations=4, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.25):
    """rt.h's formulas in float64 on the binary32 inputs (c = (float)canva / 255,
    the guide planes and sigmas rounded to float32 first): the filtered colour
    without the binary32 roundings of the filter itself.  Taps outside the
    image are masked in zero-padded planes, not sliced away."""
    D = np.float64
    H, W = canva.shape[:2]
    c = canva.astype(F).astype(D) / 255.0
    guides = [(x.astype(F).astype(D), D(F(sig)) ** 2) for x, sig in ((normal, sigma_normal), (albedo, sigma_albedo))
              if x is not None]
    inside = np.ones((H, W), dtype=D)
    for i in range(iterations):
        s = 1 << i
        sc2 = (D(F(sigma_color)) * 2.0 ** -i) ** 2
        m = 2 * s

        def pad(X):
            return np.pad(X, [(m, m), (m, m)] + [(0, 0)] * (X.ndim - 2))

        cp, gp, ip = pad(c), [pad(g) for g, _ in guides], pad(inside)
        acc, ws = np.zeros((H, W, 3)), np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                at = (slice(m + s * dy, m + s * dy + H), slice(m + s * dx, m + s * dx + W))
                w = float(TAP_H[dy + 2]) * float(TAP_H[dx + 2]) / (1.0 + ((cp[at] - c) ** 2).sum(-1) / sc2)
                for (g, sig2), p in zip(guides, gp):
                    w = w / (1.0 + ((p[at] - g) ** 2).sum(-1) / sig2)
                w = w * ip[at]
                acc += w[..., None] * cp[at]
                ws += w
        c = acc / ws[..., None]
    return c


def check_bit_exact(W, H, seed, use_albedo=True, use_normal=True, **kw):
    canva, albedo, normal = frames(H=H, W=W, seed=seed)
    albedo = albedo if use_albedo else None
    normal = normal if use_normal else None
    want_c, want_canva = restate(canva, albedo, normal, **dict(DEFAULTS, **kw))
    got_c, got_canva, got_a, got_n = device_denoise(canva, albedo, normal, **kw)
    assert (got_c.view(np.uint32) == want_c.view(np.uint32)).all(), \
        "%d of %d floats differ" % ((got_c.view(np.uint32) != want_c.view(np.uint32)).sum(), want_c.size)
    assert (got_canva == want_canva).all()
    if use_albedo:
        assert (got_a == albedo).all()
    if use_normal:
        assert (got_n == normal).all()


# ---- without a GPU ------------------------------------------------------------

def test_params_init_defaults():
    p = T.DenoiseParams(99, 9.0, 9.0, 9.0)
    tipe_rt.lib().rt_denoise_params_init(C.byref(p))
    assert (p.iterations, p.sigma_color, p.sigma_normal, p.sigma_albedo) == (4, 1.0, 0.5, 0.25)
    assert tipe_rt.lib().rt_abi_version() == 5 == T.RT_ABI_VERSION


def test_workspace_bytes_positive_and_monotone():
    wsb = tipe_rt.lib().rt_denoise_workspace_bytes
    shapes = sorted([(1, 1), (3, 2), (2, 3), (64, 1), (67, 35), (130, 70), (1200, 900), (3840, 2880), (1, 4000),
                     (32768, 32768)], key=lambda s: s[0] * s[1])
    sizes = [wsb(w, h) for w, h in shapes]
    assert all(b > 0 for b in sizes)
    assert all(b0 <= b1 for b0, b1 in zip(sizes, sizes[1:]))
    assert wsb(3840, 2880) > wsb(1200, 900) > wsb(67, 35)
    assert wsb(67, 35) >= 67 * 35 * 4 * 3 * 4          # two colour buffers and the two guide planes, float3
    assert wsb(0, 5) == 0 and wsb(5, -1) == 0


def test_validation_fails_before_any_device_work():
    """Every refused argument is RT_EINVAL with a message; the pointers are
    never dereferenced (they are not device memory)."""
    L = tipe_rt.lib()
    W, H = 8, 6
    fake = 0x10000
    nbytes = L.rt_denoise_workspace_bytes(W, H)
    good = params_of()
    frame = T.Frame(fake, fake, fake, None)

    def refused(rc):
        assert rc == T.RT_EINVAL
        assert L.rt_last_error()

    def run(W=W, H=H, frame=frame, params=good, ws=fake, nbytes=nbytes):
        return L.rt_denoise_async(W, H, None if frame is None else C.byref(frame),
                                  None if params is None else C.byref(params), ws, nbytes, None, None)

    refused(run(W=0))
    refused(run(H=0))
    refused(run(W=-3))
    refused(run(frame=None))
    refused(run(frame=T.Frame(None, fake, fake, None)))
    refused(run(params=None))
    refused(run(ws=None))
    refused(run(nbytes=nbytes - 1))
    refused(run(nbytes=0))
    refused(run(ws=fake + 4))                      # misaligned: 16 bytes are required
    refused(run(ws=fake + 8))
    # a frame above 2^30 pixels, with nothing else to refuse it for
    assert L.rt_denoise_workspace_bytes(32769, 32768) == 0
    refused(run(W=32769, H=32768, nbytes=1 << 62))
    refused(L.rt_denoise_host(32769, 32768, fake, None, None, C.byref(good)))
    for it in (0, -1, 9):
        refused(run(params=params_of(iterations=it)))
    bad_sigmas = (math.nan, math.inf, -math.inf, 0.0, -1.0, 2.0 ** -9, np.nextafter(F(2.0 ** -8), F(0)),
                  np.nextafter(F(2.0 ** 8), F(1e9)), 1e30)
    for field in ("sigma_color", "sigma_normal", "sigma_albedo"):
        for v in bad_sigmas:
            refused(run(params=params_of(**{field: float(v)})))
            refused(L.rt_set_denoise_params(C.byref(params_of(**{field: float(v)}))))
    # the host path and the process-wide parameters validate the same way
    buf = np.zeros((H, W, 3))
    refused(L.rt_denoise_host(0, H, buf.ctypes.data, None, None, C.byref(good)))
    refused(L.rt_denoise_host(W, H, None, None, None, C.byref(good)))
    refused(L.rt_denoise_host(W, H, buf.ctypes.data, None, None, None))
    refused(L.rt_denoise_host(W, H, buf.ctypes.data, None, None, C.byref(params_of(iterations=9))))
    refused(L.rt_set_denoise_params(C.byref(params_of(iterations=0))))
    assert L.rt_set_denoise_params(C.byref(params_of(sigma_color=2.0 ** -8, sigma_albedo=2.0 ** 8))) == T.RT_OK
    assert L.rt_set_denoise_params(None) == T.RT_OK


def test_restatement_keeps_a_flat_image():
    """A sanity check of the restatement itself: equal taps average to themselves."""
    canva = np.full((9, 11, 3), 51.0)
    c, q = restate(canva, np.zeros((9, 11, 3)), np.zeros((9, 11, 3)), iterations=3)
    # 3 passes of at most 27 roundings each, 2^-24 relative, on values of 0.2: below 1e-6
    assert np.abs(c - F(0.2)).max() <= 1e-6 and np.abs(q - 51.0).max() <= 1.0


@pytest.mark.parametrize("use_albedo,use_normal", [(True, True), (False, True), (True, False), (False, False)])
def test_restatement_equals_a_scalar_reading_of_the_header(use_albedo, use_normal):
    """The oracle's shifted slices against per-pixel loops over the same text, bit for bit."""
    canva, albedo, normal = frames(H=7, W=9, seed=31)
    args = (canva, albedo if use_albedo else None, normal if use_normal else None)
    kw = dict(iterations=3, sigma_color=0.37, sigma_normal=1.7, sigma_albedo=2.0 ** -8)
    want_c, want_canva = restate_scalar(*args, **kw)
    got_c, got_canva = restate(*args, **kw)
    assert (got_c.view(np.uint32) == want_c.view(np.uint32)).all()
    assert (got_canva == want_canva).all()


F64_SEEDS = (41, 42, 43)
F64_BOUND = 4 * 8.329e-07


@pytest.mark.parametrize("kw", [{}, {"iterations": 8}], ids=["defaults", "8-iterations"])
def test_restatement_is_close_to_a_float64_evaluation(kw):
    """max |c - float64 evaluation| on 19x23 frames.  Measured (restatement
    against evaluate_f64, no GPU involved), seeds 41 / 42 / 43:
        defaults      6.679e-07  7.733e-07  7.760e-07   (11.2, 13.0, 13.0 x 2^-24)
        8 iterations  6.949e-07  7.766e-07  8.329e-07   (11.7, 13.0, 14.0 x 2^-24)
    The bound is 4 x the largest of the six, which leaves room for other seeds;
    a wrong formula shows at 1e-3 or more."""
    for seed in F64_SEEDS:
        fr = frames(H=23, W=19, seed=seed)
        err = float(np.abs(restate(*fr, **dict(DEFAULTS, **kw))[0] - evaluate_f64(*fr, **dict(DEFAULTS, **kw))).max())
        print("seed %d %s: max |c32 - c64| = %.3e = %.2f x 2^-24" % (seed, kw, err, err * 2.0 ** 24))
        assert err <= F64_BOUND


# ---- on the GPU: bit-exact against the restatement ----------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("W,H,iterations", [(1, 1, 1),        # only the centre tap is inside
                                            (3, 2, 5),        # every step leaves the image
                                            (67, 35, 1), (67, 35, 2), (67, 35, 3), (67, 35, 4), (67, 35, 5),
                                            (130, 70, 5),     # step-16 taps cross blocks in both directions
                                            (130, 70, 8)])    # steps 32..128: the other (plain) pass kernel
def test_device_filter_is_bit_exact(W, H, iterations):
    check_bit_exact(W, H, seed=10 + iterations, iterations=iterations)


@pytest.mark.gpu
@pytest.mark.parametrize("use_albedo,use_normal", [(False, True), (True, False), (False, False)])
def test_null_planes_drop_their_factor(use_albedo, use_normal):
    check_bit_exact(67, 35, seed=21, use_albedo=use_albedo, use_normal=use_normal, iterations=3)


@pytest.mark.gpu
@pytest.mark.parametrize("sig", [(2.0 ** -8, 2.0 ** 8, 1.5), (2.0 ** 8, 2.0 ** -8, 0.3), (0.37, 1.7, 2.0 ** -8),
                                 (2.0 ** -8, 2.0 ** -8, 2.0 ** -8), (2.0 ** 8, 2.0 ** 8, 2.0 ** 8)])
def test_non_default_sigmas(sig):
    check_bit_exact(67, 35, seed=22, iterations=5, sigma_color=sig[0], sigma_normal=sig[1], sigma_albedo=sig[2])


# ---- host path and hook --------------------------------------------------------

@pytest.mark.gpu
def test_host_path_equals_device_path():
    canva, albedo, normal = frames(H=35, W=67, seed=23)
    before = [x.copy() for x in (canva, albedo, normal)]
    _, dev_canva, _, _ = device_denoise(canva, albedo, normal)
    got = tipe_rt.denoise(canva, albedo, normal)
    assert (got == dev_canva).all()
    assert all((x == b).all() for x, b in zip((canva, albedo, normal), before))
    # planes left out on the host are left out on the device
    _, dev_canva, _, _ = device_denoise(canva, None, None, iterations=2)
    assert (tipe_rt.denoise(canva, params=params_of(iterations=2)) == dev_canva).all()


@pytest.mark.gpu
def test_hook_denoises_the_full_frame_only():
    bundle = helpers.cornell()
    W, H = 24, 18
    p = helpers.params(W, H, 2, 4)
    plain = tipe_rt.render_rows(bundle.scene, p)
    want = restate(*plain, **DEFAULTS)[1]
    assert (want != plain[0]).any()
    try:
        tipe_rt.set_denoise_atrous(True)
        full = tipe_rt.render_rows(bundle.scene, p)
        band = tipe_rt.render_rows(bundle.scene, p, row_hi=9, row_lo=0)
        tipe_rt.set_denoise_atrous(True, params_of(iterations=2, sigma_color=0.5))
        other = tipe_rt.render_rows(bundle.scene, p)
    finally:
        tipe_rt.set_denoise_atrous(False)
    assert not tipe_rt.lib().rt_get_denoise_hook()
    assert (full[0] == want).all()
    assert (full[1] == plain[1]).all() and (full[2] == plain[2]).all()
    assert (band[0][:10] == plain[0][:10]).all() and (band[0][10:] == 0).all()     # a band: rendered, not filtered
    assert (other[0] == restate(*plain, **dict(DEFAULTS, iterations=2, sigma_color=0.5))[1]).all()
    # back to the defaults: the process-wide parameters were restored
    canva = plain[0].copy()
    tipe_rt.lib().rt_denoise_atrous(W, H, canva.ctypes.data, p.cam, plain[1].ctypes.data, plain[2].ctypes.data)
    assert (canva == want).all()


# ---- it denoises ----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "pyramid"])
def test_denoised_frame_is_closer_to_the_converged_one(scene):
    """64x48, 6 bounces, chunks = 1: a 16-spp frame (seed 7), denoised with
    the default parameters, against the 2048-spp frame (seed 1010):
    RMSE(denoised, ref) <= 0.6 RMSE(noisy, ref) over the canva.  CPU oracle
    renders filtered with the restatement give ratios of 0.481
    (cornell) and 0.494 (pyramid); render and filter are both bit-exact, so the
    GPU reproduces them."""
    bundle = helpers.cornell() if scene == "cornell" else helpers.pyramid_scene()
    W, H = 64, 48
    noisy = tipe_rt.render_rows(bundle.scene, helpers.params(W, H, 16, 6, seed=7, chunks=1))
    ref = tipe_rt.render_rows(bundle.scene, helpers.params(W, H, 2048, 6, seed=1010, chunks=1))[0]
    den = tipe_rt.denoise(*noisy)
    rmse = lambda x: float(np.sqrt(((x - ref) ** 2).mean()))  # noqa: E731
    ratio = rmse(den) / rmse(noisy[0])
    print("%s: RMSE noisy %.4f, denoised %.4f, ratio %.3f" % (scene, rmse(noisy[0]), rmse(den), ratio))
    assert ratio <= 0.6
