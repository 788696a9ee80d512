"""What the variance-guided denoiser's test files share: seeded synthetic
accumulators, the float32 restatement of rt.h's text (the thing the filter is
specified by) and one call of rt_vdenoise_async."""
import functools

import numpy as np

import tipe_rt

F = np.float32
D = np.float64
TAP_H = np.array([1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0], dtype=F)
BLUR_G = np.array([0.25, 0.5, 0.25], dtype=F)
L_FLOOR = F(2.0 ** -26)
DEFAULTS = dict(iterations=4, sigma_luminance=4.0, sigma_normal=0.5, sigma_albedo=0.25)
PLANES = ("canva", "albedo", "normal", "radiance")


def sums(W, H, n, seed):
    """Two (H, W, 9) float64 accumulators of n samples per pixel: radiance in
    [0, 4] n, albedo in [0, 1] n, normal in [-1, 1] n."""
    rng = np.random.default_rng(seed)
    lo = np.array([0.0] * 6 + [-1.0] * 3)
    hi = np.array([4.0] * 3 + [1.0] * 6)
    return tuple(rng.uniform(lo, hi, (H, W, 9)) * n for _ in range(2))


def lum2(d):
    """(0.25f*(D0*D0) + 0.5f*(D1*D1)) + 0.25f*(D2*D2) over the last axis."""
    return (F(0.25) * (d[..., 0] * d[..., 0]) + F(0.5) * (d[..., 1] * d[..., 1])) + F(0.25) * (d[..., 2] * d[..., 2])


def dist2(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def means(A, B, n):
    """rt.h "means and variance": the float32 planes c, v, a, nn."""
    rap = D(1.0) / D(n)
    mA, mB = (rap * A).astype(F), (rap * B).astype(F)
    half = F(0.5)
    c = half * (mA[..., 0:3] + mB[..., 0:3])
    a = half * (mA[..., 3:6] + mB[..., 3:6])
    nn = half * (mA[..., 6:9] + mB[..., 6:9])
    d = half * (mA[..., 0:3] - mB[..., 0:3])
    return c, lum2(d), a, nn


def shifted(H, W, oy, ox):
    """Index pairs (P, Q): the pixels p whose tap q = p + (ox, oy) is inside, and those taps; None if there are none."""
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def luminance_bound(v, sl2):
    """L = sl2 * (3x3 blur of v) + 2^-26."""
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
    return sl2 * (bn / bd) + L_FLOOR


def finish(c, A, B, n):
    """rt.h "finish": the four output planes of the filtered colour c."""
    r = np.sqrt(c).astype(D)
    assert np.sqrt(c).dtype == F
    r = np.where(r < 0.0, 0.0, np.where(r > 0.999, 0.999, r))
    rap2 = D(1.0) / (D(2.0) * D(n))
    return dict(canva=np.trunc(256 * r), albedo=(A[..., 3:6] + B[..., 3:6]) * rap2,
                normal=(A[..., 6:9] + B[..., 6:9]) * rap2, radiance=c.astype(D), c=c)


def restate(A, B, n, iterations=4, sigma_luminance=4.0, sigma_normal=0.5, sigma_albedo=0.25):
    """rt.h's variance-guided filter in float32 on the accumulators A, B of n
    samples each: dict of canva, albedo, normal, radiance (float64) and c (float32)."""
    c, v, a, nn = means(A, B, n)
    H, W = v.shape
    sl2 = F(sigma_luminance) * F(sigma_luminance)
    sn2 = F(sigma_normal) * F(sigma_normal)
    sa2 = F(sigma_albedo) * F(sigma_albedo)
    snsa = sn2 * sa2
    for i in range(iterations):
        s = 1 << i
        L = luminance_bound(v, sl2)
        acc = np.zeros((H, W, 3), dtype=F)
        accv = np.zeros((H, W), dtype=F)
        ws = np.zeros((H, W), dtype=F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                pq = shifted(H, W, s * dy, s * dx)
                if pq is None:
                    continue                      # the tap is outside the image for every pixel
                P, Q = pq
                dl = lum2(c[Q] - c[P])
                dn, da = dist2(nn[Q] - nn[P]), dist2(a[Q] - a[P])
                num = ((TAP_H[dy + 2] * TAP_H[dx + 2]) * L[P]) * snsa
                den = ((L[P] + dl) * (sn2 + dn)) * (sa2 + da)
                w = num / den
                assert w.dtype == F, w.dtype
                acc[P] = acc[P] + w[..., None] * c[Q]
                accv[P] = accv[P] + (w * w) * v[Q]
                ws[P] = ws[P] + w
        c, v = acc / ws[..., None], accv / (ws * ws)
        assert c.dtype == F and v.dtype == F
    return finish(c, A, B, n)


@functools.lru_cache(maxsize=None)
def case(W, H, n, seed, iterations, sigmas=None):
    """(A, B, restated planes) of a seeded frame; shared among tests, never written."""
    A, B = sums(W, H, n, seed)
    kw = dict(DEFAULTS, iterations=iterations)
    if sigmas is not None:
        kw.update(zip(("sigma_luminance", "sigma_normal", "sigma_albedo"), sigmas))
    return A, B, restate(A, B, n, **kw)


def params_of(**kw):
    return tipe_rt.vdenoise_params(**kw)


def enqueue(A, B, n, stream, planes=PLANES, ws=None, **kw):
    """Uploads the accumulators and calls rt_vdenoise_async, all on `stream`,
    and waits for nothing.  ws: a uint8 device tensor (default: a fresh one of
    exactly the required size, filled with NaN bytes: nothing is read
    unwritten).  Returns {plane: device tensor} for the planes asked for."""
    import torch
    H, W = A.shape[:2]
    with torch.cuda.stream(stream):
        dA, dB = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (A, B))
        nbytes = tipe_rt.lib().rt_vdenoise_workspace_bytes(W, H)
        if ws is None:
            ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda:0")
        out = {k: torch.full((H, W, 3), -7.0, dtype=torch.float64, device="cuda:0") for k in planes}
    tipe_rt.vdenoise_async(W, H, dA.data_ptr(), dB.data_ptr(), n, params_of(**kw), ws.data_ptr(), nbytes,
                           *[out[k].data_ptr() if k in out else None for k in PLANES], stream=stream.cuda_stream)
    out["_keep"] = (dA, dB, ws)
    return out


def device_vdenoise(A, B, n, **kw):
    """One rt_vdenoise_async call on torch's current stream: {plane: host array}."""
    import torch
    out = enqueue(A, B, n, torch.cuda.current_stream(), **kw)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items() if k != "_keep"}


def assert_planes(got, want):
    """Bit for bit on every plane that was asked for."""
    for k in PLANES:
        if k not in got:
            continue
        g = got[k] if isinstance(got[k], np.ndarray) else got[k].cpu().numpy()
        bad = g.view(np.uint64) != np.ascontiguousarray(want[k]).view(np.uint64)
        assert not bad.any(), "%s: %d of %d values differ, first at (y, x, ch) %s" % (
            k, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]))


def check_case(W, H, n, seed, iterations, sigmas=None):
    A, B, want = case(W, H, n, seed, iterations, sigmas)
    kw = dict(iterations=iterations)
    if sigmas is not None:
        kw.update(zip(("sigma_luminance", "sigma_normal", "sigma_albedo"), sigmas))
    assert_planes(device_vdenoise(A, B, n, **kw), want)
