"""What the tests of the variance-guided denoiser with per-pixel sample counts
share: the float32 restatement of rt.h's text ("variance-guided denoiser with
per-pixel sample counts": the uniform filter's text with n_p in two places),
seeded synthetic accumulators whose pixel p holds n_p samples' worth of sums,
and one call of rt_vdenoise_adaptive_async."""
import functools

import numpy as np

import tipe_rt
from vdenoise_support import D, DEFAULTS, F, PLANES, TAP_H, dist2, lum2, luminance_bound, params_of, shifted

SIGMAS = ("sigma_luminance", "sigma_normal", "sigma_albedo")


# ---- rt.h in float32 -----------------------------------------------------------

def counts(rounds, first_half):
    """n_p = first_half * 2^(k-1), k = min(max(rounds[p], 1), 32): int64, the shape of rounds."""
    k = np.clip(np.asarray(rounds, dtype=np.int64), 1, 32)
    return np.int64(first_half) << (k - 1)


def means(A, B, n_p):
    """"Means and variance" with rap = 1.0 / (double)n_p per pixel: the float32 planes c, v, a, nn."""
    rap = (D(1.0) / n_p.astype(D))[..., None]
    mA, mB = (rap * A).astype(F), (rap * B).astype(F)
    half = F(0.5)
    c = half * (mA[..., 0:3] + mB[..., 0:3])
    a = half * (mA[..., 3:6] + mB[..., 3:6])
    nn = half * (mA[..., 6:9] + mB[..., 6:9])
    d = half * (mA[..., 0:3] - mB[..., 0:3])
    return c, lum2(d), a, nn


def passes(c, v, a, nn, iterations, sigma_luminance, sigma_normal, sigma_albedo):
    """The passes i = 0 .. iterations-1 of the uniform filter's text: they do not know the counts."""
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
                    continue
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
    return c


def finish(c, A, B, n_p):
    """"Finish" with 1.0 / (2.0 * (double)n_p) per pixel, that quotient first."""
    r = np.sqrt(c).astype(D)
    assert np.sqrt(c).dtype == F
    r = np.where(r < 0.0, 0.0, np.where(r > 0.999, 0.999, r))
    rap2 = (D(1.0) / (D(2.0) * n_p.astype(D)))[..., None]
    return dict(canva=np.trunc(256 * r), albedo=(A[..., 3:6] + B[..., 3:6]) * rap2,
                normal=(A[..., 6:9] + B[..., 6:9]) * rap2, radiance=c.astype(D), c=c)


def restate(A, B, rounds, first_half, iterations=4, sigma_luminance=4.0, sigma_normal=0.5, sigma_albedo=0.25):
    """The filter on accumulators A, B (H, W, 9) whose pixel p holds n_p
    samples each, rounds (H, W) ints: dict of canva, albedo, normal, radiance
    (float64) and c (float32)."""
    n_p = counts(rounds, first_half)
    c, v, a, nn = means(A, B, n_p)
    return finish(passes(c, v, a, nn, iterations, sigma_luminance, sigma_normal, sigma_albedo), A, B, n_p)


# ---- synthetic inputs -----------------------------------------------------------

def sums(rounds, first_half, seed):
    """Two (H, W, 9) float64 accumulators, pixel p holding n_p samples' worth:
    radiance in [0, 4] n_p, albedo in [0, 1] n_p, normal in [-1, 1] n_p
    (vdenoise_support.sums' distributions)."""
    rng = np.random.default_rng(seed)
    lo = np.array([0.0] * 6 + [-1.0] * 3)
    hi = np.array([4.0] * 3 + [1.0] * 6)
    n_p = counts(rounds, first_half).astype(D)[..., None]
    return tuple(rng.uniform(lo, hi, rounds.shape + (9,)) * n_p for _ in range(2))


def mixed_rounds(W, H, seed, lo=1, hi=5):
    """Seeded round counts lo..hi, one per pixel: (H, W) int32."""
    return np.random.default_rng(seed).integers(lo, hi + 1, (H, W)).astype(np.int32)


def kwargs_of(iterations, sigmas=None):
    kw = dict(DEFAULTS, iterations=iterations)
    if sigmas is not None:
        kw.update(zip(SIGMAS, sigmas))
    return kw


@functools.lru_cache(maxsize=None)
def case(W, H, first_half, seed, iterations, sigmas=None):
    """(A, B, rounds, restated planes) of a seeded frame with mixed round counts 1..5; shared, never written."""
    rounds = mixed_rounds(W, H, seed)
    A, B = sums(rounds, first_half, seed + 1)
    return A, B, rounds, restate(A, B, rounds, first_half, **kwargs_of(iterations, sigmas))


# ---- device driver ---------------------------------------------------------------

def enqueue(A, B, rounds, first_half, stream, planes=PLANES, **kw):
    """Uploads the accumulators and the round counts and calls
    rt_vdenoise_adaptive_async, all on `stream`, and waits for nothing.  The
    workspace is exactly the required size and filled with 0xFF bytes (NaNs).
    Returns {plane: device tensor} and, under "_keep", (dA, dB, d_rounds, ws)."""
    import torch
    H, W = A.shape[:2]
    with torch.cuda.stream(stream):
        dA, dB = (torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (A, B))
        dR = torch.from_numpy(np.ascontiguousarray(rounds, dtype=np.int32)).to("cuda:0")
        nbytes = tipe_rt.lib().rt_vdenoise_workspace_bytes(W, H)
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda:0")
        out = {k: torch.full((H, W, 3), -7.0, dtype=torch.float64, device="cuda:0") for k in planes}
    tipe_rt.vdenoise_adaptive_async(W, H, dA.data_ptr(), dB.data_ptr(), dR.data_ptr(), first_half, params_of(**kw),
                                    ws.data_ptr(), nbytes, *[out[k].data_ptr() if k in out else None for k in PLANES],
                                    stream=stream.cuda_stream)
    out["_keep"] = (dA, dB, dR, ws)
    return out


def device_filter(A, B, rounds, first_half, **kw):
    """One call on torch's current stream: ({plane: host array}, the device tensors kept)."""
    import torch
    out = enqueue(A, B, rounds, first_half, torch.cuda.current_stream(), **kw)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items() if k != "_keep"}, out["_keep"]
