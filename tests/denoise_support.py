"""What the three denoiser test files share: random frames, denoiser.h's
buffer formats, the float32 restatement of rt.h's filter (the thing the
built-in denoiser is specified by) and one call of rt_denoise_async."""
import numpy as np

import tipe_rt

F = np.float32
TAP_H = np.array([1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0], dtype=F)
DEFAULTS = dict(iterations=4, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.25)


def reference_pack(canva, albedo, normal):
    """denoiser.h:44-60: (float)canva / 255.0f, (float)albedo, (float)normal."""
    return (canva.astype(np.float32) / np.float32(255.0), albedo.astype(np.float32), normal.astype(np.float32))


def frames(H=7, W=9, seed=0):
    rng = np.random.default_rng(seed)
    canva = rng.integers(0, 256, (H, W, 3)).astype(np.float64)
    albedo = rng.uniform(0, 1, (H, W, 3))
    normal = rng.uniform(-1, 1, (H, W, 3))
    return canva, albedo, normal


def restate(canva, albedo, normal, iterations=4, sigma_color=1.0, sigma_normal=0.5, sigma_albedo=0.25):
    """rt.h's filter in float32: returns (c before quantisation, canva after)."""
    c = canva.astype(F) / F(255.0)
    a = None if albedo is None else albedo.astype(F)
    n = None if normal is None else normal.astype(F)
    H, W = c.shape[:2]
    one = F(1.0)
    sn2 = F(sigma_normal) * F(sigma_normal)
    sa2 = F(sigma_albedo) * F(sigma_albedo)

    def d2(X, Q, P):
        D = X[Q] - X[P]
        return (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]

    def k(x):
        return one / (one + x)

    for i in range(iterations):
        s = 1 << i
        sc = F(sigma_color) * F(2.0 ** -i)
        sc2 = sc * sc
        acc = np.zeros((H, W, 3), dtype=F)
        ws = np.zeros((H, W), dtype=F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = s * dy, s * dx
                y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
                if y0 >= y1 or x0 >= x1:
                    continue                      # the tap is outside the image for every pixel
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                w = (TAP_H[dy + 2] * TAP_H[dx + 2]) * k(d2(c, Q, P) / sc2)
                if n is not None:
                    w = w * k(d2(n, Q, P) / sn2)
                if a is not None:
                    w = w * k(d2(a, Q, P) / sa2)
                assert w.dtype == F, w.dtype
                acc[P] = acc[P] + w[..., None] * c[Q]
                ws[P] = ws[P] + w
        c = acc / ws[..., None]
        assert c.dtype == F, c.dtype
    return c, np.trunc(c * F(255.0)).astype(np.int64).astype(np.float64)


def params_of(**kw):
    return tipe_rt.denoise_params(**kw)


def device_denoise(canva, albedo, normal, **kw):
    """rt_denoise_async on device copies: (color3_out, canva, albedo, normal) back on the host."""
    import torch
    dev = torch.device("cuda:0")
    H, W = canva.shape[:2]
    t = [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (canva, albedo, normal)]
    nbytes = tipe_rt.lib().rt_denoise_workspace_bytes(W, H)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    c3 = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    tipe_rt.denoise_async(W, H, t[0].data_ptr(), None if t[1] is None else t[1].data_ptr(),
                          None if t[2] is None else t[2].data_ptr(), params_of(**kw), ws.data_ptr(), nbytes,
                          c3.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [c3.cpu().numpy()] + [None if x is None else x.cpu().numpy() for x in t]
