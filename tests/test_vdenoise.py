"""The variance-guided denoiser (rt.h "variance-guided denoiser"): an
edge-avoiding a-trous filter of the pre-gamma radiance whose colour weight
follows the dual-buffer variance of two half-sample accumulators.

rt.h specifies it operation by operation in IEEE binary32, so the NumPy
float32 restatement in tests/vdenoise_support.py (written from that text, not
from the kernels) must equal the GPU bit for bit on canva, radiance, albedo
and normal.  Defaults, the workspace size, validation, the restatement's own
checks and the kernels' resource usage run without a GPU."""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import tipe_rt
from tipe_rt import types as T
from gpu_driver import device_planes
from vdenoise_support import (F, D, DEFAULTS, PLANES, sums, means, restate, params_of, device_vdenoise,
                              assert_planes, check_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- rt.h once more, one pixel and one tap at a time -----------------------------

def restate_scalar(A, B, n, iterations=4, sigma_luminance=4.0, sigma_normal=0.5, sigma_albedo=0.25):
    """rt.h's text on np.float32 scalars in the header's loop order: no
    slicing, so it shares nothing with restate's P/Q bookkeeping.  Returns the
    filtered colour c (H, W, 3) float32."""
    H, W = A.shape[:2]
    rap = D(1.0) / D(n)
    q, h2, h = F(0.25), F(0.5), [F(1.0) / F(16.0), F(1.0) / F(4.0), F(3.0) / F(8.0), F(1.0) / F(4.0), F(1.0) / F(16.0)]
    g = [F(0.25), F(0.5), F(0.25)]

    def lum(d):
        return (q * (d[0] * d[0]) + h2 * (d[1] * d[1])) + q * (d[2] * d[2])

    def d2(X, qy, qx, py, px):
        d = [X[qy][qx][k] - X[py][px][k] for k in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]

    c, a, nn, v = ([[None] * W for _ in range(H)] for _ in range(4))
    for y in range(H):
        for x in range(W):
            mA = [F(rap * D(A[y, x, k])) for k in range(9)]
            mB = [F(rap * D(B[y, x, k])) for k in range(9)]
            c[y][x] = [h2 * (mA[k] + mB[k]) for k in range(3)]
            a[y][x] = [h2 * (mA[3 + k] + mB[3 + k]) for k in range(3)]
            nn[y][x] = [h2 * (mA[6 + k] + mB[6 + k]) for k in range(3)]
            v[y][x] = lum([h2 * (mA[k] - mB[k]) for k in range(3)])
    sl2 = F(sigma_luminance) * F(sigma_luminance)
    sn2 = F(sigma_normal) * F(sigma_normal)
    sa2 = F(sigma_albedo) * F(sigma_albedo)
    for i in range(iterations):
        s = 1 << i
        cn, vn = [[None] * W for _ in range(H)], [[None] * W for _ in range(H)]
        for y in range(H):
            for x in range(W):
                bn, bd = F(0.0), F(0.0)
                for dy in range(-1, 2):
                    for dx in range(-1, 2):
                        if 0 <= y + dy < H and 0 <= x + dx < W:
                            gg = g[dy + 1] * g[dx + 1]
                            bn = bn + gg * v[y + dy][x + dx]
                            bd = bd + gg
                L = sl2 * (bn / bd) + F(2.0 ** -26)
                acc, accv, ws = [F(0.0), F(0.0), F(0.0)], F(0.0), F(0.0)
                for dy in range(-2, 3):
                    qy = y + s * dy
                    if qy < 0 or qy >= H:
                        continue
                    for dx in range(-2, 3):
                        qx = x + s * dx
                        if qx < 0 or qx >= W:
                            continue
                        dl = lum([c[qy][qx][k] - c[y][x][k] for k in range(3)])
                        dn, da = d2(nn, qy, qx, y, x), d2(a, qy, qx, y, x)
                        num = ((h[dy + 2] * h[dx + 2]) * L) * (sn2 * sa2)
                        den = ((L + dl) * (sn2 + dn)) * (sa2 + da)
                        w = num / den
                        assert type(w) is F
                        acc = [acc[k] + w * c[qy][qx][k] for k in range(3)]
                        accv = accv + (w * w) * v[qy][qx]
                        ws = ws + w
                cn[y][x] = [acc[k] / ws for k in range(3)]
                vn[y][x] = accv / (ws * ws)
        c, v = cn, vn
    return np.array(c, dtype=F)


def evaluate_f64(A, B, n, iterations=4, sigma_luminance=4.0, sigma_normal=0.5, sigma_albedo=0.25):
    """rt.h's formulas in float64 on the binary32 means (c, a, nn and the half
    difference rounded to float32 first, the sigmas too): the filtered colour
    without the binary32 roundings of the filter itself.  Taps outside the
    image are masked in zero-padded planes, not sliced away."""
    c, _, a, nn = (x.astype(D) for x in means(A, B, n))
    rap = D(1.0) / D(n)
    d = (F(0.5) * ((rap * A).astype(F)[..., :3] - (rap * B).astype(F)[..., :3])).astype(D)
    lum = lambda X: 0.25 * X[..., 0] ** 2 + 0.5 * X[..., 1] ** 2 + 0.25 * X[..., 2] ** 2  # noqa: E731
    v = lum(d)
    H, W = v.shape
    sl2, sn2, sa2 = (D(F(s)) ** 2 for s in (sigma_luminance, sigma_normal, sigma_albedo))
    inside = np.ones((H, W))
    hh, gg = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], [0.25, 0.5, 0.25]
    for i in range(iterations):
        s = 1 << i
        m = 2 * s
        pad = lambda X, m=m: np.pad(X, [(m, m), (m, m)] + [(0, 0)] * (X.ndim - 2))  # noqa: E731
        at = lambda X, oy, ox, m=m: X[m + oy:m + oy + H, m + ox:m + ox + W]  # noqa: E731
        cp, vp, ap, npad, ip = pad(c), pad(v), pad(a), pad(nn), pad(inside)
        bn = sum(gg[dy + 1] * gg[dx + 1] * at(vp, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
        bd = sum(gg[dy + 1] * gg[dx + 1] * at(ip, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
        L = sl2 * bn / bd + 2.0 ** -26
        acc, accv, ws = np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = s * dy, s * dx
                w = (hh[dy + 2] * hh[dx + 2] * L * sn2 * sa2 * at(ip, oy, ox)
                     / ((L + lum(at(cp, oy, ox) - c)) * (sn2 + ((at(npad, oy, ox) - nn) ** 2).sum(-1))
                        * (sa2 + ((at(ap, oy, ox) - a) ** 2).sum(-1))))
                acc += w[..., None] * at(cp, oy, ox)
                accv += w * w * at(vp, oy, ox)
                ws += w
        c, v = acc / ws[..., None], accv / ws ** 2
    return c


# ---- without a GPU ------------------------------------------------------------

def test_params_init_defaults():
    p = T.VDenoiseParams(99, 9.0, 9.0, 9.0)
    tipe_rt.lib().rt_vdenoise_params_init(C.byref(p))
    assert (p.iterations, p.sigma_luminance, p.sigma_normal, p.sigma_albedo) == (4, 4.0, 0.5, 0.25)
    q = params_of(iterations=0, sigma_albedo=2.0)
    assert (q.iterations, q.sigma_luminance, q.sigma_normal, q.sigma_albedo) == (0, 4.0, 0.5, 2.0)
    assert tipe_rt.lib().rt_abi_version() == 5          # additions to 5: detected by symbol


def test_workspace_bytes_positive_and_monotone():
    wsb = tipe_rt.lib().rt_vdenoise_workspace_bytes
    shapes = sorted([(1, 1), (3, 2), (2, 3), (64, 1), (67, 35), (130, 70), (1200, 900), (3840, 2880), (1, 4000),
                     (32768, 32768)], key=lambda s: s[0] * s[1])
    sizes = [wsb(w, h) for w, h in shapes]
    assert all(b > 0 for b in sizes)
    assert all(b0 <= b1 for b0, b1 in zip(sizes, sizes[1:]))
    assert wsb(3840, 2880) > wsb(1200, 900) > wsb(67, 35)
    # two colour and two variance buffers, the two guide planes and L
    assert wsb(67, 35) >= 67 * 35 * (4 * 3 + 3) * 4
    assert wsb(0, 5) == 0 and wsb(5, -1) == 0 and wsb(32769, 32768) == 0


def test_entry_points_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", tipe_rt.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    new = {"rt_vdenoise_params_init", "rt_vdenoise_workspace_bytes", "rt_vdenoise_async", "rt_render_vdenoised"}
    assert new <= syms and new <= set(tipe_rt.EXPORTED_SYMBOLS)


def test_validation_fails_before_any_device_work():
    """Every refused argument is RT_EINVAL with a message; the pointers are
    never dereferenced (they are not device memory)."""
    L = tipe_rt.lib()
    W, H = 8, 6
    fake = 0x10000
    nbytes = L.rt_vdenoise_workspace_bytes(W, H)
    good = params_of()
    frame = T.Frame(fake, fake, fake, fake)

    def refused(rc):
        assert rc == T.RT_EINVAL
        assert L.rt_last_error()

    def run(W=W, H=H, a=fake, b=fake, n=4, params=good, ws=fake, nbytes=nbytes, out=frame):
        return L.rt_vdenoise_async(W, H, a, b, n, None if params is None else C.byref(params), ws, nbytes,
                                   None if out is None else C.byref(out), None)

    refused(run(W=0))
    refused(run(H=0))
    refused(run(W=-3))
    refused(run(W=32769, H=32768, nbytes=1 << 62))            # above 2^30 pixels, nothing else to refuse it for
    refused(run(a=None))
    refused(run(b=None))
    refused(run(params=None))
    refused(run(out=None))
    refused(run(out=T.Frame(None, fake, fake, fake)))
    refused(run(n=0))
    refused(run(n=-2))
    refused(run(ws=None))
    refused(run(nbytes=nbytes - 1))
    refused(run(nbytes=0))
    refused(run(ws=fake + 4))                                  # misaligned: 16 bytes are required
    refused(run(ws=fake + 8))
    for it in (-1, 9):
        refused(run(params=params_of(iterations=it)))
    bad_sigmas = (math.nan, math.inf, -math.inf, 0.0, -1.0, 2.0 ** -9, np.nextafter(F(2.0 ** -8), F(0)),
                  np.nextafter(F(2.0 ** 8), F(1e9)), 1e30)
    for field in ("sigma_luminance", "sigma_normal", "sigma_albedo"):
        for v in bad_sigmas:
            refused(run(params=params_of(**{field: float(v)})))
    # the host path: the same parameters, an even sample count of at least 2, a canva
    bundle = helpers.cornell()
    buf = np.zeros((H, W, 3))

    def host(spp=4, vp=good, canva=buf.ctypes.data, scene=bundle.scene):
        p = helpers.params(W, H, spp, 2)
        return L.rt_render_vdenoised(None if scene is None else C.byref(scene), C.byref(p),
                                     None if vp is None else C.byref(vp), canva, None, None)

    for spp in (0, 1, 3, 7):
        refused(host(spp=spp))
    refused(host(vp=None))
    refused(host(vp=params_of(iterations=9)))
    refused(host(vp=params_of(sigma_luminance=math.nan)))
    refused(host(canva=None))
    refused(host(scene=None))
    assert (buf == 0).all()


SCALAR_KW = dict(iterations=3, sigma_luminance=1.7, sigma_normal=0.37, sigma_albedo=2.0 ** -8)


@pytest.mark.parametrize("n,kw", [(3, SCALAR_KW), (1, dict(DEFAULTS, iterations=2))], ids=["odd-sigmas", "defaults"])
def test_restatement_equals_a_scalar_reading_of_the_header(n, kw):
    """The restatement's shifted slices against per-pixel loops over the same text, bit for bit."""
    A, B = sums(9, 7, n, seed=31)
    want = restate_scalar(A, B, n, **kw)
    got = restate(A, B, n, **kw)["c"]
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


def test_restatement_of_zero_iterations_is_the_resolved_mean():
    """iterations 0: c is the mean of the two half means, canva its write_color_canva."""
    A, B = sums(9, 7, 8, seed=32)
    r = restate(A, B, 8, iterations=0)
    c = (F(0.5) * ((A[..., :3] / 8).astype(F) + (B[..., :3] / 8).astype(F)))       # 1/8 is exact: rap * X == X / 8
    assert (r["c"].view(np.uint32) == c.view(np.uint32)).all()
    assert (r["canva"] == np.trunc(256 * np.minimum(np.sqrt(c).astype(D), 0.999))).all()
    assert (r["albedo"] == (A[..., 3:6] + B[..., 3:6]) / 16).all()


F64_SEEDS = (41, 42, 43)
F64_MEASURED = 1.510e-06
F64_BOUND = 4 * F64_MEASURED


@pytest.mark.parametrize("kw", [{}, {"iterations": 8}], ids=["defaults", "8-iterations"])
def test_restatement_is_close_to_a_float64_evaluation(kw):
    """max |c - float64 evaluation| on 19x23 frames of radiance in [0, 4],
    spp_half 3.  Measured (restatement against evaluate_f64, no GPU involved),
    seeds 41 / 42 / 43:
        defaults      1.510e-06  1.393e-06  1.459e-06   (25.3, 23.4, 24.5 x 2^-24)
        8 iterations  1.510e-06  1.393e-06  1.322e-06   (25.3, 23.4, 22.2 x 2^-24)
    (beyond step 16 only the centre tap of a 19x23 frame is inside, so the
    later passes move little).  The bound is 4 x the largest of the six, which
    leaves room for other seeds; a wrong formula shows at 1e-2 or more."""
    for seed in F64_SEEDS:
        A, B = sums(19, 23, 3, seed)
        k = dict(DEFAULTS, **kw)
        err = float(np.abs(restate(A, B, 3, **k)["c"].astype(D) - evaluate_f64(A, B, 3, **k)).max())
        print("seed %d %s: max |c32 - c64| = %.3e = %.2f x 2^-24" % (seed, kw, err, err * 2.0 ** 24))
        assert err <= F64_BOUND


def test_new_kernels_use_no_scratch():
    """The resource-usage target's line for rt_vdenoise.hip (the Makefile's
    own flags; the render kernels' lines are test_abi's): 0 spilled VGPRs and
    0 bytes of scratch for each of the five kernels."""
    mk = ["make", "-C", os.path.join(ROOT, "tipe-raytracer_amd")]
    lines = subprocess.run(mk + ["-n", "-B", "resource-usage"], capture_output=True, text=True, check=True).stdout
    cmd = [ln for ln in lines.splitlines() if "rt_vdenoise.hip" in ln and "kernel-resource-usage" in ln]
    assert len(cmd) == 1, lines
    out = subprocess.run(cmd[0], shell=True, cwd=os.path.join(ROOT, "tipe-raytracer_amd"), capture_output=True,
                         text=True)
    txt = out.stdout + out.stderr
    assert out.returncode == 0, txt[-2000:]
    seen = set()
    # (prepare and finish: the <double> instantiations, as the symbols spell them)
    for name in ("prepare_kernelIJdE", "lum_kernel", "pass_kernel", "pass_tiled_kernel", "finish_kernelIJdE"):
        m = re.search(r"Function Name: \S*vdenoise_" + name + r"E.*?ScratchSize \[bytes/lane\]: (\d+).*?"
                      r"SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", txt, re.S)
        assert m, (name, txt[-2000:])
        assert (int(m.group(1)), int(m.group(3))) == (0, 0), (name, m.groups())
        seen.add(name)
    assert len(seen) == 5


# ---- on the GPU: bit-exact against the restatement ----------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("W,H,n,iterations", [(9, 7, 3, 4),          # every step above 2 leaves the image
                                              (1, 1, 1, 3),          # only the centre tap is inside
                                              (1, 40, 8, 6), (40, 1, 3, 6),     # only the centre dx / dy taps exist
                                              (130, 9, 1, 5),        # step-16 taps inside and outside a row, tiled
                                              (70, 40, 8, 6),        # step 32: the first plain-form pass
                                              (260, 5, 3, 8)])       # step 128: x +- 256 is inside
def test_device_filter_is_bit_exact(W, H, n, iterations):
    check_case(W, H, n, 100 + W + iterations, iterations)


# ---- end to end on rendered halves ---------------------------------------------

SIZE = (64, 48)


def bundle_of(scene):
    return helpers.cornell() if scene == "cornell" else helpers.pyramid_scene()


@functools.lru_cache(maxsize=None)
def converged(scene):
    """The 2048-spp canva at seed 1010."""
    return tipe_rt.render_rows(bundle_of(scene).scene, helpers.params(*SIZE, 2048, 6, seed=1010, chunks=1))[0]


@functools.lru_cache(maxsize=None)
def rendered_halves(scene, S, chunks=1):
    """A = samples [0, S/2), B = samples [S/2, S) through rt_accumulate_async,
    and the resolved S-spp frame of the same samples: host arrays
    (A, B, noisy canva, albedo, normal)."""
    import torch
    W, H = SIZE
    bundle = bundle_of(scene)
    half = helpers.params(W, H, S // 2, 6, seed=7, chunks=chunks)
    band = tipe_rt.band_tiling(0, H - 1)
    ds = tipe_rt.DeviceScene(bundle.scene, 0)
    st = torch.cuda.current_stream().cuda_stream
    acc = torch.zeros((3, H, W, 9), dtype=torch.float64, device="cuda:0")
    tipe_rt.accumulate_async(ds, half, 0, band, acc[0].data_ptr(), st)
    tipe_rt.accumulate_async(ds, half, S // 2, band, acc[1].data_ptr(), st)
    tipe_rt.accumulate_async(ds, half, 0, band, acc[2].data_ptr(), st)
    tipe_rt.accumulate_async(ds, half, S // 2, band, acc[2].data_ptr(), st)
    planes = device_planes(H, W, n=3)
    tipe_rt.resolve_async(acc[2].data_ptr(), half, S, band, *[t.data_ptr() for t in planes], stream=st)
    torch.cuda.synchronize()
    ds.close()
    return tuple(acc[k].cpu().numpy() for k in (0, 1)) + tuple(t.cpu().numpy() for t in planes)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [16, 256])
@pytest.mark.parametrize("scene", ["cornell", "pyramid"])
def test_rendered_halves_filter_bit_exactly_and_the_host_path_agrees(scene, S):
    A, B = rendered_halves(scene, S)[:2]
    assert (A != B).any()
    got = device_vdenoise(A, B, S // 2)
    assert_planes(got, restate(A, B, S // 2, **DEFAULTS))
    host = tipe_rt.render_vdenoised(bundle_of(scene).scene, helpers.params(*SIZE, S, 6, seed=7, chunks=1))
    for k, plane in zip(PLANES, host):
        assert (plane == got[k]).all(), k
    canva_only = tipe_rt.render_vdenoised(bundle_of(scene).scene, helpers.params(*SIZE, S, 6, seed=7, chunks=1),
                                          albedo=False, normal=False)
    assert (canva_only[0] == got["canva"]).all() and canva_only[1] is None and canva_only[2] is None


@pytest.mark.gpu
def test_host_path_with_the_default_sample_grouping():
    """spp_chunks = RT_SPP_CHUNKS_AUTO, what rt_params_init sets: each half is
    accumulated in min(32, S/2) slices, on the host path as in the device
    composition."""
    S = 64
    A, B = rendered_halves("pyramid", S, chunks=T.RT_SPP_CHUNKS_AUTO)[:2]
    got = device_vdenoise(A, B, S // 2)
    assert_planes(got, restate(A, B, S // 2, **DEFAULTS))
    p = helpers.params(*SIZE, S, 6, seed=7, chunks=T.RT_SPP_CHUNKS_AUTO)
    host = tipe_rt.render_vdenoised(bundle_of("pyramid").scene, p)
    for k, plane in zip(PLANES, host):
        assert (plane == got[k]).all(), k


def ratios(scene, S):
    """(ratio of the new filter, ratio of the a-trous filter at its defaults on the same noisy frame)."""
    A, B, noisy, albedo, normal = rendered_halves(scene, S)
    ref = converged(scene)
    rmse = lambda x: float(np.sqrt(((x - ref) ** 2).mean()))  # noqa: E731
    new = device_vdenoise(A, B, S // 2, planes=("canva",))["canva"]
    old = tipe_rt.denoise(noisy, albedo, normal)
    print("%s, %d spp: RMSE noisy %.4f, variance-guided %.4f (ratio %.3f), a-trous %.4f (ratio %.3f)"
          % (scene, S, rmse(noisy), rmse(new), rmse(new) / rmse(noisy), rmse(old), rmse(old) / rmse(noisy)))
    return rmse(new) / rmse(noisy), rmse(old) / rmse(noisy)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "pyramid"])
def test_beats_the_a_trous_filter_on_a_noisy_frame(scene):
    """16 spp: ratio(new) <= ratio(a-trous filter at its defaults), margin 0."""
    new, old = ratios(scene, 16)
    assert new <= old


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["cornell", "pyramid"])
def test_does_not_harm_a_converged_frame(scene):
    """256 spp: ratio(new) < 1, the input itself as the yardstick."""
    new, _ = ratios(scene, 256)
    assert new < 1.0
