"""tipe_rt — Python mirror of the C-ABI in include/rt/rt.h (librt_hip.so).

Thin ctypes plumbing for tests and bench.py; the product is the C-ABI
library.  Loading fails loudly when librt_hip.so is missing: there is no CPU
fallback on the product path.
"""
import ctypes as C
import os

import numpy as np

from .types import (Vec3, Ray, Material, Sphere, UV, Triangle, Camera, ThreadData, Scene,  # noqa: F401
                    Params, Tiling, Frame, DenoiseParams, VDenoiseParams, AdaptiveParams, RT_OK, RT_EINVAL, RT_EDEVICE, RT_ENOMEM, RT_EUNSUPPORTED,
                    RT_RNG_PHILOX, RT_RNG_GLIBC, RT_NCOUNTERS, COUNTER_NAMES, RT_SPP_CHUNKS_AUTO,
                    RT_SPP_CHUNKS_DEFAULT)

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("RT_HIP_LIB") or os.path.join(PKG_DIR, "librt_hip.so")   # override: A/B builds
HOST_LIB_PATH = os.path.join(PKG_DIR, "librt_host.so")


class RTError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rt error %d: %s" % (code, msg))
        self.code = code


_lib = None
_host = None

# rt_denoise_fn (rt.h): denoiser()'s signature, denoiser.h:31
DENOISE_FN = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_void_p, Camera, C.c_void_p, C.c_void_p)
_hook_ref = None

_P = C.POINTER
_int, _ll, _ull, _ptr, _size, _str = C.c_int, C.c_longlong, C.c_ulonglong, C.c_void_p, C.c_size_t, C.c_char_p
_SC, _PA, _TI, _FR, _DP, _VP, _AP = (_P(t) for t in (Scene, Params, Tiling, Frame, DenoiseParams, VDenoiseParams,
                                                     AdaptiveParams))
_ASSEMBLE = [_ptr, _ll, _int, _int, _int, _int, _int, _ptr, _ptr]

# Every function include/rt/rt.h declares: name -> (restype, argtypes), in the
# header's order.  Device and host arrays and streams go over as void pointers.
# tests/test_abi.py holds the names and the argument counts against the header.
PROTOTYPES = {
    "rt_params_init": (None, [_PA]),
    "rt_init": (_int, [_int, _P(_int)]),
    "rt_shutdown": (None, []),
    "rt_last_error": (_str, []),
    "rt_abi_version": (_int, []),
    "rt_last_render_kernel": (_str, []),
    "rt_last_list_kernel": (_str, []),
    "rt_version": (_str, []),
    "rt_device_count": (_int, []),
    "rt_render_rows": (_int, [_SC, _PA, _int, _int, _ptr, _ptr, _ptr]),
    "rt_fill_canva": (_ptr, [_ptr]),
    "rt_set_fill_spp_chunks": (_int, [_int]),
    "rt_set_fill_precision": (_int, [_int]),
    "rt_scene_cache_clear": (_int, []),
    "rt_scene_upload": (_int, [_int, _SC, _P(_ptr)]),
    "rt_scene_release": (None, [_ptr]),
    "rt_render_async": (_int, [_ptr, _PA, _TI, _FR, _ptr]),
    "rt_assemble_async": (_int, _ASSEMBLE),
    "rt_gather_async": (_int, [_int, _P(_int), _P(_ptr), _int, _int, _int, _int, _int, _ptr, _ptr]),
    "rt_render_gather_async": (_int, [_SC, _PA, _int, _FR, _ptr]),
    "rt_last_gather_transport": (_str, []),
    "rt_peer_access": (_int, [_int, _int]),
    "rt_canva_pack_async": (_int, [_ll, _ptr, _ptr, _ptr]),
    "rt_canva_unpack_async": (_int, [_ll, _ptr, _ptr, _ptr]),
    "rt_canva_unpack_host": (_int, [_ll, _ptr, _ptr]),
    "rt_assemble_packed_async": (_int, _ASSEMBLE),
    "rt_set_fill_packed_canva": (_int, [_int]),
    "rt_count_async": (_int, [_ptr, _PA, _TI, _ptr, _ptr]),
    "rt_accumulate_async": (_int, [_ptr, _PA, _ll, _TI, _ptr, _ptr]),
    "rt_resolve_async": (_int, [_ptr, _PA, _int, _TI, _FR, _ptr]),
    "rt_set_zero_throughput_exit": (_int, [_int]),
    "rt_set_accumulate_queue": (_int, [_int]),
    "rt_set_denoise_hook": (None, [DENOISE_FN]),
    "rt_get_denoise_hook": (_ptr, []),
    "rt_denoise_pack": (_int, [_int, _int] + [_ptr] * 6),
    "rt_denoise_unpack": (_int, [_int, _int, _ptr, _ptr]),
    "rt_denoise_pack_async": (_int, [_int, _int, _FR] + [_ptr] * 4),
    "rt_denoise_params_init": (None, [_DP]),
    "rt_denoise_workspace_bytes": (_size, [_int, _int]),
    "rt_denoise_async": (_int, [_int, _int, _FR, _DP, _ptr, _size, _ptr, _ptr]),
    "rt_denoise_host": (_int, [_int, _int, _ptr, _ptr, _ptr, _DP]),
    "rt_denoise_atrous": (None, [_int, _int, _ptr, Camera, _ptr, _ptr]),
    "rt_set_denoise_params": (_int, [_DP]),
    "rt_vdenoise_params_init": (None, [_VP]),
    "rt_vdenoise_workspace_bytes": (_size, [_int, _int]),
    "rt_vdenoise_async": (_int, [_int, _int, _ptr, _ptr, _int, _VP, _ptr, _size, _FR, _ptr]),
    "rt_render_vdenoised": (_int, [_SC, _PA, _VP, _ptr, _ptr, _ptr]),
    "rt_accumulate_list_async": (_int, [_ptr, _PA, _ll, _ptr, _ptr, C.c_uint, _ptr, _ptr]),
    "rt_adaptive_select_async": (_int, [_int, _int, _ptr, _ptr, _int, C.c_float, _int, _ptr, _ptr, _ptr, _ptr, _size, _ptr]),
    "rt_adaptive_workspace_bytes": (_size, [_int, _int]),
    "rt_adaptive_params_init": (None, [_AP]),
    "rt_adaptive_async": (_int, [_ptr, _PA, _AP, _ptr, _ptr, _ptr, _ptr, _size, _FR, _ptr]),
    "rt_resolve_adaptive_async": (_int, [_int, _int, _ptr, _ptr, _ptr, _int, _FR, _ptr]),
    "rt_render_adaptive": (_int, [_SC, _PA, _AP, _ptr, _ptr, _ptr, _ptr]),
    "rt_vdenoise_adaptive_async": (_int, [_int, _int, _ptr, _ptr, _ptr, _int, _VP, _ptr, _size, _FR, _ptr]),
    "rt_render_adaptive_vdenoised": (_int, [_SC, _PA, _AP, _VP, _ptr, _ptr, _ptr, _ptr]),
    "rt_selftest_math": (_int, [_int, _ptr, _ptr, _int]),
    "rt_verify_sampler_phi": (_int, [_ull, _ull, _ptr]),
    "rt_verify_sphere_pass": (_int, [_SC, _ptr, _ll, _ptr]),
    "rt_verify_normalize": (_int, [_ull, _ull, _ptr]),
    "rt_verify_texel_map": (_int, [_SC, _ptr, _ptr, _ll, _ptr]),
}
EXPORTED_SYMBOLS = list(PROTOTYPES)


def lib():
    """librt_hip.so with prototypes.  Raises if it was not built."""
    global _lib
    if _lib is None:
        try:
            # Share torch's bundled HIP runtime (SONAME libamdhip64.so.7): if
            # librt_hip.so were loaded first it would pull /opt/rocm's copy
            # and the two runtimes would contend for the device.
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("librt_hip.so not built (%s): run `make -C tipe-raytracer_amd` "
                               "or __graft_entry__.build(); there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(L, name, None)      # an older build in an A/B run (RT_HIP_LIB) may lack the newer ones
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def _planes(params, albedo, normal):
    """Fresh (H, W, 3) float64 canva / albedo / normal (None where not asked
    for) and the pointers to pass: the data pointer, or None."""
    W, H = params.largeur_image, params.hauteur_image
    arrays = [np.zeros((H, W, 3)) if want else None for want in (True, albedo, normal)]
    return arrays, [None if a is None else a.ctypes.data for a in arrays]


def _with_overrides(p, init, values):
    """p after the library's init(p), with its fields, in their order, replaced by the values that are not None."""
    init(C.byref(p))
    for (name, _), v in zip(p._fields_, values):
        if v is not None:
            setattr(p, name, v)
    return p


def set_zero_throughput_exit(enable):
    """rt_set_zero_throughput_exit (rt.h): end paths whose rayColor is exactly
    0 where that is exact (default on; frames are identical either way, only
    the counted work differs).  Returns the previous setting."""
    return bool(lib().rt_set_zero_throughput_exit(1 if enable else 0))


def set_accumulate_queue(enable):
    """rt_set_accumulate_queue (rt.h): launches with running sums
    (accumulate_async, accumulate_list_async and what is built on them) take
    the task-queue kernel where a render launch would (default off; the sums
    are bit-identical either way).  Returns the previous setting."""
    return bool(lib().rt_set_accumulate_queue(1 if enable else 0))


def set_fill_packed_canva(enable):
    """rt_set_fill_packed_canva (rt.h): render_rows / rt_fill_canva bring the
    canva to the host at 4 bytes a pixel (default off; the arrays are
    bit-identical either way).  Returns the previous setting."""
    return bool(lib().rt_set_fill_packed_canva(1 if enable else 0))


def canva_pack_async(n, canva_ptr, packed_ptr, stream=None):
    """rt_canva_pack_async: n device colours -> n packed words (f0 | f1 << 9 | f2 << 18)."""
    check(lib().rt_canva_pack_async(n, canva_ptr, packed_ptr, stream))


def canva_unpack_async(n, packed_ptr, canva_ptr, stream=None):
    """rt_canva_unpack_async: n packed words -> n device colours."""
    check(lib().rt_canva_unpack_async(n, packed_ptr, canva_ptr, stream))


def canva_unpack_host(packed):
    """rt_canva_unpack_host: a uint32 array of packed pixels -> (..., 3) float64 colours, on the host."""
    w = np.ascontiguousarray(packed, dtype=np.uint32)
    out = np.zeros(w.shape + (3,))
    check(lib().rt_canva_unpack_host(w.size, w.ctypes.data, out.ctypes.data))
    return out


def assemble_packed_async(gathered_ptr, world, tile_rows, rows_per_rank, W, H, out_ptr, stream=None, rank_stride=0):
    """rt_assemble_packed_async: assemble_async on rank-major packed words (rank_stride in pixels)."""
    check(lib().rt_assemble_packed_async(gathered_ptr, rank_stride, world, tile_rows, rows_per_rank, W, H, out_ptr,
                                         stream))


def last_list_kernel():
    """rt_last_list_kernel: the render kernel this thread's last list launch used."""
    return lib().rt_last_list_kernel().decode()


class reference_counts:
    """Context manager: zero-throughput exit off, so rt_count_async counts
    what the reference's tracer does (the oracle's counters)."""
    def __enter__(self):
        self.prev = set_zero_throughput_exit(False)
        return self

    def __exit__(self, *exc):
        set_zero_throughput_exit(self.prev)
        return False


def set_denoise_hook(fn):
    """Install a Python callable fn(W, H, canva_ptr, cam, albedo_ptr,
    normal_ptr) as the rt_render_rows denoiser hook (None clears it)."""
    global _hook_ref
    _hook_ref = DENOISE_FN(fn) if fn is not None else DENOISE_FN()
    lib().rt_set_denoise_hook(_hook_ref)


def denoise_pack(canva, albedo=None, normal=None):
    """OIDN input planes (denoiser.h:44-60) from host (H, W, 3) frames."""
    H, W = canva.shape[:2]
    outs = [np.zeros((H, W, 3), np.float32) for _ in range(3)]
    ptr = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data  # noqa: E731
    keep = [np.ascontiguousarray(x) if x is not None else None for x in (canva, albedo, normal)]
    check(lib().rt_denoise_pack(W, H, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]),
                                outs[0].ctypes.data, outs[1].ctypes.data if albedo is not None else None,
                                outs[2].ctypes.data if normal is not None else None))
    return outs


def denoise_unpack(color3):
    """canva = (int)(color * 255.0f), denoiser.h:80-84."""
    H, W = color3.shape[:2]
    out = np.zeros((H, W, 3))
    c = np.ascontiguousarray(color3, dtype=np.float32)
    check(lib().rt_denoise_unpack(W, H, c.ctypes.data, out.ctypes.data))
    return out


def denoise_params(iterations=None, sigma_color=None, sigma_normal=None, sigma_albedo=None):
    """rt_denoise_params_init's defaults (4 passes; sigmas 1, 0.5, 0.25) with the given fields replaced."""
    return _with_overrides(DenoiseParams(), lib().rt_denoise_params_init,
                           (iterations, sigma_color, sigma_normal, sigma_albedo))


def denoise(canva, albedo=None, normal=None, params=None):
    """rt_denoise_host: the built-in a-trous denoiser (rt.h; not OIDN) on host
    (H, W, 3) float64 frames; returns the filtered canva, the inputs stay."""
    H, W = canva.shape[:2]
    out = np.array(canva, dtype=np.float64, order="C")
    keep = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (albedo, normal)]
    p = params if params is not None else denoise_params()
    check(lib().rt_denoise_host(W, H, out.ctypes.data, *[None if k is None else k.ctypes.data for k in keep],
                                C.byref(p)))
    return out


def denoise_async(W, H, canva_ptr, albedo_ptr, normal_ptr, params, workspace_ptr, workspace_bytes,
                  color3_ptr=None, stream=None):
    """rt_denoise_async on device pointers (canva is filtered in place)."""
    fr = Frame(canva_ptr, albedo_ptr, normal_ptr, None)
    check(lib().rt_denoise_async(W, H, C.byref(fr), C.byref(params), workspace_ptr, workspace_bytes, color3_ptr,
                                 stream))


def set_denoise_atrous(enable=True, params=None):
    """Install rt_denoise_atrous as the rt_render_rows hook (or clear the
    hook) and set its process-wide parameters (None: the defaults)."""
    global _hook_ref
    check(lib().rt_set_denoise_params(None if params is None else C.byref(params)))
    _hook_ref = C.cast(lib().rt_denoise_atrous, DENOISE_FN) if enable else DENOISE_FN()
    lib().rt_set_denoise_hook(_hook_ref)


def vdenoise_params(iterations=None, sigma_luminance=None, sigma_normal=None, sigma_albedo=None):
    """rt_vdenoise_params_init's defaults (4 passes; sigmas 4, 0.5, 0.25) with the given fields replaced."""
    return _with_overrides(VDenoiseParams(), lib().rt_vdenoise_params_init,
                           (iterations, sigma_luminance, sigma_normal, sigma_albedo))


def vdenoise_async(W, H, sums_a_ptr, sums_b_ptr, spp_half, params, workspace_ptr, workspace_bytes, canva_ptr,
                   albedo_ptr=None, normal_ptr=None, radiance_ptr=None, stream=None):
    """rt_vdenoise_async: the variance-guided denoiser (rt.h) on two device
    accumulators of spp_half samples each, into device planes."""
    fr = Frame(canva_ptr, albedo_ptr, normal_ptr, radiance_ptr)
    check(lib().rt_vdenoise_async(W, H, sums_a_ptr, sums_b_ptr, spp_half, C.byref(params), workspace_ptr,
                                  workspace_bytes, C.byref(fr), stream))


def render_vdenoised(scene, params, vparams=None, albedo=True, normal=True):
    """rt_render_vdenoised into fresh (H, W, 3) float64 arrays (canva, albedo,
    normal): the frame's two sample halves rendered and filtered on the device."""
    planes, ptrs = _planes(params, albedo, normal)
    vp = vparams if vparams is not None else vdenoise_params()
    check(lib().rt_render_vdenoised(C.byref(scene), C.byref(params), C.byref(vp), *ptrs))
    return tuple(planes)


def adaptive_params(first_half=None, max_rounds=None, tolerance=None):
    """rt_adaptive_params_init's defaults (8, 5, 1/64) with the given fields replaced."""
    return _with_overrides(AdaptiveParams(), lib().rt_adaptive_params_init, (first_half, max_rounds, tolerance))


def accumulate_list_async(dscene, params, sample_offset, list_ptr, count_ptr, list_cap, sums_ptr, stream=None):
    """rt_accumulate_list_async: add samples [offset, offset + S) of the listed pixels into d_sums."""
    check(lib().rt_accumulate_list_async(dscene.handle, C.byref(params), sample_offset, list_ptr, count_ptr, list_cap,
                                         sums_ptr, stream))


def adaptive_select_async(W, H, sums_a_ptr, sums_b_ptr, n_half, tolerance, round, list_ptr, count_ptr, rounds_ptr,
                          workspace_ptr, workspace_bytes, stream=None):
    """rt_adaptive_select_async: the settled test and the compaction of the pixels that go on."""
    check(lib().rt_adaptive_select_async(W, H, sums_a_ptr, sums_b_ptr, n_half, tolerance, round, list_ptr, count_ptr,
                                         rounds_ptr, workspace_ptr, workspace_bytes, stream))


def adaptive_async(dscene, params, aparams, sums_a_ptr, sums_b_ptr, rounds_ptr, workspace_ptr, workspace_bytes,
                   canva_ptr=None, albedo_ptr=None, normal_ptr=None, radiance_ptr=None, stream=None):
    """rt_adaptive_async: the adaptive loop on two device accumulators; the
    frame planes are resolved when canva_ptr is given."""
    fr = Frame(canva_ptr, albedo_ptr, normal_ptr, radiance_ptr) if canva_ptr else None
    check(lib().rt_adaptive_async(dscene.handle, C.byref(params), C.byref(aparams), sums_a_ptr, sums_b_ptr,
                                  rounds_ptr, workspace_ptr, workspace_bytes, C.byref(fr) if fr else None, stream))


def resolve_adaptive_async(W, H, sums_a_ptr, sums_b_ptr, rounds_ptr, first_half, canva_ptr, albedo_ptr=None,
                           normal_ptr=None, radiance_ptr=None, stream=None):
    """rt_resolve_adaptive_async: the frame planes of A + B with each pixel's own sample count."""
    fr = Frame(canva_ptr, albedo_ptr, normal_ptr, radiance_ptr)
    check(lib().rt_resolve_adaptive_async(W, H, sums_a_ptr, sums_b_ptr, rounds_ptr, first_half, C.byref(fr), stream))


def render_adaptive(scene, params, aparams=None, albedo=True, normal=True):
    """rt_render_adaptive into fresh arrays: (canva, albedo, normal, rounds),
    three (H, W, 3) float64 planes and the (H, W) int32 round counts."""
    planes, ptrs = _planes(params, albedo, normal)
    rounds = np.zeros(planes[0].shape[:2], dtype=np.int32)
    ap = aparams if aparams is not None else adaptive_params()
    check(lib().rt_render_adaptive(C.byref(scene), C.byref(params), C.byref(ap), *ptrs, rounds.ctypes.data))
    return (*planes, rounds)


def vdenoise_adaptive_async(W, H, sums_a_ptr, sums_b_ptr, rounds_ptr, first_half, params, workspace_ptr,
                            workspace_bytes, canva_ptr, albedo_ptr=None, normal_ptr=None, radiance_ptr=None,
                            stream=None):
    """rt_vdenoise_adaptive_async: the variance-guided denoiser on an adaptive
    result, pixel p holding first_half * 2^(rounds[p] - 1) samples per accumulator."""
    fr = Frame(canva_ptr, albedo_ptr, normal_ptr, radiance_ptr)
    check(lib().rt_vdenoise_adaptive_async(W, H, sums_a_ptr, sums_b_ptr, rounds_ptr, first_half, C.byref(params),
                                           workspace_ptr, workspace_bytes, C.byref(fr), stream))


def render_adaptive_vdenoised(scene, params, aparams=None, vparams=None, albedo=True, normal=True):
    """rt_render_adaptive_vdenoised into fresh arrays: (canva, albedo, normal,
    rounds) as render_adaptive's, the planes filtered by the variance-guided denoiser."""
    planes, ptrs = _planes(params, albedo, normal)
    rounds = np.zeros(planes[0].shape[:2], dtype=np.int32)
    ap = aparams if aparams is not None else adaptive_params()
    vp = vparams if vparams is not None else vdenoise_params()
    check(lib().rt_render_adaptive_vdenoised(C.byref(scene), C.byref(params), C.byref(ap), C.byref(vp), *ptrs,
                                             rounds.ctypes.data))
    return (*planes, rounds)


def last_gather_transport():
    """rt_last_gather_transport(): the transport the thread's last rt_render_gather_async used."""
    return lib().rt_last_gather_transport().decode()


def last_render_kernel():
    """rt_last_render_kernel: the render kernel this thread's last launch used."""
    return lib().rt_last_render_kernel().decode()


def check(rc):
    if rc != RT_OK:
        raise RTError(rc, lib().rt_last_error().decode())
    return rc


def host():
    """librt_host.so (C host library: camera, OBJ/MTL/PPM IO)."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise RuntimeError("librt_host.so not built (%s)" % HOST_LIB_PATH)
        H = C.CDLL(HOST_LIB_PATH)
        H.rt_host_init_camera.argtypes = [Vec3, Vec3, Vec3, C.c_double, C.c_double]
        H.rt_host_init_camera.restype = Camera
        _host = H
    return _host


def init_camera(origin, target, up, vfov, ratio):
    """init_camera (camera.h:21-40) via the C host library."""
    return host().rt_host_init_camera(Vec3(*origin), Vec3(*target), Vec3(*up), float(vfov), float(ratio))


def make_scene(spheres=None, triangles=None, quel_mat=None, mat_list=None, tex_width=0, tex_height=0,
               n_materials=0, sky=None):
    """rt_scene over ctypes arrays; sky = (texels, width, height) or None."""
    sc = Scene()
    keep = []
    if sky is not None:
        sc.sky_mat_list = C.cast(sky[0], C.POINTER(Material))
        sc.sky_width, sc.sky_height = sky[1], sky[2]
        keep.append(sky[0])
    if spheres is not None and len(spheres):
        sc.sphere_list = C.cast(spheres, C.POINTER(Sphere))
        sc.nbSpheres = len(spheres)
        keep.append(spheres)
    if triangles is not None and len(triangles):
        sc.triangle_list = C.cast(triangles, C.POINTER(Triangle))
        sc.nbTriangles = len(triangles)
        sc.quelMatPourTri = C.cast(quel_mat, C.POINTER(C.c_int))
        sc.mat_list = C.cast(mat_list, C.POINTER(Material))
        sc.tex_width, sc.tex_height, sc.nbMaterials = tex_width, tex_height, n_materials
        keep += [triangles, quel_mat, mat_list]
    sc._keep = keep
    return sc


def make_params(W, H, spp, bounces, cam, focus=3.0, aperture=(0.0, 0.0), use_ao=False, ao=2.5,
                seed=1010, rng=RT_RNG_PHILOX, compat=1, chunks=1, accel=0, sky_mode=0, semantics=0,
                precision=0, gather=0):
    p = Params()
    p.largeur_image, p.hauteur_image = W, H
    p.nbRayonParPixel, p.nbRebondMax = spp, bounces
    p.cam = cam
    p.focus_distance = focus
    p.ouverture_x, p.ouverture_y = aperture
    p.useAO, p.AO_intensity = int(bool(use_ao)), ao
    p.compat_int_truncation = compat
    p.rng, p.seed = rng, seed
    p.spp_chunks = chunks
    p.accel = accel
    p.sky_mode = sky_mode
    p.semantics = semantics
    p.precision = precision
    p.gather = gather
    return p


def render_rows(scene, params, row_hi=None, row_lo=0, albedo=True, normal=True):
    """rt_render_rows into fresh (H, W, 3) float64 arrays (canva, albedo, normal)."""
    if row_hi is None:
        row_hi = params.hauteur_image - 1
    planes, ptrs = _planes(params, albedo, normal)
    check(lib().rt_render_rows(C.byref(scene), C.byref(params), row_hi, row_lo, *ptrs))
    return tuple(planes)


class DeviceScene:
    """rt_scene_upload handle (released on close / garbage collection)."""

    def __init__(self, scene, device=0):
        self.handle = C.c_void_p()
        check(lib().rt_scene_upload(device, C.byref(scene), C.byref(self.handle)))
        self.device = device

    def close(self):
        if self.handle:
            lib().rt_scene_release(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cyclic_tiling(H, tile_rows, rank, world):
    """Rank `rank` of `world` with cyclic `tile_rows`-row tiles (rt.h rt_tiling)."""
    n_tiles_total = (H + tile_rows - 1) // tile_rows
    per_rank = (n_tiles_total + world - 1) // world
    return Tiling(0, tile_rows, rank, world, per_rank)


def band_tiling(row_lo, row_hi):
    return Tiling(row_lo, row_hi - row_lo + 1, 0, 1, 1)


def render_async(dscene, params, tiling, canva_ptr, albedo_ptr=None, normal_ptr=None, radiance_ptr=None,
                 stream=None):
    fr = Frame(canva_ptr, albedo_ptr, normal_ptr, radiance_ptr)
    check(lib().rt_render_async(dscene.handle, C.byref(params), C.byref(tiling), C.byref(fr), stream))


def accumulate_async(dscene, params, sample_offset, tiling, sums_ptr, stream=None):
    """rt_accumulate_async: add samples [offset, offset + S) into d_sums."""
    check(lib().rt_accumulate_async(dscene.handle, C.byref(params), sample_offset, C.byref(tiling), sums_ptr,
                                    stream))


def resolve_async(sums_ptr, params, total_spp, tiling, canva_ptr, albedo_ptr=None, normal_ptr=None,
                  radiance_ptr=None, stream=None):
    """rt_resolve_async: frame planes of the running sums for total_spp."""
    fr = Frame(canva_ptr, albedo_ptr, normal_ptr, radiance_ptr)
    check(lib().rt_resolve_async(sums_ptr, C.byref(params), total_spp, C.byref(tiling), C.byref(fr), stream))


def count_async(dscene, params, tiling, counters_ptr, stream=None):
    check(lib().rt_count_async(dscene.handle, C.byref(params), C.byref(tiling), counters_ptr, stream))


def assemble_async(gathered_ptr, world, tile_rows, rows_per_rank, W, H, out_ptr, stream=None, rank_stride=0):
    check(lib().rt_assemble_async(gathered_ptr, rank_stride, world, tile_rows, rows_per_rank, W, H, out_ptr,
                                  stream))


def gather_async(src_devices, local_ptrs, tile_rows, rows_per_rank, W, H, dst_device, out_ptr, stream=None):
    """rt_gather_async: slot r's local plane (device src_devices[r]) -> out on
    dst_device over peer copies, un-permuted into row order."""
    n = len(src_devices)
    devs = (C.c_int * n)(*src_devices)
    locs = (C.c_void_p * n)(*local_ptrs)
    check(lib().rt_gather_async(n, devs, locs, tile_rows, rows_per_rank, W, H, dst_device, out_ptr, stream))


def render_gather_async(scene, params, tile_rows, canva_ptr, albedo_ptr=None, normal_ptr=None, radiance_ptr=None,
                        stream=None):
    """rt_render_gather_async: every device of rt_init's list renders its
    cyclic tiles; the planes are gathered into the first device's frame."""
    fr = Frame(canva_ptr, albedo_ptr, normal_ptr, radiance_ptr)
    check(lib().rt_render_gather_async(C.byref(scene), C.byref(params), tile_rows, C.byref(fr), stream))


def verify_sampler_phi(r0=0, n=1 << 31):
    """(fallbacks, mismatches) of the fast phi path over rand() values [r0, r0 + n)."""
    out = (C.c_ulonglong * 2)()
    check(lib().rt_verify_sampler_phi(r0, n, out))
    return int(out[0]), int(out[1])


def verify_normalize(seed=1, n=1 << 30):
    """(fast-path vectors, mismatches) of the kernel's normalize against IEEE
    a / sqrt(a.a) on n pseudo-random vectors (rt_verify_normalize)."""
    out = (C.c_ulonglong * 2)()
    check(lib().rt_verify_normalize(seed, n, out))
    return int(out[0]), int(out[1])


def verify_texel_map(scene, pts, tri):
    """(fast-path points, mismatches) of the texel lookup's affine fast path
    against the reference's barycentric path: pts (n, 3) float64 hit points,
    tri (n,) their triangles (rt_verify_texel_map)."""
    p = np.ascontiguousarray(pts, dtype=np.float64)
    t = np.ascontiguousarray(tri, dtype=np.int32)
    out = (C.c_ulonglong * 2)()
    check(lib().rt_verify_texel_map(C.byref(scene), p.ctypes.data, t.ctypes.data, len(p), out))
    return int(out[0]), int(out[1])


def verify_sphere_pass(scene, rays):
    """(fallbacks, mismatches) of the sphere candidate pass on rays (n, 6) float64."""
    r = np.ascontiguousarray(rays, dtype=np.float64)
    out = (C.c_ulonglong * 2)()
    check(lib().rt_verify_sphere_pass(C.byref(scene), r.ctypes.data, len(r), out))
    return int(out[0]), int(out[1])


def selftest_math(op, inputs, n):
    inp = np.ascontiguousarray(inputs, dtype=np.float64)
    out = np.zeros(n * (4 if op == 7 else 3 if op == 8 else 1))
    check(lib().rt_selftest_math(op, inp.ctypes.data, out.ctypes.data, n))
    return out
