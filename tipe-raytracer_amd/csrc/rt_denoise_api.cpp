// rt_denoise_api.cpp — the denoiser's entry points of the C-ABI: the hook that
// rt_render_rows calls on a finished frame, the reference's pack/unpack, and
// the built-in edge-avoiding a-trous filter (rt_denoise.hip) on a device
// frame (rt_denoise_async), on host arrays (rt_denoise_host) and as a hook
// (rt_denoise_atrous); and the variance-guided denoiser (rt_vdenoise.hip) on
// two device accumulators (rt_vdenoise_async; rt_vdenoise_adaptive_async with
// each pixel's own sample count) and as a whole-frame render into host arrays
// (rt_render_vdenoised).
#include <atomic>
#include <cmath>
#include <mutex>

#include "rt_host_slots.h"

using namespace rt;

namespace {

constexpr rt_denoise_params kDefaults = {4, 1.0f, 0.5f, 0.25f};

std::atomic<rt_denoise_fn> g_denoise{nullptr};
std::mutex g_denoise_mu;
rt_denoise_params g_denoise_params = kDefaults;    // rt_denoise_atrous's

// what the two denoisers validate alike behind the frame size: the pass count and the three sigmas
int validate_passes(int iterations, int min_iterations, const float* sig, const char* const* name)
{
    if (iterations < min_iterations || iterations > 8)
        return fail(RT_EINVAL, "denoise: iterations %d outside %d..8", iterations, min_iterations);
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(sig[i])) return fail(RT_EINVAL, "denoise: %s is not finite", name[i]);
        if (sig[i] < 0x1p-8f || sig[i] > 0x1p8f)
            return fail(RT_EINVAL, "denoise: %s %g outside [2^-8, 2^8]", name[i], (double)sig[i]);
    }
    return RT_OK;
}

// frame size and parameters of the built-in denoiser
int validate_denoise(int W, int H, const rt_denoise_params* p)
{
    const int rc = validate_frame_size("denoise", W, H);
    if (rc) return rc;
    if (!p) return fail(RT_EINVAL, "denoise: params is NULL");
    const float sig[3] = {p->sigma_color, p->sigma_normal, p->sigma_albedo};
    const char* const name[3] = {"sigma_color", "sigma_normal", "sigma_albedo"};
    return validate_passes(p->iterations, 1, sig, name);
}

constexpr rt_vdenoise_params kVDefaults = {4, 4.0f, 0.5f, 0.25f};

}  // namespace

// ... and of the variance-guided one (rt_adaptive_api.cpp validates with it too)
int rt::validate_vdenoise(int W, int H, const rt_vdenoise_params* p)
{
    const int rc = validate_frame_size("denoise", W, H);
    if (rc) return rc;
    if (!p) return fail(RT_EINVAL, "vdenoise: params is NULL");
    const float sig[3] = {p->sigma_luminance, p->sigma_normal, p->sigma_albedo};
    const char* const name[3] = {"sigma_luminance", "sigma_normal", "sigma_albedo"};
    return validate_passes(p->iterations, 0, sig, name);
}

namespace {

// rt_vdenoise_async (rounds null, n = spp_half) and rt_vdenoise_adaptive_async (n = first_half): what both
// refuse, then the launches
int vdenoise_on_stream(int W, int H, const double* d_sums_a, const double* d_sums_b, const int* d_rounds, int n,
                       const char* n_name, const rt_vdenoise_params* params, void* workspace, size_t workspace_bytes,
                       const rt_frame* out, void* hip_stream)
{
    int rc = validate_vdenoise(W, H, params);
    if (rc) return rc;
    if (!d_sums_a || !d_sums_b) return fail(RT_EINVAL, "vdenoise: an accumulator is NULL");
    if (n < 1) return fail(RT_EINVAL, "vdenoise: %s %d < 1", n_name, n);
    if (!out || !out->canva) return fail(RT_EINVAL, "vdenoise: out.canva is NULL");
    if ((rc = validate_workspace("vdenoise", W, H, workspace, workspace_bytes, rt_vdenoise_workspace_bytes(W, H))))
        return rc;
    const int e = launch_vdenoise(W, H, d_sums_a, d_sums_b, d_rounds, n, params->iterations, params->sigma_luminance,
                                  params->sigma_normal, params->sigma_albedo, (float*)workspace, (double*)out->canva,
                                  (double*)out->albedo, (double*)out->normal, (double*)out->radiance, hip_stream);
    if (e) return fail(RT_EDEVICE, "vdenoise launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

}  // namespace

extern "C" {

void rt_set_denoise_hook(rt_denoise_fn fn) { g_denoise.store(fn); }
rt_denoise_fn rt_get_denoise_hook(void) { return g_denoise.load(); }

int rt_denoise_pack(int W, int H, const rt_color* canva, const rt_color* albedo, const rt_color* normal,
                    float* color3, float* albedo3, float* normal3)
{
    if (W < 1 || H < 1 || !canva || !color3) return fail(RT_EINVAL, "bad denoise_pack arguments");
    const size_t n = (size_t)W * H;
    for (size_t i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) {
            color3[3 * i + c] = (float)canva[i].e[c] / 255.0f;          // denoiser.h:44-48
            if (albedo && albedo3) albedo3[3 * i + c] = (float)albedo[i].e[c];
            if (normal && normal3) normal3[3 * i + c] = (float)normal[i].e[c];
        }
    return RT_OK;
}

int rt_denoise_unpack(int W, int H, const float* color3, rt_color* canva)
{
    if (W < 1 || H < 1 || !canva || !color3) return fail(RT_EINVAL, "bad denoise_unpack arguments");
    const size_t n = (size_t)W * H;
    for (size_t i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) canva[i].e[c] = (int)(color3[3 * i + c] * 255.0f);   // denoiser.h:80-84
    return RT_OK;
}

int rt_denoise_pack_async(int W, int H, const rt_frame* frame, float* color3, float* albedo3, float* normal3,
                          void* hip_stream)
{
    if (W < 1 || H < 1 || !frame || !frame->canva || !color3)
        return fail(RT_EINVAL, "bad denoise_pack_async arguments");
    const int e = launch_denoise_pack((long long)W * H, (const double*)frame->canva,
                                      albedo3 ? (const double*)frame->albedo : nullptr,
                                      normal3 ? (const double*)frame->normal : nullptr, color3, albedo3, normal3,
                                      hip_stream);
    if (e) return fail(RT_EDEVICE, "denoise pack launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

void rt_denoise_params_init(rt_denoise_params* p)
{
    if (p) *p = kDefaults;
}

size_t rt_denoise_workspace_bytes(int W, int H)
{
    if (!frame_size_ok(W, H)) return 0;
    return 4 * denoise_plane_floats((long long)W * H) * sizeof(float);
}

int rt_denoise_async(int W, int H, const rt_frame* frame, const rt_denoise_params* params, void* workspace,
                     size_t workspace_bytes, float* color3_out, void* hip_stream)
{
    int rc = validate_denoise(W, H, params);
    if (rc) return rc;
    if (!frame || !frame->canva) return fail(RT_EINVAL, "denoise: canva is NULL");
    if ((rc = validate_workspace("denoise", W, H, workspace, workspace_bytes, rt_denoise_workspace_bytes(W, H))))
        return rc;
    const int e = launch_denoise(W, H, (double*)frame->canva, (const double*)frame->albedo,
                                 (const double*)frame->normal, params->iterations, params->sigma_color,
                                 params->sigma_normal, params->sigma_albedo, (float*)workspace, color3_out, hip_stream);
    if (e) return fail(RT_EDEVICE, "denoise launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

int rt_denoise_host(int W, int H, rt_color* canva, const rt_color* albedo, const rt_color* normal,
                    const rt_denoise_params* params)
{
    int rc;
    if ((rc = validate_denoise(W, H, params))) return rc;
    if (!canva) return fail(RT_EINVAL, "denoise: canva is NULL");
    const size_t npx = (size_t)W * H, plane = npx * sizeof(rt_color), ws_bytes = rt_denoise_workspace_bytes(W, H);
    HostFrameJob job;
    if ((rc = job.open("denoise", nullptr, 3 * plane, ws_bytes + 3 * plane))) return rc;
    char* ws = job.take(ws_bytes);
    rt_color* planes = (rt_color*)job.take(3 * plane);
    const rt_frame fr = {planes, albedo ? planes + npx : nullptr, normal ? planes + 2 * npx : nullptr, nullptr};
    const rt_color* src[3] = {canva, albedo, normal};
    rt_color* const dst[3] = {fr.canva, fr.albedo, fr.normal};
    for (int pl = 0; pl < 3; ++pl)
        if (src[pl] && (rc = job.upload(dst[pl], src[pl], plane))) return rc;
    if ((rc = rt_denoise_async(W, H, &fr, params, ws, ws_bytes, nullptr, job.stream()))) return rc;
    return job.finish({{canva, fr.canva, plane}});
}

int rt_set_denoise_params(const rt_denoise_params* params)
{
    const int rc = params ? validate_denoise(1, 1, params) : RT_OK;
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_denoise_mu);
    g_denoise_params = params ? *params : kDefaults;
    return RT_OK;
}

void rt_denoise_atrous(int largeur_image, int hauteur_image, rt_color* canva, rt_camera cam, rt_color* albedo,
                       rt_color* normal)
{
    (void)cam;
    rt_denoise_params p;
    {
        std::lock_guard<std::mutex> lk(g_denoise_mu);
        p = g_denoise_params;
    }
    (void)rt_denoise_host(largeur_image, hauteur_image, canva, albedo, normal, &p);
}

void rt_vdenoise_params_init(rt_vdenoise_params* p)
{
    if (p) *p = kVDefaults;
}

size_t rt_vdenoise_workspace_bytes(int W, int H)
{
    if (!frame_size_ok(W, H)) return 0;
    const long long npx = (long long)W * H;
    return (4 * denoise_plane_floats(npx) + 3 * vdenoise_scalar_floats(npx)) * sizeof(float);
}

int rt_vdenoise_async(int W, int H, const double* d_sums_a, const double* d_sums_b, int spp_half,
                      const rt_vdenoise_params* params, void* workspace, size_t workspace_bytes, const rt_frame* out,
                      void* hip_stream)
{
    return vdenoise_on_stream(W, H, d_sums_a, d_sums_b, nullptr, spp_half, "spp_half", params, workspace,
                              workspace_bytes, out, hip_stream);
}

int rt_vdenoise_adaptive_async(int W, int H, const double* d_sums_a, const double* d_sums_b, const int* d_rounds,
                               int first_half, const rt_vdenoise_params* params, void* workspace,
                               size_t workspace_bytes, const rt_frame* out, void* hip_stream)
{
    if (!d_rounds) return fail(RT_EINVAL, "vdenoise: d_rounds is NULL");
    return vdenoise_on_stream(W, H, d_sums_a, d_sums_b, d_rounds, first_half, "first_half", params, workspace,
                              workspace_bytes, out, hip_stream);
}

int rt_render_vdenoised(const rt_scene* scene, const rt_params* params, const rt_vdenoise_params* vparams,
                        rt_color* canva, rt_color* albedo, rt_color* normal)
{
    int rc;
    if ((rc = validate_scene(scene)) || (rc = validate_params(params))) return rc;
    const int W = params->largeur_image, H = params->hauteur_image, S = params->nbRayonParPixel;
    if ((rc = validate_vdenoise(W, H, vparams))) return rc;
    if (!canva) return fail(RT_EINVAL, "vdenoise: canva is NULL");
    if (S < 2 || S % 2) return fail(RT_EINVAL, "vdenoise: nbRayonParPixel %d is not even and >= 2", S);
    const size_t npx = (size_t)W * H, plane = npx * sizeof(rt_color), sums = npx * 9 * sizeof(double);
    const size_t ws_bytes = rt_vdenoise_workspace_bytes(W, H);
    HostFrameJob job;
    if ((rc = job.open("vdenoise", scene, 3 * plane, 2 * sums + ws_bytes + 3 * plane))) return rc;
    char* acc = job.take(2 * sums);                      // the two accumulators, back to back
    char* ws = job.take(ws_bytes);
    rt_color* planes = (rt_color*)job.take(3 * plane);
    const hipError_t e = hipMemsetAsync(acc, 0, 2 * sums, job.stream());
    if (e != hipSuccess) return fail(RT_EDEVICE, "vdenoise clear: %s", hipGetErrorString(e));
    rt_params half = *params;
    half.nbRayonParPixel = S / 2;
    const rt_tiling whole = {0, H, 0, 1, 1};
    for (int k = 0; k < 2; ++k)
        if ((rc = rt_accumulate_async(job.scene(), &half, (long long)k * (S / 2), &whole, (double*)(acc + k * sums),
                                      job.stream())))
            return rc;
    const rt_frame fr = {planes, albedo ? planes + npx : nullptr, normal ? planes + 2 * npx : nullptr, nullptr};
    if ((rc = rt_vdenoise_async(W, H, (double*)acc, (double*)(acc + sums), S / 2, vparams, ws, ws_bytes, &fr,
                                job.stream())))
        return rc;
    return job.finish({{canva, planes, plane}, {albedo, planes + npx, plane}, {normal, planes + 2 * npx, plane}});
}

}  // extern "C"
