// rt_denoise_api.cpp — the denoiser's entry points of the C-ABI: the hook that
// rt_render_rows calls on a finished frame, the reference's pack/unpack, and
// the built-in edge-avoiding a-trous filter (rt_denoise.hip) on a device
// frame (rt_denoise_async), on host arrays (rt_denoise_host) and as a hook
// (rt_denoise_atrous).
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>

#include "rt_host_slots.h"

using namespace rt;

namespace {

constexpr rt_denoise_params kDefaults = {4, 1.0f, 0.5f, 0.25f};

std::atomic<rt_denoise_fn> g_denoise{nullptr};
std::mutex g_denoise_mu;
rt_denoise_params g_denoise_params = kDefaults;    // rt_denoise_atrous's

// frame size and parameters of the built-in denoiser
int validate_denoise(int W, int H, const rt_denoise_params* p)
{
    if (W < 1 || H < 1) return fail(RT_EINVAL, "denoise: frame %dx%d", W, H);
    if ((long long)W * H > (1ll << 30)) return fail(RT_EINVAL, "denoise: frame %dx%d above 2^30 pixels", W, H);
    if (!p) return fail(RT_EINVAL, "denoise: params is NULL");
    if (p->iterations < 1 || p->iterations > 8)
        return fail(RT_EINVAL, "denoise: iterations %d outside 1..8", p->iterations);
    const float sig[3] = {p->sigma_color, p->sigma_normal, p->sigma_albedo};
    const char* const name[3] = {"sigma_color", "sigma_normal", "sigma_albedo"};
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(sig[i])) return fail(RT_EINVAL, "denoise: %s is not finite", name[i]);
        if (sig[i] < 0x1p-8f || sig[i] > 0x1p8f)
            return fail(RT_EINVAL, "denoise: %s %g outside [2^-8, 2^8]", name[i], (double)sig[i]);
    }
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
    if (W < 1 || H < 1 || (long long)W * H > (1ll << 30)) return 0;
    return 4 * denoise_plane_floats((long long)W * H) * sizeof(float);
}

int rt_denoise_async(int W, int H, const rt_frame* frame, const rt_denoise_params* params, void* workspace,
                     size_t workspace_bytes, float* color3_out, void* hip_stream)
{
    const int rc = validate_denoise(W, H, params);
    if (rc) return rc;
    if (!frame || !frame->canva) return fail(RT_EINVAL, "denoise: canva is NULL");
    if (!workspace) return fail(RT_EINVAL, "denoise: workspace is NULL");
    if ((uintptr_t)workspace % 16) return fail(RT_EINVAL, "denoise: workspace is not 16-byte aligned");
    if (workspace_bytes < rt_denoise_workspace_bytes(W, H))
        return fail(RT_EINVAL, "denoise: workspace of %zu bytes, %dx%d needs %zu", workspace_bytes, W, H,
                    rt_denoise_workspace_bytes(W, H));
    const int e = launch_denoise(W, H, (double*)frame->canva, (const double*)frame->albedo,
                                 (const double*)frame->normal, params->iterations, params->sigma_color,
                                 params->sigma_normal, params->sigma_albedo, (float*)workspace, color3_out, hip_stream);
    if (e) return fail(RT_EDEVICE, "denoise launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

int rt_denoise_host(int W, int H, rt_color* canva, const rt_color* albedo, const rt_color* normal,
                    const rt_denoise_params* params)
{
    int rc, dev;
    if ((rc = validate_denoise(W, H, params))) return rc;
    if (!canva) return fail(RT_EINVAL, "denoise: canva is NULL");
    if ((rc = first_device(dev))) return rc;
    StreamLease ps;                  // drained on every return: the caller reads canva next
    if ((rc = ps.acquire(dev, true))) return rc;
    DeviceGuard g(dev);
    const size_t plane = (size_t)W * H * sizeof(rt_color), ws_bytes = rt_denoise_workspace_bytes(W, H);
    const rt_color* src[3] = {canva, albedo, normal};
    StreamBuffer dbuf;               // device: the workspace, then the given planes
    hipError_t e = ps->reserve_host(3 * plane);
    if (e == hipSuccess) e = dbuf.alloc(ws_bytes + 3 * plane, ps->st, dev);
    if (e != hipSuccess) return fail(RT_ENOMEM, "denoise buffers: %s", hipGetErrorString(e));
    char* buf = (char*)dbuf.p;
    rt_frame fr = {nullptr, nullptr, nullptr, nullptr};
    rt_color** dst[3] = {&fr.canva, &fr.albedo, &fr.normal};
    for (int pl = 0; pl < 3 && e == hipSuccess; ++pl) {
        if (!src[pl]) continue;
        char* host = (char*)ps->host + pl * plane;
        std::memcpy(host, src[pl], plane);
        *dst[pl] = (rt_color*)(buf + ws_bytes + pl * plane);
        e = hipMemcpyAsync(*dst[pl], host, plane, hipMemcpyHostToDevice, ps->st);
    }
    if (e != hipSuccess) return fail(RT_EDEVICE, "denoise upload: %s", hipGetErrorString(e));
    if ((rc = rt_denoise_async(W, H, &fr, params, buf, ws_bytes, nullptr, ps->st))) return rc;
    e = hipMemcpyAsync(ps->host, fr.canva, plane, hipMemcpyDeviceToHost, ps->st);
    if (e == hipSuccess) e = hipStreamSynchronize(ps->st);
    if (e != hipSuccess) return fail(RT_EDEVICE, "denoise: %s", hipGetErrorString(e));
    std::memcpy(canva, ps->host, plane);
    return RT_OK;
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

}  // extern "C"
