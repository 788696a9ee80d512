// rt_api.cpp — C-ABI of librt_hip.so (include/rt/rt.h): validation, init,
// scene upload into the HBM layout of rt_internal.h (prepared on the host by
// rt_scene_prep.cpp), launches (plan: rt_launch_plan.cpp; scratch: LaunchScratch),
// the refusals that several files share and the single-device async entry points.
// The host-buffer drop-ins are in rt_drop_in.cpp, the multi-device gather in
// rt_gather.cpp, the denoisers' entry points in rt_denoise_api.cpp, adaptive
// sampling's in rt_adaptive_api.cpp, the diagnostics in rt_diag.cpp.
// Every HIP call is checked; failures return RT_E* and set rt_last_error().
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "rt_api_internal.h"
#include "rt_rccl.h"

namespace rt {

namespace {

thread_local std::string g_err;

std::mutex g_mu;
std::vector<int> g_devices;
bool g_inited = false;

std::atomic<int> g_zero_exit{1};
std::atomic<int> g_acc_queue{0};     // rt_set_accumulate_queue

int validate_tiling(const rt_tiling* t)
{
    if (!t) return fail(RT_EINVAL, "tiling is NULL");
    if (t->tile_rows < 1 || t->tile_step < 1 || t->tile_first < 0 || t->n_tiles < 0 || t->row_base < 0)
        return fail(RT_EINVAL, "bad tiling {%d,%d,%d,%d,%d}", t->row_base, t->tile_rows, t->tile_first,
                    t->tile_step, t->n_tiles);
    if ((long long)t->n_tiles * t->tile_rows > (1ll << 30)) return fail(RT_EINVAL, "tiling too large");
    return RT_OK;
}

void set_frame(KParams& kp, const rt_frame* frame)
{
    kp.canva = (double*)frame->canva;
    kp.albedo = (double*)frame->albedo;
    kp.normal = (double*)frame->normal;
    kp.radiance = (double*)frame->radiance;
}

}  // namespace

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int device_list(std::vector<int>& devs)
{
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_inited) {
        int n = 0;
        HIP_TRY(hipGetDeviceCount(&n));
        if (n < 1) return fail(RT_EDEVICE, "no HIP device");
        g_devices.assign(1, 0);
        g_inited = true;
    }
    devs = g_devices;
    return RT_OK;
}

int first_device(int& dev)
{
    std::vector<int> devs;
    const int rc = device_list(devs);
    if (rc == RT_OK) dev = devs[0];
    return rc;
}

int validate_scene(const rt_scene* sc)
{
    if (!sc) return fail(RT_EINVAL, "scene is NULL");
    if (sc->nbSpheres < 0 || sc->nbTriangles < 0) return fail(RT_EINVAL, "negative primitive count");
    if (sc->nbSpheres > 0 && !sc->sphere_list) return fail(RT_EINVAL, "sphere_list is NULL");
    if (sc->nbTriangles > 0) {
        if (!sc->triangle_list || !sc->mat_list || !sc->quelMatPourTri)
            return fail(RT_EINVAL, "triangles need triangle_list, mat_list and quelMatPourTri");
        if (sc->tex_width < 1 || sc->tex_height < 1 || sc->nbMaterials < 1)
            return fail(RT_EINVAL, "texture table %dx%d x %d materials", sc->tex_width, sc->tex_height,
                        sc->nbMaterials);
        for (int i = 0; i < sc->nbTriangles; ++i)
            if (sc->quelMatPourTri[i] < 0 || sc->quelMatPourTri[i] >= sc->nbMaterials)
                return fail(RT_EINVAL, "quelMatPourTri[%d] = %d outside [0, %d)", i, sc->quelMatPourTri[i],
                            sc->nbMaterials);
    }
    if (sc->sky_mat_list && (sc->sky_width < 1 || sc->sky_height < 1))
        return fail(RT_EINVAL, "sky table %dx%d", sc->sky_width, sc->sky_height);
    return RT_OK;
}

int validate_params(const rt_params* p)
{
    if (!p) return fail(RT_EINVAL, "params is NULL");
    if (p->largeur_image < 1 || p->hauteur_image < 1)
        return fail(RT_EINVAL, "image %dx%d", p->largeur_image, p->hauteur_image);
    if (p->nbRayonParPixel < 1) return fail(RT_EINVAL, "nbRayonParPixel %d < 1", p->nbRayonParPixel);
    if (p->nbRebondMax < 0) return fail(RT_EINVAL, "nbRebondMax %d < 0", p->nbRebondMax);
    if (p->rng == RT_RNG_GLIBC)
        return fail(RT_EUNSUPPORTED,
                    "RT_RNG_GLIBC is one sequential rand() stream with data-dependent draw counts; "
                    "only the CPU oracle replays it");
    if (p->rng != RT_RNG_PHILOX) return fail(RT_EINVAL, "unknown rng %d", p->rng);
    if (p->accel != RT_ACCEL_AUTO && p->accel != RT_ACCEL_NONE) return fail(RT_EINVAL, "unknown accel %d", p->accel);
    if (p->sky_mode != RT_SKY_OFF && p->sky_mode != RT_SKY_LAST_SPHERE)
        return fail(RT_EINVAL, "unknown sky_mode %d", p->sky_mode);
    if (p->semantics != RT_SEM_MAIN_C && p->semantics != RT_SEM_CUDA)
        return fail(RT_EINVAL, "unknown semantics %d", p->semantics);
    if (p->semantics == RT_SEM_CUDA && p->sky_mode != RT_SKY_OFF)
        return fail(RT_EINVAL, "sky_mode needs RT_SEM_MAIN_C (main_cuda.cu has no sky)");
    if (p->precision == RT_PREC_FP32)
        return fail(RT_EUNSUPPORTED, "RT_PREC_FP32 was removed (r05): its 1.1-3.4e-4 per-channel RMSE against the "
                                     "reference exceeded north_star's 1e-4; only the bit-exact FP64 path renders");
    if (p->precision != RT_PREC_FP64) return fail(RT_EINVAL, "unknown precision %d", p->precision);
    const int transport = p->gather & ~RT_GATHER_PACKED_CANVA;        // the flag goes with either transport
    if (transport != RT_GATHER_RCCL && transport != RT_GATHER_PEER)
        return fail(RT_EINVAL, "unknown gather transport %d", p->gather);
    if ((unsigned long long)p->largeur_image * (unsigned long long)p->hauteur_image > 0xffffffffull)
        return fail(RT_EUNSUPPORTED, "pixel index exceeds the 32-bit Philox counter word");
    return RT_OK;
}

void free_scene(rt_device_scene* s)
{
    if (!s) return;
    DeviceGuard g(s->device);
    delete s;
}

void fill_kparams(const rt_device_scene* sc, const rt_params* p, const rt_tiling* t, KParams& kp, double* uni)
{
    fill_kparams(*sc, sc->facts, p, t, g_zero_exit.load() != 0, kp, uni);
    kp.acc_queue = g_acc_queue.load();           // read by plan_render, and only for a launch with running sums
}

// The current device's default memory pool keeps freed blocks (release
// threshold raised once per device), so repeated launches do not re-map their
// stream-ordered scratch.
int keep_pool_memory()
{
    static std::once_flag pool_once[64];
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev >= 0 && dev < 64) {
        std::call_once(pool_once[dev], [dev]() {
            hipMemPool_t pool;
            if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess) {
                uint64_t thr = UINT64_MAX;
                (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thr);
            }
        });
    }
    return RT_OK;
}

bool frame_size_ok(int W, int H) { return W >= 1 && H >= 1 && (long long)W * H <= (1ll << 30); }

int validate_frame_size(const char* what, int W, int H)
{
    if (W < 1 || H < 1) return fail(RT_EINVAL, "%s: frame %dx%d", what, W, H);
    if (!frame_size_ok(W, H)) return fail(RT_EINVAL, "%s: frame %dx%d above 2^30 pixels", what, W, H);
    return RT_OK;
}

int validate_workspace(const char* what, int W, int H, const void* workspace, size_t workspace_bytes, size_t need)
{
    if (!workspace) return fail(RT_EINVAL, "%s: workspace is NULL", what);
    if ((uintptr_t)workspace % 16) return fail(RT_EINVAL, "%s: workspace is not 16-byte aligned", what);
    if (workspace_bytes < need)
        return fail(RT_EINVAL, "%s: workspace of %zu bytes, %dx%d needs %zu", what, workspace_bytes, W, H, need);
    return RT_OK;
}

int validate_sample_window(long long sample_offset, int S)
{
    if (sample_offset < 0 || sample_offset + S > (1ll << 32))
        return fail(RT_EINVAL, "samples [%lld, %lld) exceed the 32-bit Philox sample word", sample_offset,
                    sample_offset + S);
    return RT_OK;
}

int LaunchScratch::open(KParams& kp, const double* uni, int stack_cap, size_t partial_bytes, bool queue,
                        hipStream_t stream)
{
    st = stream;
    HIP_TRY(hipMallocAsync((void**)&block, kLaunchScratchBytes, st));
    UniBlock ub;
    for (int i = 0; i < U_COUNT; ++i) ub.v[i] = uni[i];
    e = (hipError_t)launch_set_uniforms(ub, block, st);
    if (partial_bytes && e == hipSuccess) e = hipMallocAsync((void**)&partial, partial_bytes, st);
    kp.uni = block;
    kp.task_ctr = (partial && queue) ? (unsigned*)(block + kTaskCtrDouble) : nullptr;
    kp.stack_cap = stack_cap;
    return RT_OK;
}

// One render or count run of kp as plan_render lays it out, band by band (the
// scratch holds the chunk partials of one band).
int launch_on_stream(KParams& kp, const double* uni, hipStream_t st, bool count)
{
    int rc;
    if ((rc = keep_pool_memory())) return rc;
    const RenderPlan plan = plan_render(kp, count);     // kernel, stack and bands, decided once
    LaunchScratch s;
    if ((rc = s.open(kp, uni, plan.stack_cap, plan.partial_bytes, plan.task_ok, st))) return rc;
    kp.partial = s.partial;
    kp.band_rows = plan.band_rows;
    for (int y0 = 0; s.e == hipSuccess && y0 < kp.local_rows; y0 += plan.band_rows) {
        kp.band_y0 = y0;
        s.e = (hipError_t)(count ? launch_count(kp, plan, st) : launch_render(kp, plan, st));
    }
    return s.result("render");
}

// What the scene-taking entry points do once their arguments are checked: the
// launch descriptor with set's outputs, launched on the scene's device.
template <class F>
int launch_scene(const rt_device_scene* scene, const rt_params* params, const rt_tiling* tiling, void* hip_stream,
                 bool count, const F& set)
{
    KParams kp;
    double uni[U_COUNT];
    fill_kparams(scene, params, tiling, kp, uni);
    set(kp);
    if (kp.local_rows == 0) return RT_OK;      // (validate_params: W >= 1)
    DeviceGuard guard(scene->device);
    return launch_on_stream(kp, uni, (hipStream_t)hip_stream, count);
}

}  // namespace rt

using namespace rt;

extern "C" {

void rt_params_init(rt_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->rng = RT_RNG_PHILOX;
    p->seed = 1010ull;
    p->compat_int_truncation = 1;
    p->spp_chunks = RT_SPP_CHUNKS_AUTO;
}

int rt_init(int ndev, const int* devices)
{
    std::lock_guard<std::mutex> lk(g_mu);
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (n < 1) return fail(RT_EDEVICE, "no HIP device");
    std::vector<int> devs;             // committed only when every id is visible
    if (ndev <= 0 || !devices) {
        devs.push_back(0);
    } else {
        for (int i = 0; i < ndev; ++i) {
            if (devices[i] < 0 || devices[i] >= n)
                return fail(RT_EINVAL, "device %d is not visible (%d device%s)", devices[i], n, n == 1 ? "" : "s");
            devs.push_back(devices[i]);
        }
    }
    g_devices.swap(devs);
    g_inited = true;
    return RT_OK;
}

void rt_shutdown(void)
{
    {
        std::lock_guard<std::mutex> lk(g_mu);
        g_devices.clear();
        g_inited = false;
    }
    scene_cache_clear();
    stream_pool_clear();
    rccl_release();
}

const char* rt_last_error(void) { return g_err.c_str(); }
int rt_abi_version(void) { return RT_ABI_VERSION; }
const char* rt_last_render_kernel(void) { return last_render_kernel(); }

const char* rt_version(void)
{
#define RT_STR2(x) #x
#define RT_STR(x) RT_STR2(x)
    return "tipe-raytracer-mi355x 0.6 (abi " RT_STR(RT_ABI_VERSION) ", gfx950; precision FP64, bit-exact against "
           "the reference's own composition; RT_PREC_FP32 removed (RT_EUNSUPPORTED); rt_params_init defaults "
           "spp_chunks to RT_SPP_CHUNKS_AUTO, a fixed per-pixel slice grouping; multi-device gathers over RCCL "
           "(RT_GATHER_RCCL) or peer copies (RT_GATHER_PEER))";
#undef RT_STR
#undef RT_STR2
}

int rt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rt_set_zero_throughput_exit(int enable) { return g_zero_exit.exchange(enable ? 1 : 0); }
int rt_set_accumulate_queue(int enable) { return g_acc_queue.exchange(enable ? 1 : 0); }

int rt_scene_upload(int device, const rt_scene* scene, rt_device_scene** out)
{
    if (!out) return fail(RT_EINVAL, "out is NULL");
    *out = nullptr;
    int rc = validate_scene(scene);
    if (rc) return rc;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(RT_EINVAL, "device %d of %d", device, n);
    DeviceGuard guard(device);
    if (!guard.ok) return fail(RT_EDEVICE, "hipSetDevice(%d) failed", device);
    HostScene hs;
    std::string err;
    if ((rc = prepare_scene(scene, hs, err))) return fail(rc, "%s", err.c_str());
    rt_device_scene* ds = new rt_device_scene();
    ds->device = device;
    ds->facts = hs.facts;
    const auto upload = [](auto& dst, const auto& src) -> int {
        HIP_TRY(dst.upload(src.data(), src.size()));
        return RT_OK;
    };
    if ((rc = upload(ds->sph, hs.sph)) || (rc = upload(ds->sph_cand, hs.sph_cand)) || (rc = upload(ds->cand_orig, hs.cand_orig)) ||
        (rc = upload(ds->sph_slot, hs.sph_slot)) || (rc = upload(ds->sph_mat, hs.sph_mat)) || (rc = upload(ds->tri, hs.tri)) ||
        (rc = upload(ds->tri_tex, hs.tri_tex)) || (rc = upload(ds->tri_uv, hs.tri_uv)) || (rc = upload(ds->texels, hs.texels)) ||
        (rc = upload(ds->bvh, hs.bvh)) || (rc = upload(ds->bvhh, hs.bvhh)) || (rc = upload(ds->bvhw, hs.bvhw)) || (rc = upload(ds->tri_orig, hs.tri_orig)) ||
        (rc = upload(ds->sky, hs.sky)) || (rc = upload(ds->sph_rinv, hs.sph_rinv)) || (rc = upload(ds->sph_disp, hs.sph_disp)) ||
        (rc = upload(ds->tri_mat, hs.tri_mat))) {
        free_scene(ds);
        return rc;
    }
    *out = ds;
    return RT_OK;
}

void rt_scene_release(rt_device_scene* scene) { free_scene(scene); }

int rt_render_async(const rt_device_scene* scene, const rt_params* params, const rt_tiling* tiling,
                    const rt_frame* frame, void* hip_stream)
{
    if (!scene) return fail(RT_EINVAL, "scene is NULL");
    int rc;
    if ((rc = validate_params(params)) || (rc = validate_tiling(tiling))) return rc;
    if (!frame || !frame->canva) return fail(RT_EINVAL, "frame.canva is NULL");
    return launch_scene(scene, params, tiling, hip_stream, false, [&](KParams& kp) { set_frame(kp, frame); });
}

int rt_accumulate_async(const rt_device_scene* scene, const rt_params* params, long long sample_offset,
                        const rt_tiling* tiling, double* d_sums, void* hip_stream)
{
    if (!scene) return fail(RT_EINVAL, "scene is NULL");
    int rc;
    if ((rc = validate_params(params)) || (rc = validate_tiling(tiling))) return rc;
    if (!d_sums) return fail(RT_EINVAL, "d_sums is NULL");
    if ((rc = validate_sample_window(sample_offset, params->nbRayonParPixel))) return rc;
    return launch_scene(scene, params, tiling, hip_stream, false, [&](KParams& kp) {
        kp.sums = d_sums;
        kp.s_base = sample_offset;
    });
}

int rt_resolve_async(const double* d_sums, const rt_params* params, int total_spp, const rt_tiling* tiling,
                     const rt_frame* frame, void* hip_stream)
{
    int rc;
    if ((rc = validate_tiling(tiling))) return rc;
    if (!params || params->largeur_image < 1 || params->hauteur_image < 1) return fail(RT_EINVAL, "bad params");
    if (!d_sums || !frame || !frame->canva) return fail(RT_EINVAL, "NULL buffer");
    if (total_spp < 1) return fail(RT_EINVAL, "total_spp %d < 1", total_spp);
    KParams kp;
    std::memset(&kp, 0, sizeof kp);
    kp.W = params->largeur_image;
    kp.H = params->hauteur_image;
    kp.S = total_spp;
    set_tiling(kp, tiling, params->hauteur_image);
    kp.sums = (double*)d_sums;
    set_frame(kp, frame);
    if (kp.local_rows == 0) return RT_OK;
    const int e = launch_resolve(kp, hip_stream);
    if (e) return fail(RT_EDEVICE, "resolve launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

int rt_count_async(const rt_device_scene* scene, const rt_params* params, const rt_tiling* tiling,
                   unsigned long long* d_counters, void* hip_stream)
{
    if (!scene) return fail(RT_EINVAL, "scene is NULL");
    int rc;
    if ((rc = validate_params(params)) || (rc = validate_tiling(tiling))) return rc;
    if (!d_counters) return fail(RT_EINVAL, "d_counters is NULL");
    return launch_scene(scene, params, tiling, hip_stream, true, [&](KParams& kp) { kp.counters = d_counters; });
}

}  // extern "C"
