// rt_drop_in.cpp — the C-ABI's host-buffer drop-ins (rt_render_rows /
// rt_fill_canva) with their stream pool and scene cache, the one device
// slot's render (rt_host_slots.h) that they share with rt_gather.cpp, and the
// whole-frame job (HostFrameJob) of the single-device renders and filters into
// host arrays (rt_denoise_api.cpp, rt_adaptive_api.cpp).
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "rt_host_slots.h"
#include "rt_pack.h"

using namespace rt;

namespace {

// ---- host-buffer drop-in plumbing (rt_render_rows / rt_fill_canva) --------
// main.c runs fill_canva on NUM_THREADS pthreads (main.c:404-453); each of
// them becomes one rt_render_rows call.  So that those calls neither re-upload
// the scene (and rebuild its BVH) nor serialise on hipFree/hipStreamDestroy:
//  * uploaded scenes are cached per device, keyed by the exact bytes of the
//    caller's arrays (a changed array is a different scene, never stale);
//  * streams come from a per-device pool, each with a pinned staging buffer
//    for its D2H copy, reused across calls;
//  * frame planes are stream-ordered allocations (hipMallocAsync) from the
//    device pool whose release threshold launch_on_stream raises.
std::atomic<int> g_fill_chunks{RT_SPP_CHUNKS_AUTO};

std::mutex g_pool_mu;
std::vector<PooledStream*> g_pool_free;    // idle streams (any device); destroyed by rt_shutdown

std::atomic<int> g_calls_in_flight{0};    // rt_render_rows calls running (rt_fill_canva's threads)

// fn(i0, i1) over [0, n) split into nthr contiguous ranges, the first on
// the calling thread (host-side scatter of a frame's rows)
template <class F>
void par_ranges(int n, int nthr, const F& fn)
{
    nthr = std::max(1, std::min(nthr, n));
    if (nthr == 1) {
        fn(0, n);
        return;
    }
    std::vector<std::thread> th;
    th.reserve((size_t)nthr - 1);
    for (int t = 1; t < nthr; ++t) th.emplace_back(fn, (int)((long long)n * t / nthr), (int)((long long)n * (t + 1) / nthr));
    fn(0, (int)((long long)n / nthr));
    for (auto& x : th) x.join();
}

// Exact bytes of everything rt_scene_upload reads.
std::vector<unsigned char> scene_key(const rt_scene* sc)
{
    std::vector<unsigned char> k;
    auto put = [&k](const void* p, size_t n) {
        const unsigned char* b = (const unsigned char*)p;
        k.insert(k.end(), b, b + n);
    };
    const int hdr[7] = {sc->nbSpheres, sc->nbTriangles, sc->tex_width, sc->tex_height, sc->nbMaterials,
                        sc->sky_mat_list ? sc->sky_width : -1, sc->sky_mat_list ? sc->sky_height : -1};
    put(hdr, sizeof hdr);
    if (sc->nbSpheres > 0) put(sc->sphere_list, sizeof(rt_sphere) * (size_t)sc->nbSpheres);
    if (sc->nbTriangles > 0) {
        put(sc->triangle_list, sizeof(rt_triangle) * (size_t)sc->nbTriangles);
        put(sc->quelMatPourTri, sizeof(int) * (size_t)sc->nbTriangles);
        put(sc->mat_list, sizeof(rt_material) * (size_t)sc->nbMaterials * sc->tex_width * sc->tex_height);
    }
    if (sc->sky_mat_list) put(sc->sky_mat_list, sizeof(rt_material) * (size_t)sc->sky_width * sc->sky_height);
    return k;
}

struct CachedScene {
    int device;
    std::vector<unsigned char> key;
    std::shared_ptr<rt_device_scene> ds;
    unsigned long long used;
};
// The cache is a heap object that is never destroyed: a process that exits
// without rt_shutdown (main.c's drop-in flow never calls it) must not run
// free_scene -> hipFree from a static destructor after the HIP runtime may
// already be torn down; the driver reclaims the device memory at exit.
std::mutex g_cache_mu;
std::vector<CachedScene>& g_cache = *new std::vector<CachedScene>();   // at most kCacheEntries, LRU evicted
unsigned long long g_cache_clock = 0;
constexpr size_t kCacheEntries = 4;

}  // namespace

int StreamLease::acquire(int device, bool drain_on_return)
{
    drain = drain_on_return;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (size_t i = 0; i < g_pool_free.size(); ++i)
            if (g_pool_free[i]->device == device) {
                ps = g_pool_free[i];
                g_pool_free.erase(g_pool_free.begin() + (long)i);
                return RT_OK;
            }
    }
    DeviceGuard g(device);
    PooledStream* n = new PooledStream();
    n->device = device;
    hipError_t e = hipStreamCreateWithFlags(&n->st, hipStreamNonBlocking);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&n->plane_done[i], hipEventDisableTiming);
    if (e != hipSuccess) {
        for (hipEvent_t ev : n->plane_done)
            if (ev) (void)hipEventDestroy(ev);
        if (n->st) (void)hipStreamDestroy(n->st);
        delete n;
        return fail(RT_EDEVICE, "device %d stream: %s", device, hipGetErrorString(e));
    }
    ps = n;
    return RT_OK;
}

StreamLease::~StreamLease()
{
    if (!ps) return;
    if (drain) {
        DeviceGuard g(ps->device);
        (void)hipStreamSynchronize(ps->st);
    }
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool_free.push_back(ps);
}

// The device copy of *sc on `device`, uploaded on first use.  Held under the
// cache lock: concurrent callers of one new scene wait for its single upload.
int rt::scene_cache_get(int device, const rt_scene* sc, std::shared_ptr<rt_device_scene>& out)
{
    std::vector<unsigned char> key = scene_key(sc);
    std::lock_guard<std::mutex> lk(g_cache_mu);
    for (CachedScene& c : g_cache)
        if (c.device == device && c.key == key) {
            c.used = ++g_cache_clock;
            out = c.ds;
            return RT_OK;
        }
    rt_device_scene* ds = nullptr;
    const int rc = rt_scene_upload(device, sc, &ds);
    if (rc) return rc;
    if (g_cache.size() >= kCacheEntries) {
        size_t lru = 0;
        for (size_t i = 1; i < g_cache.size(); ++i)
            if (g_cache[i].used < g_cache[lru].used) lru = i;
        g_cache.erase(g_cache.begin() + (long)lru);    // in-flight users keep their reference
    }
    g_cache.push_back(CachedScene{device, std::move(key), std::shared_ptr<rt_device_scene>(ds, free_scene),
                                  ++g_cache_clock});
    out = g_cache.back().ds;
    return RT_OK;
}

int RenderSlot::render(int device, const rt_scene* scene, const rt_params* params, const rt_tiling& t, int row_end,
                       rt_color* const* want, hipEvent_t go, bool pack_canva)
{
    int rc;
    if ((rc = scene_cache_get(device, scene, sc)) || (rc = stream.acquire(device, !go))) return rc;
    DeviceGuard g(device);
    plane = (size_t)t.n_tiles * t.tile_rows * params->largeur_image * 3;
    size_t n = 0;
    for (int pl = 0; pl < 4; ++pl) n += want[pl] ? plane : 0;
    hipError_t e = go ? hipStreamWaitEvent(stream->st, go, 0) : hipSuccess;
    if (e == hipSuccess) e = buf.alloc(n * sizeof(double) + (pack_canva ? plane / 3 * sizeof(unsigned) : 0), stream->st, device);
    if (e == hipSuccess && go) e = rendered.create();
    if (e != hipSuccess) return fail(RT_EDEVICE, "device %d frame: %s", device, hipGetErrorString(e));
    KParams kp;
    double uni[U_COUNT];
    fill_kparams(sc.get(), params, &t, kp, uni);
    kp.row_end = row_end;
    double* next = (double*)buf.p;
    double** dst[4] = {&kp.canva, &kp.albedo, &kp.normal, &kp.radiance};
    for (int pl = 0; pl < 4; ++pl)
        if (want[pl]) {
            *dst[pl] = next;
            next += plane;
        }
    if ((rc = launch_on_stream(kp, uni, stream->st, false))) return rc;
    if (pack_canva) {
        packed = (unsigned*)((double*)buf.p + n);
        if ((rc = rt_canva_pack_async((long long)(plane / 3), (const rt_color*)kp.canva, packed, stream->st))) return rc;
    }
    if (go && (e = hipEventRecord(rendered, stream->st)) != hipSuccess)
        return fail(RT_EDEVICE, "device %d event: %s", device, hipGetErrorString(e));
    return RT_OK;
}

int HostFrameJob::open(const char* name, const rt_scene* scene, size_t host_bytes, size_t device_bytes)
{
    what = name;
    int rc, dev;
    if ((rc = first_device(dev))) return rc;
    if (scene && (rc = scene_cache_get(dev, scene, sc))) return rc;
    if ((rc = lease.acquire(dev, true))) return rc;     // drained on every return: the caller reads its arrays next
    current.emplace(dev);
    hipError_t e = lease->reserve_host(host_bytes);
    if (e == hipSuccess) e = buf.alloc(device_bytes, lease->st, dev);
    if (e != hipSuccess) return fail(RT_ENOMEM, "%s buffers: %s", what, hipGetErrorString(e));
    return RT_OK;
}

// (a caller whose pieces exceed what it opened the job with must not get as far as the device)
char* HostFrameJob::bump(void* base, size_t size, size_t& used, size_t bytes)
{
    if (bytes > size - used) std::abort();
    used += bytes;
    return (char*)base + used - bytes;
}

int HostFrameJob::upload(void* dst_dev, const void* src_host, size_t bytes)
{
    char* host = stage(bytes);
    std::memcpy(host, src_host, bytes);
    const hipError_t e = hipMemcpyAsync(dst_dev, host, bytes, hipMemcpyHostToDevice, lease->st);
    if (e != hipSuccess) return fail(RT_EDEVICE, "%s upload: %s", what, hipGetErrorString(e));
    return RT_OK;
}

int HostFrameJob::finish(std::initializer_list<Copy> copies)
{
    hipError_t e = hipSuccess;
    staged = 0;              // behind the uploads in stream order, so their staging is free again
    for (const Copy& c : copies)
        if (c.host && e == hipSuccess) e = hipMemcpyAsync(stage(c.bytes), c.dev, c.bytes, hipMemcpyDeviceToHost, lease->st);
    if (e == hipSuccess) e = hipStreamSynchronize(lease->st);
    if (e != hipSuccess) return fail(RT_EDEVICE, "%s: %s", what, hipGetErrorString(e));
    staged = 0;
    for (const Copy& c : copies)
        if (c.host) std::memcpy(c.host, stage(c.bytes), c.bytes);
    return RT_OK;
}

// Idle pooled streams and their pinned staging buffers (streams a call still
// holds go back to the pool when it returns and are released by the next
// rt_shutdown).
void rt::stream_pool_clear()
{
    std::vector<PooledStream*> idle;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        idle.swap(g_pool_free);
    }
    for (PooledStream* ps : idle) {
        DeviceGuard g(ps->device);
        (void)hipStreamSynchronize(ps->st);
        (void)hipStreamDestroy(ps->st);
        for (hipEvent_t ev : ps->plane_done)
            if (ev) (void)hipEventDestroy(ev);
        if (ps->host) (void)hipHostFree(ps->host);
        delete ps;
    }
}

int rt::scene_cache_clear()
{
    std::lock_guard<std::mutex> lk(g_cache_mu);
    const int n = (int)g_cache.size();
    g_cache.clear();
    return n;
}

extern "C" {

int rt_render_rows(const rt_scene* scene, const rt_params* params, int row_hi, int row_lo, rt_color* canva,
                   rt_color* albedo, rt_color* normal)
{
    int rc;
    if ((rc = validate_scene(scene)) || (rc = validate_params(params))) return rc;
    if (!canva) return fail(RT_EINVAL, "canva is NULL");
    if (row_lo < 0 || row_hi >= params->hauteur_image || row_hi < row_lo)
        return fail(RT_EINVAL, "rows %d..%d outside [0, %d)", row_hi, row_lo, params->hauteur_image);
    std::vector<int> devs;
    if ((rc = device_list(devs))) return rc;
    const int W = params->largeur_image;
    const int nrows = row_hi - row_lo + 1;
    const int ndev = (int)devs.size();
    struct InFlight {
        InFlight() { ++g_calls_in_flight; }
        ~InFlight() { --g_calls_in_flight; }
    } in_flight;
    // One device: one band.  Several: cyclic 1-row tiles (load balance: the
    // busiest device renders at most one row more than the average).
    const int k = ndev == 1 ? nrows : 1;
    const int ntiles = (nrows + k - 1) / k;
    rt_color* outs[4] = {canva, albedo, normal, nullptr};
    const int nplanes = 3;
    // rt_set_fill_packed_canva: the canva leaves the device as one word per
    // pixel (packed behind the render) and is widened into the caller's rows
    const bool packed = fill_packed_canva();
    if (packed && (long long)((nrows + ndev - 1) / ndev) * W > kPackMaxPixels)     // the busiest device's rows
        return fail(RT_EINVAL, "packed canva: more than 2^30 pixels per device");
    // a slot's destructor frees its planes in stream order, then waits for its
    // stream and hands it back: on every return below
    std::vector<RenderSlot> slots((size_t)ndev);
    auto tiles_of = [&](int q) { return ntiles > q ? (ntiles - q + ndev - 1) / ndev : 0; };   // 0: the slot is not used
    // 1. every device: cached scene, pooled stream, stream-ordered planes, launch
    for (int q = 0; q < ndev; ++q) {
        const rt_tiling t{row_lo, k, q, ndev, tiles_of(q)};
        if (t.n_tiles > 0 &&
            (rc = slots[(size_t)q].render(devs[(size_t)q], scene, params, t, row_hi + 1, outs, nullptr, packed)))
            return rc;
    }
    // 2. every device: D2H of the requested planes into its stream's pinned
    //    staging buffer, one copy and event per plane, all enqueued before
    //    any wait (the devices' copies overlap)
    for (int q = 0; q < ndev; ++q) {
        RenderSlot& s = slots[(size_t)q];
        if (tiles_of(q) == 0) continue;
        DeviceGuard g(devs[(size_t)q]);
        hipError_t e = s.stream->reserve_host(s.buf.bytes);
        size_t off = 0;
        for (int pl = 0; pl < nplanes && e == hipSuccess; ++pl) {
            if (!outs[pl]) continue;
            if (pl == 0 && packed)         // the words sit behind the planes, on the device and in the staging
                e = hipMemcpyAsync((char*)s.stream->host + ((char*)s.packed - (char*)s.buf.p), s.packed,
                                   s.plane / 3 * sizeof(unsigned), hipMemcpyDeviceToHost, s.stream->st);
            else
                e = hipMemcpyAsync((double*)s.stream->host + off, (const double*)s.buf.p + off,
                                   s.plane * sizeof(double), hipMemcpyDeviceToHost, s.stream->st);
            if (e == hipSuccess) e = hipEventRecord(s.stream->plane_done[pl], s.stream->st);
            off += s.plane;
        }
        if (e != hipSuccess) return fail(RT_EDEVICE, "device %d copy: %s", devs[(size_t)q], hipGetErrorString(e));
    }
    // 3. each device and plane as its copy lands: scatter its rows into the
    //    caller's array on several host threads (the next plane is still in
    //    flight meanwhile)
    // (concurrent calls, e.g. rt_fill_canva's pthreads, share the threads)
    const int nthr = std::max(1, std::min(8, (int)std::thread::hardware_concurrency() / 2) / g_calls_in_flight.load());
    for (int q = 0; q < ndev; ++q) {
        RenderSlot& s = slots[(size_t)q];
        if (tiles_of(q) == 0) continue;
        DeviceGuard g(devs[(size_t)q]);
        const double* src0 = (const double*)s.stream->host;
        for (int pl = 0; pl < nplanes; ++pl) {
            if (!outs[pl]) continue;
            const hipError_t e = hipEventSynchronize(s.stream->plane_done[pl]);
            if (e != hipSuccess)
                return fail(RT_EDEVICE, "device %d render/copy: %s", devs[(size_t)q], hipGetErrorString(e));
            // this device's local rows [r0, r1), tile by tile (the part of each that lies in the range):
            // tile lt = caller rows row_lo + (q + lt * ndev) * k + [0, k); rows past row_hi are padding
            const unsigned* words =
                pl == 0 && packed ? (const unsigned*)((const char*)s.stream->host + ((char*)s.packed - (char*)s.buf.p))
                                  : nullptr;
            auto rows = [&, src0, pl, words](int r0, int r1) {
                for (int r = r0; r < r1; r += k - r % k) {
                    const int gr = row_lo + (q + r / k * ndev) * k + r % k;
                    const int n = std::min({k - r % k, r1 - r, row_hi + 1 - gr});
                    if (n <= 0) continue;
                    if (words)
                        (void)rt_canva_unpack_host((long long)W * n, words + (size_t)r * W, outs[pl] + (size_t)gr * W);
                    else
                        std::memcpy(outs[pl] + (size_t)gr * W, src0 + (size_t)r * W * 3, sizeof(double) * 3 * (size_t)W * n);
                }
            };
            const int nloc = tiles_of(q) * k;
            par_ranges(nloc, (size_t)nloc * W * 24 >= (4u << 20) ? nthr : 1, rows);
            src0 += s.plane;
        }
    }
    slots.clear();       // the frame is complete and the streams are back before the hook runs
    // main.c:455: denoiser() on the finished frame
    const rt_denoise_fn hook = rt_get_denoise_hook();
    if (hook && row_hi == params->hauteur_image - 1 && row_lo == 0 && albedo && normal)
        hook(W, params->hauteur_image, canva, params->cam, albedo, normal);
    return RT_OK;
}

int rt_set_fill_spp_chunks(int spp_chunks)
{
    if (spp_chunks < RT_SPP_CHUNKS_AUTO) spp_chunks = 1;
    return g_fill_chunks.exchange(spp_chunks);
}
int rt_set_fill_precision(int precision)
{
    // RT_PREC_FP32 was removed (r05): rt_fill_canva renders FP64 only
    if (precision == RT_PREC_FP32)
        return fail(RT_EUNSUPPORTED, "RT_PREC_FP32 was removed (r05); rt_fill_canva renders FP64");
    if (precision != RT_PREC_FP64) return fail(RT_EINVAL, "unknown precision %d", precision);
    return RT_PREC_FP64;
}
int rt_scene_cache_clear(void) { return scene_cache_clear(); }

void* rt_fill_canva(void* arg)
{
    const rt_thread_data* d = (const rt_thread_data*)arg;
    if (!d) {
        fail(RT_EINVAL, "thread data is NULL");
        return (void*)1;
    }
    int nmat = 0;
    for (int i = 0; i < d->nbTriangles; ++i)
        if (d->quelMatPourTri && d->quelMatPourTri[i] + 1 > nmat) nmat = d->quelMatPourTri[i] + 1;
    rt_scene sc;
    std::memset(&sc, 0, sizeof sc);
    sc.sphere_list = d->sphere_list;
    sc.nbSpheres = d->nbSpheres;
    sc.triangle_list = d->triangle_list;
    sc.nbTriangles = d->nbTriangles;
    sc.mat_list = d->mat_list;
    sc.tex_width = d->tex_width;
    sc.tex_height = d->tex_height;
    sc.nbMaterials = nmat;
    sc.quelMatPourTri = d->quelMatPourTri;
    sc.sky_mat_list = d->sky_mat_list;        // carried like ThreadData does; sky_mode stays OFF (main.c)
    sc.sky_width = d->sky_width;
    sc.sky_height = d->sky_height;
    rt_params p;
    rt_params_init(&p);
    p.largeur_image = d->largeur_image;
    p.hauteur_image = d->hauteur_image;
    p.nbRayonParPixel = d->nbRayonParPixel;
    p.nbRebondMax = d->nbRebondMax;
    p.cam = d->cam;
    p.focus_distance = d->focus_distance;     // already int in ThreadData
    p.ouverture_x = d->ouverture_x;
    p.ouverture_y = d->ouverture_y;
    p.AO_intensity = d->AO_intensity;
    p.useAO = d->useAO ? 1 : 0;
    p.compat_int_truncation = 0;
    p.spp_chunks = g_fill_chunks.load();
    p.precision = RT_PREC_FP64;
    const int rc = rt_render_rows(&sc, &p, d->start_row, d->end_row, d->canva, d->albedo_tab, d->normal_tab);
    return rc == RT_OK ? nullptr : (void*)1;
}

}  // extern "C"
