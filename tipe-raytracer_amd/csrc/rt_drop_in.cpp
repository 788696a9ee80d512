// rt_drop_in.cpp — the C-ABI's host-buffer drop-ins (rt_render_rows /
// rt_fill_canva, the denoise hook) with their stream pool and scene cache,
// and the device-resident multi-device frame (rt_gather_async,
// rt_render_gather_async).
#include <algorithm>
#include <array>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "rt_api_internal.h"
#include "rt_rccl.h"

using namespace rt;

namespace {

std::atomic<rt_denoise_fn> g_denoise{nullptr};
std::mutex g_denoise_mu;
rt_denoise_params g_denoise_params = {4, 1.0f, 0.5f, 0.25f};   // rt_denoise_atrous's; rt_denoise_params_init's defaults

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

struct PooledStream {
    int device = 0;
    hipStream_t st = nullptr;
    void* host = nullptr;            // pinned staging for the D2H copy
    size_t host_bytes = 0;
    hipEvent_t plane_done[3] = {nullptr, nullptr, nullptr};   // D2H of each output plane
    hipError_t reserve_host(size_t n)
    {
        if (n <= host_bytes) return hipSuccess;
        if (host) (void)hipHostFree(host);
        host = nullptr;
        host_bytes = 0;
        const hipError_t e = hipHostMalloc(&host, n, hipHostMallocDefault);
        if (e == hipSuccess) host_bytes = n;
        return e;
    }
};

std::mutex g_pool_mu;
std::vector<PooledStream*> g_pool_free;    // idle streams (any device); destroyed by rt_shutdown

int stream_pool_get(int device, PooledStream** out)
{
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (size_t i = 0; i < g_pool_free.size(); ++i)
            if (g_pool_free[i]->device == device) {
                *out = g_pool_free[i];
                g_pool_free.erase(g_pool_free.begin() + (long)i);
                return RT_OK;
            }
    }
    DeviceGuard g(device);
    PooledStream* ps = new PooledStream();
    ps->device = device;
    hipError_t e = hipStreamCreateWithFlags(&ps->st, hipStreamNonBlocking);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ps->plane_done[i], hipEventDisableTiming);
    if (e != hipSuccess) {
        for (hipEvent_t ev : ps->plane_done)
            if (ev) (void)hipEventDestroy(ev);
        if (ps->st) (void)hipStreamDestroy(ps->st);
        delete ps;
        return fail(RT_EDEVICE, "device %d stream: %s", device, hipGetErrorString(e));
    }
    *out = ps;
    return RT_OK;
}

void stream_pool_put(PooledStream* ps)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool_free.push_back(ps);
}

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

// The device copy of *sc on `device`, uploaded on first use.  Held under the
// cache lock: concurrent callers of one new scene wait for its single upload.
int scene_cache_get(int device, const rt_scene* sc, std::shared_ptr<rt_device_scene>& out)
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

// ---- device-resident multi-device frame ----------------------
// main_cuda.cu:280-339 renders on one device and copies the three planes to
// the host.  Several devices of one node: each renders its cyclic row tiles,
// and the tiles travel device to device over xGMI (peer copies on the
// destination's copy engines: a gather into one device is G-1 point-to-point
// transfers, which is all ncclGather, rccl.h:745, would issue for it inside one
// process), then the assemble kernel un-permutes them into row order.

// Peer access of dst to src, enabled once per pair.  Status: 1 = enabled
// (the copy engines read src over xGMI), 0 = not available, refused
// (e.g. hipErrorPeerAccessUnsupported) or switched off with the environment
// variable RT_PEER_ACCESS=0; hipMemcpyPeerAsync then stages the copy through
// the host itself, so the gather still works, only slower.
std::mutex g_peer_mu;
std::vector<std::array<int, 3>> g_peer;      // (dst, src, status)

int enable_peer(int dst, int src)
{
    if (dst == src) return 1;
    std::lock_guard<std::mutex> lk(g_peer_mu);
    for (auto& d : g_peer)
        if (d[0] == dst && d[1] == src) return d[2];
    int status = 0;
    const char* env = std::getenv("RT_PEER_ACCESS");
    int can = 0;
    if (!(env && env[0] == '0') && hipDeviceCanAccessPeer(&can, dst, src) == hipSuccess && can) {
        DeviceGuard g(dst);
        const hipError_t e = hipDeviceEnablePeerAccess(src, 0);
        if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) status = 1;
        (void)hipGetLastError();     // a refusal must not poison the next call's error check
    }
    g_peer.push_back({dst, src, status});
    return status;
}

// One plane: slot r's rows_per_rank*W colours (device src_dev[r]) into the
// rank-major staging block r on dst_dev, then assemble into out (W*H).
int gather_plane(int world, const int* src_dev, const rt_color* const* locals, int tile_rows, int rows_per_rank,
                 int W, int H, int dst_dev, rt_color* staging, rt_color* out, hipStream_t st)
{
    const size_t n = (size_t)rows_per_rank * W;
    for (int r = 0; r < world; ++r) {
        if (!locals[r]) return fail(RT_EINVAL, "locals[%d] is NULL", r);
        enable_peer(dst_dev, src_dev[r]);
        const hipError_t e = hipMemcpyPeerAsync(staging + (size_t)r * n, dst_dev, locals[r], src_dev[r],
                                                n * sizeof(rt_color), st);
        if (e != hipSuccess) return fail(RT_EDEVICE, "peer copy %d -> %d: %s", src_dev[r], dst_dev, hipGetErrorString(e));
    }
    const int e = launch_assemble((const double*)staging, (long long)n, world, tile_rows, rows_per_rank, W, H,
                                  (double*)out, st);
    if (e) return fail(RT_EDEVICE, "assemble launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

int check_gather_geometry(int world, int tile_rows, int rows_per_rank, int W, int H)
{
    if (world < 1 || tile_rows < 1 || rows_per_rank < 0 || W < 1 || H < 1 || rows_per_rank % tile_rows)
        return fail(RT_EINVAL, "bad gather geometry");
    const long long tiles = (H + tile_rows - 1) / tile_rows;
    if ((long long)world * (rows_per_rank / tile_rows) < tiles)
        return fail(RT_EINVAL, "%d ranks x %d tiles < %lld tiles", world, rows_per_rank / tile_rows, tiles);
    return RT_OK;
}

thread_local std::string g_gather_transport = "none";

// kp's output planes out of one slot buffer: the n planes of want[] that are
// requested lie back to back, `stride` doubles each; the others are null.
void set_planes(KParams& kp, double* buf, size_t stride, rt_color* const* want, int n)
{
    double** dst[4] = {&kp.canva, &kp.albedo, &kp.normal, &kp.radiance};
    for (int pl = 0; pl < n; ++pl) {
        *dst[pl] = want[pl] ? buf : nullptr;
        if (want[pl]) buf += stride;
    }
}

}  // namespace

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

int rt_peer_access(int dst_device, int src_device)
{
    const int n = rt_device_count();
    if (dst_device < 0 || dst_device >= n || src_device < 0 || src_device >= n)
        return fail(RT_EINVAL, "peer pair %d <- %d: %d visible device%s", dst_device, src_device, n, n == 1 ? "" : "s");
    return enable_peer(dst_device, src_device);
}

int rt_gather_async(int world, const int* src_devices, const rt_color* const* locals, int tile_rows,
                    int rows_per_rank, int W, int H, int dst_device, rt_color* out, void* hip_stream)
{
    int rc;
    if (!src_devices || !locals || !out) return fail(RT_EINVAL, "NULL argument");
    if ((rc = check_gather_geometry(world, tile_rows, rows_per_rank, W, H))) return rc;
    DeviceGuard g(dst_device);
    hipStream_t st = (hipStream_t)hip_stream;
    rt_color* staging = nullptr;
    HIP_TRY(hipMallocAsync((void**)&staging, (size_t)world * rows_per_rank * W * sizeof(rt_color), st));
    rc = gather_plane(world, src_devices, locals, tile_rows, rows_per_rank, W, H, dst_device, staging, out, st);
    (void)hipFreeAsync(staging, st);
    return rc;
}

const char* rt_last_gather_transport(void) { return g_gather_transport.c_str(); }

int rt_render_gather_async(const rt_scene* scene, const rt_params* params, int tile_rows, const rt_frame* frame,
                           void* hip_stream)
{
    int rc;
    if ((rc = validate_scene(scene)) || (rc = validate_params(params))) return rc;
    if (!frame || !frame->canva) return fail(RT_EINVAL, "frame.canva is NULL");
    if (tile_rows < 1) return fail(RT_EINVAL, "tile_rows %d < 1", tile_rows);
    std::vector<int> devs;
    if ((rc = device_list(devs))) return rc;
    const int G = (int)devs.size(), W = params->largeur_image, H = params->hauteur_image;
    // RT_GATHER_RCCL: one rank per device, so the list must not repeat one; the
    // communicators are made (once per list) before anything is enqueued
    const bool rccl = params->gather == RT_GATHER_RCCL;
    if (rccl) {
        for (int a = 0; a < G; ++a)
            for (int b = a + 1; b < G; ++b)
                if (devs[(size_t)a] == devs[(size_t)b])
                    return fail(RT_EUNSUPPORTED, "RT_GATHER_RCCL needs distinct devices (rt_init's list names device %d "
                                                 "twice; RCCL has one rank per GPU): use RT_GATHER_PEER", devs[(size_t)a]);
        std::string err;
        if (rccl_comms(devs, err)) return fail(RT_EDEVICE, "RCCL: %s", err.c_str());
    }
    const int dst = devs[0];
    const int n_tiles = (((H + tile_rows - 1) / tile_rows) + G - 1) / G;      // per slot (rows >= H skipped)
    const int rows_pr = n_tiles * tile_rows;
    rt_color* outs[4] = {frame->canva, frame->albedo, frame->normal, frame->radiance};
    int nplanes = 0;
    for (rt_color* o : outs) nplanes += o ? 1 : 0;
    const size_t plane = (size_t)rows_pr * W;                            // colours per plane and slot
    hipStream_t dst_st = (hipStream_t)hip_stream;

    struct Slot {
        std::shared_ptr<rt_device_scene> sc;
        PooledStream* ps = nullptr;
        rt_color* buf = nullptr;
        hipEvent_t ev = nullptr;
    };
    std::vector<Slot> slots((size_t)G);
    auto release = [&]() {           // stream-ordered: nothing here waits for the GPU
        for (auto& s : slots) {
            if (!s.ps) continue;
            DeviceGuard g(s.ps->device);
            if (s.buf) (void)hipFreeAsync(s.buf, s.ps->st);
            if (s.ev) (void)hipEventDestroy(s.ev);
            stream_pool_put(s.ps);
            s.ps = nullptr;
        }
    };
    // 1. every slot renders its tiles on its own device and pooled stream,
    //    after whatever the caller enqueued on hip_stream before this call
    hipEvent_t go = nullptr;
    {
        DeviceGuard g(dst);
        HIP_TRY(hipEventCreateWithFlags(&go, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(go, dst_st));
    }
    for (int q = 0; q < G && rc == RT_OK; ++q) {
        Slot& s = slots[(size_t)q];
        if ((rc = scene_cache_get(devs[(size_t)q], scene, s.sc)) || (rc = stream_pool_get(devs[(size_t)q], &s.ps))) break;
        DeviceGuard g(devs[(size_t)q]);
        hipError_t e = hipStreamWaitEvent(s.ps->st, go, 0);
        if (e == hipSuccess) e = hipMallocAsync((void**)&s.buf, plane * nplanes * sizeof(rt_color), s.ps->st);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming);
        if (e != hipSuccess) {
            rc = fail(RT_EDEVICE, "device %d frame: %s", devs[(size_t)q], hipGetErrorString(e));
            break;
        }
        rt_tiling t{0, tile_rows, q, G, n_tiles};
        KParams kp;
        double uni[U_COUNT];
        make_kparams(s.sc.get(), params, &t, kp, uni);
        set_planes(kp, (double*)s.buf, plane * 3, outs, 4);
        if ((rc = launch_on_stream(kp, uni, s.ps->st, false))) break;
        if ((e = hipEventRecord(s.ev, s.ps->st)) != hipSuccess)
            rc = fail(RT_EDEVICE, "device %d event: %s", devs[(size_t)q], hipGetErrorString(e));
    }
    // 2. the destination's stream waits for every slot, gathers each plane over
    //    xGMI and un-permutes it; 3. each slot frees its planes after the copies
    if (rc == RT_OK) {
        DeviceGuard g(dst);
        for (int q = 0; q < G && rc == RT_OK; ++q) {
            const hipError_t e = hipStreamWaitEvent(dst_st, slots[(size_t)q].ev, 0);
            if (e != hipSuccess) rc = fail(RT_EDEVICE, "wait: %s", hipGetErrorString(e));
        }
        rt_color* staging = nullptr;
        const size_t per_slot = rccl ? plane * nplanes : plane;             // colours staged per slot
        if (rc == RT_OK) {
            const hipError_t e = hipMallocAsync((void**)&staging, (size_t)G * per_slot * sizeof(rt_color), dst_st);
            if (e != hipSuccess) rc = fail(RT_ENOMEM, "gather staging: %s", hipGetErrorString(e));
        }
        if (rccl && rc == RT_OK) {
            // every slot's planes (contiguous in its buffer) in one ncclGather to
            // rank 0, rank 0's part on hip_stream (which waited for its render),
            // the others' on their own streams after their renders; then one
            // assemble per plane from the rank-major staging
            std::vector<const void*> send((size_t)G);
            std::vector<hipStream_t> sst((size_t)G);
            for (int q = 0; q < G; ++q) {
                send[(size_t)q] = slots[(size_t)q].buf;
                sst[(size_t)q] = q == 0 ? dst_st : slots[(size_t)q].ps->st;
            }
            std::string err;
            if (rccl_gather(devs, send, staging, per_slot * 3, sst, err)) rc = fail(RT_EDEVICE, "RCCL: %s", err.c_str());
            for (int k = 0; k < nplanes && rc == RT_OK; ++k) {
                int pl = -1;
                for (int j = 0, m = 0; j < 4; ++j)
                    if (outs[j] && m++ == k) pl = j;
                const int e = launch_assemble((const double*)(staging + (size_t)k * plane), (long long)per_slot, G,
                                              tile_rows, rows_pr, W, H, (double*)outs[pl], dst_st);
                if (e) rc = fail(RT_EDEVICE, "assemble launch: %s", hipGetErrorString((hipError_t)e));
            }
            if (rc == RT_OK)
                g_gather_transport = "rccl: ncclGather, " + rccl_describe() + ", " + std::to_string(G) + " ranks";
        } else {
            int k = 0;
            for (int pl = 0; pl < 4 && rc == RT_OK; ++pl) {
                if (!outs[pl]) continue;
                std::vector<const rt_color*> loc((size_t)G);
                for (int q = 0; q < G; ++q) loc[(size_t)q] = slots[(size_t)q].buf + (size_t)k * plane;
                rc = gather_plane(G, devs.data(), loc.data(), tile_rows, rows_pr, W, H, dst, staging, outs[pl], dst_st);
                ++k;
            }
            if (rc == RT_OK) g_gather_transport = "peer: hipMemcpyPeerAsync, " + std::to_string(G) + " slots";
        }
        if (staging) (void)hipFreeAsync(staging, dst_st);
        if (rc == RT_OK) {
            // the slots free their planes only after the copies that read them
            hipError_t e = hipEventRecord(go, dst_st);            // reused: "the copies are done"
            if (e != hipSuccess) rc = fail(RT_EDEVICE, "gather event: %s", hipGetErrorString(e));
            for (int q = 0; q < G && rc == RT_OK; ++q) {
                DeviceGuard gq(devs[(size_t)q]);
                if ((e = hipStreamWaitEvent(slots[(size_t)q].ps->st, go, 0)) != hipSuccess)
                    rc = fail(RT_EDEVICE, "device %d wait: %s", devs[(size_t)q], hipGetErrorString(e));
            }
        }
    }
    if (rc != RT_OK) {
        // Keep the error message.  Copies already queued on the destination's
        // stream may still read slot planes, and the slots may still render
        // into them: drain both before release() hands the memory back.
        {
            DeviceGuard g(dst);
            (void)hipStreamSynchronize(dst_st);
        }
        for (auto& s : slots)
            if (s.ps) {
                DeviceGuard gq(s.ps->device);
                (void)hipStreamSynchronize(s.ps->st);
            }
    }
    release();
    {
        DeviceGuard g(dst);
        (void)hipEventDestroy(go);
    }
    return rc;
}

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
    rt_color* outs[3] = {canva, albedo, normal};
    const int nplanes = 3;

    struct Slot {
        std::shared_ptr<rt_device_scene> sc;
        PooledStream* ps = nullptr;
        double* buf = nullptr;      // device planes canva | albedo | normal (only the requested ones)
        int n_tiles = 0;
        size_t plane = 0;           // doubles per plane
        size_t nbuf = 0;            // doubles of the requested planes
    };
    std::vector<Slot> slots((size_t)ndev);
    auto done = [&](int code) {      // every return below: hands the planes and streams back
        for (auto& s : slots) {
            if (!s.ps) continue;
            DeviceGuard g(s.ps->device);
            if (s.buf) (void)hipFreeAsync(s.buf, s.ps->st);
            (void)hipStreamSynchronize(s.ps->st);
            stream_pool_put(s.ps);
            s.ps = nullptr;
        }
        return code;
    };
    // 1. every device: cached scene, pooled stream, stream-ordered planes, launch
    for (int q = 0; q < ndev; ++q) {
        Slot& s = slots[(size_t)q];
        s.n_tiles = ntiles > q ? (ntiles - q + ndev - 1) / ndev : 0;
        if (s.n_tiles == 0) continue;
        if ((rc = scene_cache_get(devs[(size_t)q], scene, s.sc)) || (rc = stream_pool_get(devs[(size_t)q], &s.ps)))
            return done(rc);
        DeviceGuard g(devs[(size_t)q]);
        s.plane = (size_t)s.n_tiles * k * W * 3;
        for (int pl = 0; pl < nplanes; ++pl) s.nbuf += outs[pl] ? s.plane : 0;
        hipError_t e = hipMallocAsync((void**)&s.buf, s.nbuf * sizeof(double), s.ps->st);
        if (e != hipSuccess)
            return done(fail(RT_EDEVICE, "device %d frame: %s", devs[(size_t)q], hipGetErrorString(e)));
        rt_tiling t{row_lo, k, q, ndev, s.n_tiles};
        KParams kp;
        double uni[U_COUNT];
        make_kparams(s.sc.get(), params, &t, kp, uni);
        kp.row_end = row_hi + 1;
        set_planes(kp, s.buf, s.plane, outs, nplanes);
        if ((rc = launch_on_stream(kp, uni, s.ps->st, false))) return done(rc);
    }
    // 2. every device: D2H of the requested planes into its stream's pinned
    //    staging buffer, one copy and event per plane, all enqueued before
    //    any wait (the devices' copies overlap)
    for (int q = 0; q < ndev; ++q) {
        Slot& s = slots[(size_t)q];
        if (s.n_tiles == 0) continue;
        DeviceGuard g(devs[(size_t)q]);
        hipError_t e = s.ps->reserve_host(s.nbuf * sizeof(double));
        size_t off = 0;
        for (int pl = 0; pl < nplanes && e == hipSuccess; ++pl) {
            if (!outs[pl]) continue;
            e = hipMemcpyAsync((double*)s.ps->host + off, s.buf + off, s.plane * sizeof(double), hipMemcpyDeviceToHost,
                               s.ps->st);
            if (e == hipSuccess) e = hipEventRecord(s.ps->plane_done[pl], s.ps->st);
            off += s.plane;
        }
        if (e != hipSuccess) return done(fail(RT_EDEVICE, "device %d copy: %s", devs[(size_t)q], hipGetErrorString(e)));
    }
    // 3. each device and plane as its copy lands: scatter its rows into the
    //    caller's array on several host threads (the next plane is still in
    //    flight meanwhile)
    // (concurrent calls, e.g. rt_fill_canva's pthreads, share the threads)
    const int nthr = std::max(1, std::min(8, (int)std::thread::hardware_concurrency() / 2) / g_calls_in_flight.load());
    for (int q = 0; q < ndev; ++q) {
        Slot& s = slots[(size_t)q];
        if (s.n_tiles == 0) continue;
        DeviceGuard g(devs[(size_t)q]);
        const double* src0 = (const double*)s.ps->host;
        for (int pl = 0; pl < nplanes; ++pl) {
            if (!outs[pl]) continue;
            const hipError_t e = hipEventSynchronize(s.ps->plane_done[pl]);
            if (e != hipSuccess)
                return done(fail(RT_EDEVICE, "device %d render/copy: %s", devs[(size_t)q], hipGetErrorString(e)));
            // this device's local rows [r0, r1), tile by tile (the part of each that lies in the range):
            // tile lt = caller rows row_lo + (q + lt * ndev) * k + [0, k); rows past row_hi are padding
            auto rows = [&, src0, pl](int r0, int r1) {
                for (int r = r0; r < r1; r += k - r % k) {
                    const int gr = row_lo + (q + r / k * ndev) * k + r % k;
                    const int n = std::min({k - r % k, r1 - r, row_hi + 1 - gr});
                    if (n > 0)
                        std::memcpy(outs[pl] + (size_t)gr * W, src0 + (size_t)r * W * 3, sizeof(double) * 3 * (size_t)W * n);
                }
            };
            const int nloc = s.n_tiles * k;
            par_ranges(nloc, (size_t)nloc * W * 24 >= (4u << 20) ? nthr : 1, rows);
            src0 += s.plane;
        }
    }
    done(RT_OK);
    // main.c:455: denoiser() on the finished frame
    const rt_denoise_fn hook = g_denoise.load();
    if (hook && row_hi == params->hauteur_image - 1 && row_lo == 0 && albedo && normal)
        hook(W, params->hauteur_image, canva, params->cam, albedo, normal);
    return RT_OK;
}

void rt_set_denoise_hook(rt_denoise_fn fn) { g_denoise.store(fn); }
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

int rt_denoise_host(int W, int H, rt_color* canva, const rt_color* albedo, const rt_color* normal,
                    const rt_denoise_params* params)
{
    int rc, dev;
    if ((rc = validate_denoise(W, H, params))) return rc;
    if (!canva) return fail(RT_EINVAL, "denoise: canva is NULL");
    if ((rc = first_device(dev))) return rc;
    PooledStream* ps = nullptr;
    if ((rc = stream_pool_get(dev, &ps))) return rc;
    DeviceGuard g(dev);
    const size_t plane = (size_t)W * H * sizeof(rt_color), ws_bytes = rt_denoise_workspace_bytes(W, H);
    const rt_color* src[3] = {canva, albedo, normal};
    char* buf = nullptr;             // device: the workspace, then the given planes
    auto done = [&](int code) {
        if (buf) (void)hipFreeAsync(buf, ps->st);
        (void)hipStreamSynchronize(ps->st);
        stream_pool_put(ps);
        return code;
    };
    hipError_t e = ps->reserve_host(3 * plane);
    if (e == hipSuccess) e = hipMallocAsync((void**)&buf, ws_bytes + 3 * plane, ps->st);
    if (e != hipSuccess) return done(fail(RT_ENOMEM, "denoise buffers: %s", hipGetErrorString(e)));
    rt_frame fr = {nullptr, nullptr, nullptr, nullptr};
    rt_color** dst[3] = {&fr.canva, &fr.albedo, &fr.normal};
    for (int pl = 0; pl < 3 && e == hipSuccess; ++pl) {
        if (!src[pl]) continue;
        char* host = (char*)ps->host + pl * plane;
        std::memcpy(host, src[pl], plane);
        *dst[pl] = (rt_color*)(buf + ws_bytes + pl * plane);
        e = hipMemcpyAsync(*dst[pl], host, plane, hipMemcpyHostToDevice, ps->st);
    }
    if (e != hipSuccess) return done(fail(RT_EDEVICE, "denoise upload: %s", hipGetErrorString(e)));
    if ((rc = rt_denoise_async(W, H, &fr, params, buf, ws_bytes, nullptr, ps->st))) return done(rc);
    e = hipMemcpyAsync(ps->host, fr.canva, plane, hipMemcpyDeviceToHost, ps->st);
    if (e == hipSuccess) e = hipStreamSynchronize(ps->st);
    if (e != hipSuccess) return done(fail(RT_EDEVICE, "denoise: %s", hipGetErrorString(e)));
    std::memcpy(canva, ps->host, plane);
    return done(RT_OK);
}

int rt_set_denoise_params(const rt_denoise_params* params)
{
    rt_denoise_params p;
    rt_denoise_params_init(&p);
    if (params) {
        const int rc = validate_denoise(1, 1, params);
        if (rc) return rc;
        p = *params;
    }
    std::lock_guard<std::mutex> lk(g_denoise_mu);
    g_denoise_params = p;
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
