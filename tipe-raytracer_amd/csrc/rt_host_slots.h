// rt_host_slots.h — what a host-buffer drop-in or a gather holds while it
// runs, as owning types: an event, a stream-ordered device buffer, a pooled
// stream, one device slot's render, and one whole frame's way to the host
// (HostFrameJob).  Shared by rt_drop_in.cpp (the pool, the scene cache,
// RenderSlot::render, HostFrameJob), rt_gather.cpp, rt_denoise_api.cpp and
// rt_adaptive_api.cpp.
#pragma once
#include <initializer_list>
#include <memory>
#include <optional>

#include "rt_api_internal.h"

namespace rt {

// A stream of the per-device pool with its pinned staging buffer and one
// "copy landed" event per output plane; all of them live until rt_shutdown.
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

// The device copy of *sc on `device` from the scene cache, uploaded on first use.
int scene_cache_get(int device, const rt_scene* sc, std::shared_ptr<rt_device_scene>& out);

// An event without timing, destroyed with its owner.
struct Event : NoCopy {
    hipEvent_t ev = nullptr;
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t create() { return hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
    operator hipEvent_t() const { return ev; }
};

// hipMallocAsync on a stream of the current device; freed in the order of
// that same stream, which therefore has to outlive the buffer.
struct StreamBuffer : NoCopy {
    void* p = nullptr;
    size_t bytes = 0;
    hipStream_t st = nullptr;
    int device = 0;
    ~StreamBuffer()
    {
        if (!p) return;
        DeviceGuard g(device);
        (void)hipFreeAsync(p, st);
    }
    hipError_t alloc(size_t n, hipStream_t stream, int current_device)
    {
        bytes = n;
        st = stream;
        device = current_device;
        return hipMallocAsync(&p, n, st);
    }
};

// A stream of the pool (rt_drop_in.cpp) for the length of a call.  drain: the
// host waits for the stream before the pool gets it back (the host-buffer
// drop-ins, whose callers read the results next); without it the release
// waits for nothing and the next user's work simply queues behind this one's.
struct StreamLease : NoCopy {
    PooledStream* ps = nullptr;
    bool drain = false;
    ~StreamLease();
    int acquire(int device, bool drain_on_return);     // an idle stream of the device's, or a new one
    PooledStream* operator->() const { return ps; }
};

// One device slot of rt_render_rows or rt_render_gather_async.  Members are
// destroyed last to first: the planes' stream-ordered free is enqueued before
// the stream goes back to the pool (drained first, when the lease says so).
struct RenderSlot {
    std::shared_ptr<rt_device_scene> sc;
    StreamLease stream;
    Event rendered;          // a gather slot's: recorded behind the render
    StreamBuffer buf;        // the requested planes back to back, `plane` doubles each
    size_t plane = 0;
    unsigned* packed = nullptr;   // pack_canva: the canva as plane / 3 packed words, behind the planes in buf

    // Renders tiling t of the frame, up to row_end, on `device`: cached scene,
    // pooled stream, stream-ordered planes for the non-null entries of
    // want[0..4), launch.  Without `go` this is a host-buffer slot, whose
    // stream is drained when the slot goes.  With it, a gather slot: the
    // stream first waits for go, `rendered` is recorded behind the render,
    // and the slot goes without waiting for the GPU.  pack_canva: the canva
    // is packed (rt.h "packed canva transport") into `packed` on the same
    // stream right behind the render, before `rendered`.
    int render(int device, const rt_scene* scene, const rt_params* params, const rt_tiling& t, int row_end,
               rt_color* const* want, hipEvent_t go, bool pack_canva = false);
};

// One whole frame rendered or filtered into the caller's host arrays on the
// first device of rt_init's list (rt_render_vdenoised, rt_render_adaptive[_vdenoised],
// rt_denoise_host): open, enqueue the async entry points on stream() with
// pieces of the device buffer, finish.  Members are destroyed last to first,
// and the job relies on that order: the buffer's stream-ordered free is
// enqueued first, then the caller's device is current again, then the lease
// waits for the stream (the caller reads its arrays next) and returns it.
struct HostFrameJob {
    struct Copy { void* host; const void* dev; size_t bytes; };     // host: the caller's array; null: not asked for
    // `scene` may be null.  host_bytes: the pinned staging, enough for all that upload is given and for all that
    // finish copies.  A failed reservation or allocation is RT_ENOMEM "<what> buffers: ...".
    int open(const char* what, const rt_scene* scene, size_t host_bytes, size_t device_bytes);
    hipStream_t stream() const { return lease->st; }
    const rt_device_scene* scene() const { return sc.get(); }
    // The next `bytes` of the device buffer, back to back (callers round up to 16 where a piece needs it).  More
    // than open was given is a bug of the entry point, never user input: an invariant check that abort()s.
    char* take(size_t bytes) { return bump(buf.p, buf.bytes, taken, bytes); }
    // H2D through the staging, behind what the stream already holds (RT_EDEVICE "<what> upload: ...")
    int upload(void* dst_dev, const void* src_host, size_t bytes);
    // D2H of every asked-for copy into the staging, the stream drained, then the staging into the caller's
    // arrays: none of them is written unless everything succeeded (RT_EDEVICE "<what>: ...")
    int finish(std::initializer_list<Copy> copies);

private:
    const char* what = "";
    std::shared_ptr<rt_device_scene> sc;
    StreamLease lease;
    std::optional<DeviceGuard> current;      // the job's device, from open on
    StreamBuffer buf;
    size_t taken = 0, staged = 0;
    static char* bump(void* base, size_t size, size_t& used, size_t bytes);
    char* stage(size_t bytes) { return bump(lease->host, lease->host_bytes, staged, bytes); }   // of the pinned staging
};

}  // namespace rt
