// rt_host_slots.h — what a host-buffer drop-in or a gather holds while it
// runs, as owning types: an event, a stream-ordered device buffer, a pooled
// stream, and one device slot's render.  Shared by rt_drop_in.cpp (the pool,
// the scene cache, RenderSlot::render), rt_gather.cpp and rt_denoise_api.cpp.
#pragma once
#include <memory>

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

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};

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

}  // namespace rt
