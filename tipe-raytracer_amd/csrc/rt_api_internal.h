// rt_api_internal.h — what the C-ABI's files (rt_api.cpp, rt_drop_in.cpp,
// rt_gather.cpp, rt_denoise_api.cpp, rt_adaptive_api.cpp, rt_diag.cpp) share:
// error reporting, the device list, the refusals, owning device memory, a
// launch's scratch and the uploaded scene.  What a drop-in holds while it runs
// (streams, buffers, slots, the whole-frame job) is in rt_host_slots.h.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "rt/rt.h"
#include "rt_internal.h"
#include "rt_launch_plan.h"
#include "rt_scene_prep.h"

namespace rt {

// Sets the calling thread's rt_last_error() text (one object for the whole
// library, rt_api.cpp) and returns code.
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(RT_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                \
    } while (0)

// Restores the caller's current device on scope exit (torch owns it in bench).
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess) ok = true;
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};

// Device memory that is freed with its owner (on the device that is current
// then).  Null until alloc/upload; an empty upload leaves it null.
template <class T>
struct DevArray : NoCopy {
    T* p = nullptr;
    ~DevArray() { (void)hipFree(p); }
    operator T*() const { return p; }
    hipError_t alloc(size_t n) { return hipMalloc((void**)&p, n * sizeof(T)); }
    hipError_t upload(const T* src, size_t n)
    {
        if (n == 0) return hipSuccess;
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
    }
};

// The rt_init device list (device 0 when rt_init was not called), and its
// first entry: where the diagnostics run.
int device_list(std::vector<int>& devs);
int first_device(int& dev);

int validate_scene(const rt_scene* sc);
int validate_params(const rt_params* p);
int validate_vdenoise(int W, int H, const rt_vdenoise_params* p);    // rt_denoise_api.cpp: the frame size too

// What adaptive sampling and the two denoisers refuse alike; `what` is the caller's prefix ("adaptive",
// "denoise", "vdenoise").  A frame: W, H >= 1 and at most 2^30 pixels.  A workspace: not NULL, 16-byte aligned,
// `need` bytes, checked in that order.  A sample window: [offset, offset + S) within the 32-bit Philox word.
bool frame_size_ok(int W, int H);
int validate_frame_size(const char* what, int W, int H);
int validate_workspace(const char* what, int W, int H, const void* workspace, size_t workspace_bytes, size_t need);
int validate_sample_window(long long sample_offset, int S);

// rt_launch_plan.h's fill_kparams on an uploaded scene, with rt_set_zero_throughput_exit's switch;
// launch_on_stream plans the launch (plan_render) and runs its bands.
// keep_pool_memory: the launches' stream-ordered scratch stays mapped between calls (once per device).
void fill_kparams(const rt_device_scene* sc, const rt_params* p, const rt_tiling* t, KParams& kp, double* uni);
int keep_pool_memory();
int launch_on_stream(KParams& kp, const double* uni, hipStream_t st, bool count);
void free_scene(rt_device_scene* s);

// The stream-ordered scratch of one launch, dense (launch_on_stream) or listed (rt_adaptive_api.cpp): one block
// in rt_internal.h's layout (kLaunchScratchBytes) with the uniforms uploaded, and one band's partials when
// partial_bytes is not 0.  open sets kp.uni, kp.stack_cap and kp.task_ctr (the block's counter when there are
// partials and `queue` holds, else null); the caller runs its bands while e is hipSuccess, keeps the first
// failure in e and returns result().  Both blocks are freed in stream order when the scratch goes.
struct LaunchScratch : NoCopy {
    double* block = nullptr;
    double* partial = nullptr;
    hipStream_t st = nullptr;
    hipError_t e = hipSuccess;
    ~LaunchScratch()
    {
        if (partial) (void)hipFreeAsync(partial, st);
        if (block) (void)hipFreeAsync(block, st);
    }
    // RT_E* when the block itself could not be had (nothing was enqueued); a later failure is in e
    int open(KParams& kp, const double* uni, int stack_cap, size_t partial_bytes, bool queue, hipStream_t stream);
    int result(const char* what) const { return e == hipSuccess ? RT_OK : fail(RT_EDEVICE, "%s launch: %s", what, hipGetErrorString(e)); }
};

// rt_drop_in.cpp, for rt_shutdown
int scene_cache_clear();
void stream_pool_clear();

}  // namespace rt

struct rt_device_scene : rt::SceneArrays<rt::DevArray> {
    int device = 0;
    rt::SceneFacts facts;
};
