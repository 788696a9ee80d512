// rt_rccl.h — RCCL communicators and the frame gather (rt_rccl.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

namespace rt {

// Communicators over devs (rank q on device devs[q], ncclCommInitAll), made
// once per device list and kept until rccl_release.  0, or -1 with err set.
int rccl_comms(const std::vector<int>& devs, std::string& err);
// One ncclGather: `count` elements (doubles, or 32-bit words) from send[q] on
// devs[q] into recv on rank 0, q * count elements apart.
struct GatherPart {
    std::vector<const void*> send;
    void* recv = nullptr;
    size_t count = 0;
    bool words = false;          // ncclUint32 instead of ncclFloat64
};
// The parts' ncclGathers, rank q's on stream streams[q], every call of every
// rank in one group.  Enqueued only (stream-ordered).  0, or -1 with err set.
int rccl_gather(const std::vector<int>& devs, const std::vector<GatherPart>& parts,
                const std::vector<hipStream_t>& streams, std::string& err);
// The loaded library is the tests' stand-in (tests/stubs: it exports
// rt_rccl_stub_marker), whose ranks may share a device.  Loads the library on
// first use; false when it cannot be loaded.
bool rccl_ranks_may_share_a_device();
// Destroys the communicators (rt_shutdown).
void rccl_release();
// "RCCL x.y.z (path)" once loaded.
std::string rccl_describe();

}  // namespace rt
