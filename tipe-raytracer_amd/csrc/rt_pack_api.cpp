// rt_pack_api.cpp — the packed canva's entry points (rt.h "packed canva
// transport"): the device pack and unpack on the caller's stream, the host
// unpack, and the drop-ins' switch.  rt_assemble_packed_async is with the
// other assemble in rt_gather.cpp.
#include <atomic>
#include <cstdint>

#include "rt_api_internal.h"
#include "rt_pack.h"

using namespace rt;

namespace {

std::atomic<int> g_fill_packed{0};     // rt_set_fill_packed_canva

int check_pack_args(long long n, const void* canva, const void* packed)
{
    if (!canva || !packed) return fail(RT_EINVAL, "NULL buffer");
    if (n < 1 || n > kPackMaxPixels) return fail(RT_EINVAL, "%lld pixels outside [1, 2^30]", n);
    if ((uintptr_t)packed % 4) return fail(RT_EINVAL, "packed canva is not 4-byte aligned");
    return RT_OK;
}

}  // namespace

bool rt::fill_packed_canva() { return g_fill_packed.load() != 0; }

extern "C" {

int rt_canva_pack_async(long long n, const rt_color* canva, unsigned* packed, void* hip_stream)
{
    int rc;
    if ((rc = check_pack_args(n, canva, packed))) return rc;
    const int e = launch_canva_pack(n, (const double*)canva, packed, hip_stream);
    if (e) return fail(RT_EDEVICE, "pack launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

int rt_canva_unpack_async(long long n, const unsigned* packed, rt_color* canva, void* hip_stream)
{
    int rc;
    if ((rc = check_pack_args(n, canva, packed))) return rc;
    const int e = launch_canva_unpack(n, packed, (double*)canva, hip_stream);
    if (e) return fail(RT_EDEVICE, "unpack launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

int rt_canva_unpack_host(long long n, const unsigned* packed, rt_color* canva)
{
    int rc;
    if ((rc = check_pack_args(n, canva, packed))) return rc;
    double* out = (double*)canva;
    for (long long px = 0; px < n; ++px) {
        const unsigned w = packed[px];
        out[px * 3 + 0] = unpack_field(w, 0);
        out[px * 3 + 1] = unpack_field(w, 1);
        out[px * 3 + 2] = unpack_field(w, 2);
    }
    return RT_OK;
}

int rt_set_fill_packed_canva(int enable) { return g_fill_packed.exchange(enable ? 1 : 0); }

}  // extern "C"
