// rt_pack.h — the packed canva (rt.h "packed canva transport"): one 32-bit
// word per pixel, f0 | f1 << 9 | f2 << 18.  The field arithmetic, shared by the
// kernels (rt_pack.hip) and rt_canva_unpack_host, and the launchers.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RT_PACK_FN __host__ __device__ inline
#else
#define RT_PACK_FN inline
#endif

namespace rt {

constexpr unsigned kPackMarker = 256;              // the field of every value that is not an integer 0..255
constexpr long long kPackMaxPixels = 1LL << 30;    // n of the pack entry points

// Field of one canva channel: v itself for +0.0, 1.0, ..., 255.0, else the
// marker (NaN, a fraction, -0.0, anything outside 0..255).  The comparison of
// the bit patterns is what tells -0.0 from +0.0.
RT_PACK_FN unsigned pack_field(double v)
{
    if (!(v >= 0.0 && v <= 255.0)) return kPackMarker;
    const int i = (int)v;
    const double back = (double)i;
    uint64_t a, b;
    memcpy(&a, &back, 8);
    memcpy(&b, &v, 8);
    return a == b ? (unsigned)i : kPackMarker;
}

// Channel k of a packed word: fields 0..255 are the value, every other field
// (the marker 256, and 257..511, which no pack writes) is -2147483648.0, what
// write_color_canva stores for a NaN radiance.  Bits 27..31 are not read.
RT_PACK_FN double unpack_field(unsigned w, int k)
{
    const unsigned f = (w >> (9 * k)) & 0x1ffu;
    return f < kPackMarker ? (double)(int)f : -2147483648.0;
}

// launchers (rt_pack.hip); each returns the launch's hipError_t
int launch_canva_pack(long long n, const double* canva, unsigned* packed, void* stream);
int launch_canva_unpack(long long n, const unsigned* packed, double* canva, void* stream);
// launch_assemble's un-permute (rt_kernels.hip) on a rank-major staging of
// packed words, rank_stride in pixels, widened into out (W*H colours).
int launch_assemble_packed(const unsigned* gathered, long long rank_stride, int world, int tile_rows,
                           int rows_per_rank, int W, int H, double* out, void* stream);

// rt_set_fill_packed_canva's switch (rt_pack_api.cpp), read by rt_render_rows.
bool fill_packed_canva();

}  // namespace rt
