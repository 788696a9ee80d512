// rt_pack.hip — the packed canva's kernels (rt.h "packed canva transport"):
// a canva channel is one of 257 values (an integer 0..255, or the marker
// -2147483648.0 of a NaN radiance), so a pixel travels as one 32-bit word
// instead of three doubles.  pack and unpack are the two directions; the
// assemble form is assemble_kernel's un-permute (rt_kernels.hip) of a
// rank-major gather, reading words and writing the widened colours.
//
// All three stream: one pixel per thread per grid-stride step, 28 bytes of
// traffic per pixel (the 24 B of a colour on one side, which the compiler
// moves as one 16-byte and one 8-byte access per lane, adjacent lanes
// contiguous, and one coalesced 4-byte word on the other), no LDS, no scratch.
#include <hip/hip_runtime.h>

#include "rt_pack.h"

namespace rt {

namespace {

// Grid-stride kernels: 2048 blocks of 256 threads fill the 256 CUs (8 blocks each).
unsigned grid_1d(long long n) { return (unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048); }

__device__ __forceinline__ void store_unpacked(double* __restrict__ dst, unsigned w)
{
    dst[0] = unpack_field(w, 0);
    dst[1] = unpack_field(w, 1);
    dst[2] = unpack_field(w, 2);
}

}  // namespace

__global__ __launch_bounds__(256) void canva_pack_kernel(long long n, const double* __restrict__ canva,
                                                         unsigned* __restrict__ packed)
{
    for (long long px = (long long)blockIdx.x * blockDim.x + threadIdx.x; px < n;
         px += (long long)gridDim.x * blockDim.x) {
        const double* c = canva + px * 3;
        packed[px] = pack_field(c[0]) | pack_field(c[1]) << 9 | pack_field(c[2]) << 18;
    }
}

__global__ __launch_bounds__(256) void canva_unpack_kernel(long long n, const unsigned* __restrict__ packed,
                                                           double* __restrict__ canva)
{
    for (long long px = (long long)blockIdx.x * blockDim.x + threadIdx.x; px < n;
         px += (long long)gridDim.x * blockDim.x)
        store_unpacked(canva + px * 3, packed[px]);
}

// Pixel (g, i) of the frame is row lt*tile_rows + y of rank r's block, with
// tile t = g / tile_rows = lt*world + r (rt.h rt_tiling); the blocks' padding
// rows (frame rows >= H) are never read.
__global__ __launch_bounds__(256) void assemble_packed_kernel(const unsigned* __restrict__ gathered,
                                                              long long rank_stride, int world, int tile_rows,
                                                              int rows_per_rank, int W, int H,
                                                              double* __restrict__ out)
{
    const long long n = (long long)W * H;
    for (long long px = (long long)blockIdx.x * blockDim.x + threadIdx.x; px < n;
         px += (long long)gridDim.x * blockDim.x) {
        const int g = (int)(px / W), i = (int)(px - (long long)g * W);
        const int t = g / tile_rows, y = g - t * tile_rows;
        const int r = t % world, lt = t / world;
        const long long src = (long long)r * rank_stride + ((long long)lt * tile_rows + y) * W + i;
        store_unpacked(out + px * 3, gathered[src]);
    }
}

int launch_canva_pack(long long n, const double* canva, unsigned* packed, void* stream)
{
    hipLaunchKernelGGL(canva_pack_kernel, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, n, canva, packed);
    return (int)hipGetLastError();
}

int launch_canva_unpack(long long n, const unsigned* packed, double* canva, void* stream)
{
    hipLaunchKernelGGL(canva_unpack_kernel, dim3(grid_1d(n)), dim3(256), 0, (hipStream_t)stream, n, packed, canva);
    return (int)hipGetLastError();
}

int launch_assemble_packed(const unsigned* gathered, long long rank_stride, int world, int tile_rows,
                           int rows_per_rank, int W, int H, double* out, void* stream)
{
    hipLaunchKernelGGL(assemble_packed_kernel, dim3(grid_1d((long long)W * H)), dim3(256), 0, (hipStream_t)stream,
                       gathered, rank_stride, world, tile_rows, rows_per_rank, W, H, out);
    return (int)hipGetLastError();
}

}  // namespace rt
