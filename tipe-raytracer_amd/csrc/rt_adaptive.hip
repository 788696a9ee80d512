// rt_adaptive.hip — adaptive sampling's kernels (rt.h "adaptive sampling"):
//   * render_kernel_list / render_kernel_list_w: the fixed-grid render kernels
//     (rt_fixed_grid.h render_kernel / render_kernel_w) over a compacted list of
//     pixels instead of a dense row band; combine_list_kernel, their combine_kernel;
//   * the selection pass of rt_adaptive_select_async: per-pixel variance of the
//     two half-sample accumulators, the settled test, and the ordered compaction
//     of the pixels that go on (flags, block counts, one scan, a scatter);
//   * rt_resolve_adaptive_async's per-pixel resolve.
// A translation unit of its own that includes the device headers of
// rt_kernels.hip: that file's kernels keep their machine code.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "rt/rt.h"
#include "rt_internal.h"
#include "rt_bvh.h"
#include "rt_launch_plan.h"
#include "rt_device_math.h"
#include "rt_tunables.h"

#include "rt_vec.h"
#include "rt_spheres.h"
#include "rt_triangles.h"
#include "rt_shading.h"
#include "rt_fixed_grid.h"
#include "rt_denoise_tile.h"

namespace rt {

// ---- samples for listed pixels -------------------------------------------

// render_body (rt_fixed_grid.h) with one difference, the thread-to-pixel map:
// thread t of block b takes entry e = e0 + 256 b + t of the list, so a wave
// holds 64 consecutive entries; the list is ascending, which keeps a wave's
// pixels close together on screen.  The count is a device word; it is read
// once per wave through the scalar unit (a uniform address, read before any
// store of the kernel), and a block whose first entry is at or beyond it
// exits before it touches LDS.  Chunk partials are per entry of the band.
template <bool BVH, bool SKY, class SE = unsigned short>
__device__ __forceinline__ void list_body(const KParams& kp, const ListArgs& la)
{
    const unsigned end = min(*la.count, la.e1);
    const unsigned first = la.e0 + blockIdx.x * 256u;
    if (first >= end) return;
    const unsigned e = first + threadIdx.x;
    const int chunk = blockIdx.z;
    Cnt cnt;
    const uint32_t pixel = e < end ? la.list[e] : 0u;
    // (an index beyond the frame is not a pixel: skipped, nothing is written)
    if (e < end && pixel < (uint32_t)kp.W * (uint32_t)kp.H) {
        const int g = (int)(pixel / (uint32_t)kp.W), x = (int)(pixel - (uint32_t)g * (uint32_t)kp.W);
        const int s0 = chunk_start(kp.S, kp.chunks, kp.chunk_taper, kp.chunk_den, 0u, (unsigned)chunk);
        const int s1 = chunk_start(kp.S, kp.chunks, kp.chunk_taper, kp.chunk_den, 0u, (unsigned)chunk + 1u);
        __shared__ double acc_lds[ACC_SLOTS * 256];
        __shared__ uint32_t rng_lds[4 * 256];
        double* acc = acc_lds + threadIdx.x;
        const long long li = (long long)pixel;           // the whole-frame tiling: local pixel = global pixel
        // one chunk continues the running sums in sample order, as render_body's carry
        const bool carry = kp.chunks == 1;
#pragma unroll
        for (int j = 0; j < 9; ++j) acc[j * 256] = carry ? kp.sums[li * 9 + j] : 0.0;
        // where the sums go, fixed before the sample loop: the launch's scalars need not outlive it
        double* const p = carry ? kp.sums + li * 9
                                : la.partial + ((long long)chunk * la.stride + (long long)(e - la.e0)) * 9;
        if constexpr (BVH) {
            samples_coop<false, SKY, SE>(kp, x, g, pixel, s0, s1, rng_lds + threadIdx.x, acc, cnt);
        } else {
            samples_flat<false, SKY>(kp, x, g, pixel, s0, s1, rng_lds + threadIdx.x, acc, cnt);
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) p[j] = acc[j * 256];
    }
}

// The six instantiations: no tree, narrow tree, wide tree, each with the sky
// off and on, under their dense twins' launch bounds.
template <bool BVH, bool SKY>
__global__ __launch_bounds__(256, BVH ? RT_WAVES_PER_SIMD_BVH : RT_WAVES_PER_SIMD) void render_kernel_list(
    const KParams kp, const ListArgs la)
{
    list_body<BVH, SKY>(kp, la);
}
template <bool SKY>
__global__ __launch_bounds__(256, 2) void render_kernel_list_w(const KParams kp, const ListArgs la)
{
    list_body<true, SKY, uint32_t>(kp, la);
}

// combine_kernel's accumulate branch for a band of entries: the running sums
// of pixel list[e] plus the band's chunk partials of entry e, in chunk order.
__global__ __launch_bounds__(256) void combine_list_kernel(const ListArgs la, double* __restrict__ sums, int chunks,
                                                           unsigned npx)
{
    const unsigned end = min(*la.count, la.e1);
    for (unsigned long long e = (unsigned long long)la.e0 + blockIdx.x * 256u + threadIdx.x; e < end;
         e += (unsigned long long)gridDim.x * 256u) {
        const unsigned pixel = la.list[e];
        if (pixel >= npx) continue;
        double* s = sums + (long long)pixel * 9;
        double a[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) a[j] = s[j];
        for (int c = 0; c < chunks; ++c) {
            const double* q = la.partial + ((long long)c * la.stride + (long long)(e - la.e0)) * 9;
#pragma unroll
            for (int j = 0; j < 9; ++j) a[j] = a[j] + q[j];
        }
#pragma unroll
        for (int j = 0; j < 9; ++j) s[j] = a[j];
    }
}

// One entry band [la.e0, la.e1) of a list launch: the six-way pick from the
// plan's facts (plan_render decided tree, width and sky), then the combine.
int launch_render_list(const KParams& kp, const RenderPlan& pl, const ListArgs& la, void* stream)
{
    using K = void (*)(const KParams, const ListArgs);
    const K kernel = pl.wide  ? (pl.sky ? K(render_kernel_list_w<true>) : K(render_kernel_list_w<false>))
                     : pl.bvh ? (pl.sky ? K(render_kernel_list<true, true>) : K(render_kernel_list<true, false>))
                              : (pl.sky ? K(render_kernel_list<false, true>) : K(render_kernel_list<false, false>));
    const unsigned blocks = (la.e1 - la.e0 + 255u) / 256u;
    hipLaunchKernelGGL(kernel, dim3(blocks, 1, (unsigned)kp.chunks), dim3(256), 0, (hipStream_t)stream, kp, la);
    if (kp.chunks > 1) return launch_combine_list(kp, la, stream);
    return (int)hipGetLastError();
}

// The band's combine, for either render kernel (rt_queue_list.hip writes the same partials).
int launch_combine_list(const KParams& kp, const ListArgs& la, void* stream)
{
    const unsigned blocks = (la.e1 - la.e0 + 255u) / 256u;
    hipLaunchKernelGGL(combine_list_kernel, dim3(std::min(blocks, 8192u)), dim3(256), 0, (hipStream_t)stream, la,
                       kp.sums, kp.chunks, (unsigned)kp.W * (unsigned)kp.H);
    return (int)hipGetLastError();
}

// ---- selection and compaction --------------------------------------------

namespace {

constexpr unsigned kNone = 0xffffffffu;     // "settled" in the keep plane (a frame has at most 2^30 pixels)

// The active count: every pixel (round 0), or the incoming list's, clamped to the frame.
__device__ __forceinline__ unsigned active_count(const AdaptiveSelect& s)
{
    return s.all ? s.npx : min(*s.count, s.npx);
}

// v and y of every active pixel (rt.h), into their workspace planes.
__global__ __launch_bounds__(256) void adaptive_measure_kernel(const AdaptiveSelect s)
{
    const unsigned n = active_count(s);
    for (unsigned long long a = (unsigned long long)blockIdx.x * 256u + threadIdx.x; a < n;
         a += (unsigned long long)gridDim.x * 256u) {
        const unsigned p = s.all ? (unsigned)a : s.list[a];
        if (p >= s.npx) continue;
        const double* sa = s.sums_a + (long long)p * 9;
        const double* sb = s.sums_b + (long long)p * 9;
        float c[3], d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float ma = (float)(s.rap * sa[k]), mb = (float)(s.rap * sb[k]);
            c[k] = 0.5f * (ma + mb);
            d[k] = 0.5f * (ma - mb);
        }
        s.v[p] = lum2(d[0], d[1], d[2]);
        s.y[p] = (0.25f * c[0] + 0.5f * c[1]) + 0.25f * c[2];
    }
}

// Block b owns the active entries [256 b, 256 b + 256): the settled test of
// each (the 3x3 blur of the v plane as rt_vdenoise.hip's vdenoise_lum_kernel
// forms it), its round count, its keep word (the pixel, or kNone) and the
// block's number of kept entries.
__global__ __launch_bounds__(256) void adaptive_flag_kernel(const AdaptiveSelect s)
{
    __shared__ unsigned wcnt[4];
    const unsigned n = active_count(s);
    const unsigned base = blockIdx.x * 256u;
    if (base >= n) {                             // wave-uniform: nothing active here
        if (threadIdx.x == 0) s.counts[blockIdx.x] = 0u;
        return;
    }
    const unsigned a = base + threadIdx.x;
    unsigned p = kNone;
    bool keep = false;
    if (a < n) p = s.all ? a : s.list[a];
    if (p < s.npx) {
        const float g[3] = {0.25f, 0.5f, 0.25f};
        const int y = (int)(p / (unsigned)s.W), x = (int)(p - (unsigned)y * (unsigned)s.W);
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= s.H) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= s.W) continue;
                const float gg = g[dy + 1] * g[dx + 1];
                num += gg * s.v[(long long)qy * s.W + qx];
                den += gg;
            }
        }
        const float vb = num / den;
        const bool settled = vb <= ((4.0f * (s.tolerance * s.tolerance)) * (s.y[p] + 0x1p-8f));
        s.rounds[p] = s.round + 1;
        keep = !settled;                         // a NaN compares false: the pixel runs on
    }
    s.keep[a] = keep ? p : kNone;                // (the plane is padded to whole blocks)
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = (unsigned)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) s.counts[blockIdx.x] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
}

// Inclusive prefix sum over the wave's 64 lanes in DPP moves: within rows of
// 16 lanes by row_shr 1, 2, 4, 8 (a lane without a source adds 0), then the
// last lane of row 0 / 2 into the next row (row_bcast:15, rows 1 and 3) and of
// row 1 into rows 2 and 3 (row_bcast:31).
__device__ __forceinline__ unsigned wave_inclusive_sum(unsigned x)
{
    int v = (int)x;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    return (unsigned)v;
}

// Exclusive scan of the block counts, in place, by one block (1024 counts per
// step, the steps in order with a running carry); it then records the incoming
// count for the scatter and publishes the new one.  No block waits on another.
__global__ __launch_bounds__(1024) void adaptive_scan_kernel(const AdaptiveSelect s, unsigned nblk)
{
    __shared__ unsigned wsum[16];
    const unsigned n_in = active_count(s);       // read before the barriers below; written after them
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned carry = 0u;
    for (unsigned base = 0u; base < nblk; base += 1024u) {
        const unsigned i = base + threadIdx.x;
        const unsigned x = i < nblk ? s.counts[i] : 0u;
        const unsigned incl = wave_inclusive_sum(x);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned before = 0u, total = 0u;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const unsigned t = wsum[w];
            before += w < wave ? t : 0u;
            total += t;
        }
        if (i < nblk) s.counts[i] = carry + before + (incl - x);
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *s.n_in = n_in;
        *s.count = carry;
    }
}

// Block b writes its kept entries, in order, from its offset on.  It reads the
// keep plane and the recorded incoming count, never the list it overwrites.
__global__ __launch_bounds__(256) void adaptive_scatter_kernel(const AdaptiveSelect s)
{
    __shared__ unsigned wcnt[4];
    const unsigned n = *s.n_in;
    const unsigned base = blockIdx.x * 256u;
    if (base >= n) return;
    const unsigned a = base + threadIdx.x;
    const unsigned p = a < n ? s.keep[a] : kNone;
    const bool keep = p != kNone;
    const unsigned long long b = __ballot(keep);
    const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wcnt[wave] = (unsigned)__popcll(b);
    __syncthreads();
    unsigned before = 0u;
#pragma unroll
    for (int w = 0; w < 3; ++w) before += w < wave ? wcnt[w] : 0u;
    if (keep) s.list[s.counts[blockIdx.x] + before + rank] = p;
}

// d_rounds[p] = value for every active pixel (the loop's last round, which selects nothing).
__global__ __launch_bounds__(256) void adaptive_mark_kernel(const AdaptiveSelect s, int value)
{
    const unsigned n = active_count(s);
    for (unsigned long long a = (unsigned long long)blockIdx.x * 256u + threadIdx.x; a < n;
         a += (unsigned long long)gridDim.x * 256u) {
        const unsigned p = s.all ? (unsigned)a : s.list[a];
        if (p < s.npx) s.rounds[p] = value;
    }
}

// rt_resolve_adaptive_async: write_pixel's write_planes (rt_fixed_grid.h) on A + B with the
// pixel's own sample count 2 * first_half * 2^(k-1), k = rounds[p].
__global__ __launch_bounds__(256) void adaptive_resolve_kernel(long long npx, const double* __restrict__ sums_a,
                                                               const double* __restrict__ sums_b,
                                                               const int* __restrict__ rounds, int first_half,
                                                               double* __restrict__ canva, double* __restrict__ albedo,
                                                               double* __restrict__ normal,
                                                               double* __restrict__ radiance)
{
    for (long long px = (long long)blockIdx.x * blockDim.x + threadIdx.x; px < npx;
         px += (long long)gridDim.x * blockDim.x) {
        const int k = min(max(rounds[px], 1), 32);
        const double S = (double)((long long)first_half << k);
        double t[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) t[j] = sums_a[px * 9 + j] + sums_b[px * 9 + j];
        write_planes(canva, albedo, normal, radiance, px, S, v3(t[0], t[1], t[2]), v3(t[3], t[4], t[5]),
                     v3(t[6], t[7], t[8]));
    }
}

// Grid-stride kernels: 2048 blocks of 256 threads fill the 256 CUs (8 blocks each).
unsigned grid_1d(long long n) { return (unsigned)std::max(1ll, std::min((n + 255) / 256, 2048ll)); }

}  // namespace

unsigned adaptive_blocks(long long npx) { return (unsigned)((npx + 255) / 256); }

int launch_adaptive_select(const AdaptiveSelect& s, void* stream)
{
    const hipStream_t st = (hipStream_t)stream;
    const unsigned nblk = adaptive_blocks(s.npx);
    hipLaunchKernelGGL(adaptive_measure_kernel, dim3(grid_1d(s.npx)), dim3(256), 0, st, s);
    hipLaunchKernelGGL(adaptive_flag_kernel, dim3(nblk), dim3(256), 0, st, s);
    hipLaunchKernelGGL(adaptive_scan_kernel, dim3(1), dim3(1024), 0, st, s, nblk);
    hipLaunchKernelGGL(adaptive_scatter_kernel, dim3(nblk), dim3(256), 0, st, s);
    return (int)hipGetLastError();
}

int launch_adaptive_mark(const AdaptiveSelect& s, int value, void* stream)
{
    hipLaunchKernelGGL(adaptive_mark_kernel, dim3(grid_1d(s.npx)), dim3(256), 0, (hipStream_t)stream, s, value);
    return (int)hipGetLastError();
}

int launch_adaptive_resolve(long long npx, const double* sums_a, const double* sums_b, const int* rounds,
                            int first_half, double* canva, double* albedo, double* normal, double* radiance,
                            void* stream)
{
    hipLaunchKernelGGL(adaptive_resolve_kernel, dim3(grid_1d(npx)), dim3(256), 0, (hipStream_t)stream, npx, sums_a,
                       sums_b, rounds, first_half, canva, albedo, normal, radiance);
    return (int)hipGetLastError();
}

}  // namespace rt
