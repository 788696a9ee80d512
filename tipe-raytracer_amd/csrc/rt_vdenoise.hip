// rt_vdenoise.hip — the variance-guided radiance denoiser's kernels: the
// filter rt.h specifies operation by operation ("variance-guided denoiser")
// over two half-sample accumulators of rt_accumulate_async.  Every + - * /
// below is one IEEE binary32 rounding in rt.h's order (-ffp-contract=off; the
// kernels' float mode keeps f32 subnormals and the divisions are correctly
// rounded), "double" where rt.h says double, so a float32 restatement of
// rt.h equals these kernels bit for bit.
//
// Private workspace (rt_vdenoise_workspace_bytes), in floats, npx = W*H:
//   colour ping | colour pong | albedo | normal   float3 planes, denoise_plane_floats(npx) each
//   variance ping | variance pong | L              one float per pixel, vdenoise_scalar_floats(npx) each
#include <hip/hip_runtime.h>

#include "rt_denoise_tile.h"
#include "rt_internal.h"

namespace rt {

namespace {

// Grid-stride kernels: 2048 blocks of 256 threads fill the 256 CUs (8 blocks each).
unsigned grid_1d(long long n) { return (unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048); }

// n_p of rt.h "per-pixel sample counts": first_half * 2^(k-1) samples per
// accumulator, k = rounds[px] under adaptive_resolve_kernel's clamp (rt_adaptive.hip)
__device__ __forceinline__ double pixel_count(const int* __restrict__ rounds, long long px, int first_half)
{
    const int k = min(max(rounds[px], 1), 32);
    return (double)((long long)first_half << (k - 1));
}

// What pixel px's sums are scaled by, from the count arguments N... of the prepare
// and finish kernels.  <double>: every pixel holds n samples per accumulator and
// the host passes the reciprocal, 1.0 / n (prepare) or 1.0 / (2 n) (finish).
// <const int* __restrict__, int>: rounds and first_half, n_p per pixel -- one more
// 4-byte load and one double division.  (The arguments stay a pack and the loops
// stay in the kernels: a struct of the two costs the per-pixel forms two
// instructions, a device function around the loop the uniform forms a VGPR.)
__device__ __forceinline__ double mean_scale(long long, double rap) { return rap; }
__device__ __forceinline__ double mean_scale(long long px, const int* __restrict__ rounds, int first_half)
{
    return 1.0 / pixel_count(rounds, px, first_half);
}
__device__ __forceinline__ double sum_scale(long long, double rap2) { return rap2; }
__device__ __forceinline__ double sum_scale(long long px, const int* __restrict__ rounds, int first_half)
{
    return 1.0 / (2.0 * pixel_count(rounds, px, first_half));
}

// the two accumulators -> the planes c, v, a, nn
template <class... N>
__global__ __launch_bounds__(256) void vdenoise_prepare_kernel(long long npx, const double* __restrict__ sums_a,
                                                               const double* __restrict__ sums_b, const N... n,
                                                               float* __restrict__ c3, float* __restrict__ v1,
                                                               float* __restrict__ a3, float* __restrict__ n3)
{
    for (long long px = (long long)blockIdx.x * blockDim.x + threadIdx.x; px < npx;
         px += (long long)gridDim.x * blockDim.x) {
        const double rap = mean_scale(px, n...);
        const double* sa = sums_a + px * 9;
        const double* sb = sums_b + px * 9;
        float ma[9], mb[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            ma[k] = (float)(rap * sa[k]);
            mb[k] = (float)(rap * sb[k]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c3[px * 3 + k] = 0.5f * (ma[k] + mb[k]);
            a3[px * 3 + k] = 0.5f * (ma[3 + k] + mb[3 + k]);
            n3[px * 3 + k] = 0.5f * (ma[6 + k] + mb[6 + k]);
        }
        v1[px] = lum2(0.5f * (ma[0] - mb[0]), 0.5f * (ma[1] - mb[1]), 0.5f * (ma[2] - mb[2]));
    }
}

// L = sl2 * (3x3 blur of v at step 1) + 2^-26, one pixel per thread.  A kernel
// of its own: the step-1 neighbours are not in a step-s tile of the pass.
__global__ __launch_bounds__(256) void vdenoise_lum_kernel(int W, int H, float sl2, const float* __restrict__ v,
                                                           float* __restrict__ L)
{
    const float g[3] = {0.25f, 0.5f, 0.25f};
    const long long npx = (long long)W * H;
    for (long long px = (long long)blockIdx.x * blockDim.x + threadIdx.x; px < npx;
         px += (long long)gridDim.x * blockDim.x) {
        const int y = (int)((unsigned)px / (unsigned)W), x = (int)px - y * W;     // npx <= 2^30
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= H) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= W) continue;
                const float gg = g[dy + 1] * g[dx + 1];
                num += gg * v[(long long)qy * W + qx];
                den += gg;
            }
        }
        L[px] = sl2 * (num / den) + 0x1p-26f;
    }
}

struct Tap {
    F3 c;
    float v;
    F3 n, a;
};

// One pixel of one pass in rt.h's operation order.  fetch(dy, dx, qx, qy)
// returns the planes at the tap (qx, qy) = (x, y) + step * (dx, dy), which
// lies inside the image.  One division per tap; the only per-lane branch in
// the tap loop is the image-bounds skip.
template <class Fetch>
__device__ __forceinline__ void vfilter_pixel(int W, int H, int x, int y, int step, float sn2, float sa2,
                                              const float* __restrict__ Lp, const Fetch& fetch,
                                              float* __restrict__ cout, float* __restrict__ vout)
{
    const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const long long px = (long long)y * W + x;
    const float L = Lp[px];
    const float snsa = sn2 * sa2;
    const Tap p = fetch(0, 0, x, y);
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, accv = 0.0f, ws = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + step * dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + step * dx;
            if (qx < 0 || qx >= W) continue;
            const Tap q = fetch(dy, dx, qx, qy);
            const float dl = lum2(q.c.x - p.c.x, q.c.y - p.c.y, q.c.z - p.c.z);
            const float dn = dist2(q.n, p.n), da = dist2(q.a, p.a);
            const float num = ((h[dy + 2] * h[dx + 2]) * L) * snsa;
            const float den = ((L + dl) * (sn2 + dn)) * (sa2 + da);
            const float w = num / den;
            acc0 += w * q.c.x;
            acc1 += w * q.c.y;
            acc2 += w * q.c.z;
            accv += (w * w) * q.v;
            ws += w;
        }
    }
    float* o = cout + px * 3;
    o[0] = acc0 / ws;
    o[1] = acc1 / ws;
    o[2] = acc2 / ws;
    vout[px] = accv / (ws * ws);
}

// One pass, plain form: one thread per pixel, every tap a global load.
// Serves the steps above kTiledMaxStep.
__global__ __launch_bounds__(kTileX* kTileY) void vdenoise_pass_kernel(int W, int H, int step, float sn2, float sa2,
                                                                       const float* __restrict__ cin,
                                                                       const float* __restrict__ vin,
                                                                       const float* __restrict__ alb,
                                                                       const float* __restrict__ nrm,
                                                                       const float* __restrict__ Lp,
                                                                       float* __restrict__ cout,
                                                                       float* __restrict__ vout)
{
    const unsigned nbx = (unsigned)((W + kTileX - 1) / kTileX);
    const int x = (int)(blockIdx.x % nbx) * kTileX + (int)threadIdx.x;
    const int y = (int)(blockIdx.x / nbx) * kTileY + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const auto fetch = [=](int, int, int qx, int qy) {
        const long long g = (long long)qy * W + qx;
        return Tap{ld3(cin, g), vin[g], ld3(nrm, g), ld3(alb, g)};
    };
    vfilter_pixel(W, H, x, y, step, sn2, sa2, Lp, fetch, cout, vout);
}

// One pass, tiled form (steps up to kTiledMaxStep), laid out as
// denoise_pass_tiled_kernel (rt_denoise.hip): a block owns 64 contiguous x and
// the kTileY rows r + (m0 + j) * step of one residue class r, stages
// kTiledRows rows of 64 + 4 * step pixels in LDS once, one plane of floats per
// channel (conflict-free ds_read_b32), and serves all 25 taps from there.  Ten
// channels per staged pixel (c, v, nn, a): 40 KiB of LDS at step 16.
constexpr int kTiledMaxStep = 16;
constexpr int kChannels = 10;
inline size_t tiled_lds_bytes(int step) { return (size_t)kChannels * kTiledRows * (kTileX + 4 * step) * sizeof(float); }

__global__ __launch_bounds__(kTileX* kTileY) void vdenoise_pass_tiled_kernel(int W, int H, int step, float sn2,
                                                                             float sa2, const float* __restrict__ cin,
                                                                             const float* __restrict__ vin,
                                                                             const float* __restrict__ alb,
                                                                             const float* __restrict__ nrm,
                                                                             const float* __restrict__ Lp,
                                                                             float* __restrict__ cout,
                                                                             float* __restrict__ vout)
{
    extern __shared__ float tile[];      // [channel][kTiledRows][wt]: c0 c1 c2 v n0 n1 n2 a0 a1 a2
    const int wt = kTileX + 4 * step;
    const int chan = kTiledRows * wt;    // floats of one channel
    const unsigned nbx = (unsigned)((W + kTileX - 1) / kTileX);
    const int x0 = (int)(blockIdx.x % nbx) * kTileX;
    const unsigned t = blockIdx.x / nbx;
    const int r = (int)(t % (unsigned)step), m0 = (int)(t / (unsigned)step) * kTileY;
    const int tid = (int)threadIdx.y * kTileX + (int)threadIdx.x;
    for (int i = tid; i < chan; i += kTileX * kTileY) {
        const int row = i / wt, col = i - row * wt;
        const int gx = x0 - 2 * step + col, gy = r + (m0 - 2 + row) * step;
        if (gx < 0 || gx >= W || gy < 0 || gy >= H) continue;      // never read: the same test skips the tap
        const long long g = (long long)gy * W + gx;
        const F3 c = ld3(cin, g), n = ld3(nrm, g), a = ld3(alb, g);
        tile[i] = c.x, tile[chan + i] = c.y, tile[2 * chan + i] = c.z;
        tile[3 * chan + i] = vin[g];
        tile[4 * chan + i] = n.x, tile[5 * chan + i] = n.y, tile[6 * chan + i] = n.z;
        tile[7 * chan + i] = a.x, tile[8 * chan + i] = a.y, tile[9 * chan + i] = a.z;
    }
    __syncthreads();
    const int x = x0 + (int)threadIdx.x, y = r + (m0 + (int)threadIdx.y) * step;
    if (x >= W || y >= H) return;
    const int centre = ((int)threadIdx.y + 2) * wt + (int)threadIdx.x + 2 * step;
    const auto fetch = [=](int dy, int dx, int, int) {
        const float* q = tile + centre + dy * wt + dx * step;
        return Tap{F3{q[0], q[chan], q[2 * chan]}, q[3 * chan], F3{q[4 * chan], q[5 * chan], q[6 * chan]},
                   F3{q[7 * chan], q[8 * chan], q[9 * chan]}};
    };
    vfilter_pixel(W, H, x, y, step, sn2, sa2, Lp, fetch, cout, vout);
}

// (int) of a double as write_pixel takes it (rt_vec.h cvt_i32_x86: the
// reference's x86-64 cvttsd2si, NaN and out-of-range values give INT_MIN)
__device__ __forceinline__ int cvt_i32_x86(double x)
{
    return (x > -2147483649.0 && x < 2147483648.0) ? (int)x : (int)0x80000000u;
}

// filtered colour -> canva = write_color_canva((double)c, 1) (rtutility.h:56-71,
// as write_pixel), radiance = (double)c; albedo / normal = (A + B) * rap2
template <class... N>
__global__ __launch_bounds__(256) void vdenoise_finish_kernel(long long npx, const float* __restrict__ c3,
                                                              const double* __restrict__ sums_a,
                                                              const double* __restrict__ sums_b, const N... n,
                                                              double* __restrict__ canva, double* __restrict__ albedo,
                                                              double* __restrict__ normal,
                                                              double* __restrict__ radiance)
{
    for (long long px = (long long)blockIdx.x * blockDim.x + threadIdx.x; px < npx;
         px += (long long)gridDim.x * blockDim.x) {
        const double rap2 = sum_scale(px, n...);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float c = c3[px * 3 + k];
            double r = (double)sqrtf(c);
            r = r < 0.0 ? 0.0 : (r > 0.999 ? 0.999 : r);
            canva[px * 3 + k] = (double)cvt_i32_x86(256 * r);
            if (radiance) radiance[px * 3 + k] = (double)c;
            if (albedo) albedo[px * 3 + k] = (sums_a[px * 9 + 3 + k] + sums_b[px * 9 + 3 + k]) * rap2;
            if (normal) normal[px * 3 + k] = (sums_a[px * 9 + 6 + k] + sums_b[px * 9 + 6 + k]) * rap2;
        }
    }
}

}  // namespace

size_t vdenoise_scalar_floats(long long npx) { return ((size_t)npx + 63) / 64 * 64; }

// rounds null: spp_half samples per accumulator in every pixel; else the per-pixel forms of prepare and
// finish with first_half = spp_half.  Between the two the filter does not know the counts.
int launch_vdenoise(int W, int H, const double* sums_a, const double* sums_b, const int* rounds, int spp_half,
                    int iterations, float sigma_luminance, float sigma_normal, float sigma_albedo, float* workspace,
                    double* canva, double* albedo, double* normal, double* radiance, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    const long long npx = (long long)W * H;
    const size_t plane3 = denoise_plane_floats(npx), plane1 = vdenoise_scalar_floats(npx);
    float* c[2] = {workspace, workspace + plane3};
    float* a3 = workspace + 2 * plane3;
    float* n3 = workspace + 3 * plane3;
    float* v[2] = {workspace + 4 * plane3, workspace + 4 * plane3 + plane1};
    float* L = workspace + 4 * plane3 + 2 * plane1;
    const double n = (double)spp_half;
    if (rounds)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(vdenoise_prepare_kernel<const int* __restrict__, int>), dim3(grid_1d(npx)),
                           dim3(256), 0, st, npx, sums_a, sums_b, rounds, spp_half, c[0], v[0], a3, n3);
    else
        hipLaunchKernelGGL(vdenoise_prepare_kernel<double>, dim3(grid_1d(npx)), dim3(256), 0, st, npx, sums_a, sums_b,
                           1.0 / n, c[0], v[0], a3, n3);
    const float sl2 = sigma_luminance * sigma_luminance, sn2 = sigma_normal * sigma_normal,
                sa2 = sigma_albedo * sigma_albedo;
    const unsigned nbx = (unsigned)((W + kTileX - 1) / kTileX);
    for (int i = 0; i < iterations; ++i) {
        const int step = 1 << i, in = i & 1, out = (i + 1) & 1;
        hipLaunchKernelGGL(vdenoise_lum_kernel, dim3(grid_1d(npx)), dim3(256), 0, st, W, H, sl2, v[in], L);
        if (step <= kTiledMaxStep) {
            // per residue class r < step: ceil(H / step) rows, kTileY per block
            const unsigned nby = (unsigned)step * (unsigned)(((H + step - 1) / step + kTileY - 1) / kTileY);
            hipLaunchKernelGGL(vdenoise_pass_tiled_kernel, dim3(nbx * nby), dim3(kTileX, kTileY),
                               tiled_lds_bytes(step), st, W, H, step, sn2, sa2, c[in], v[in], a3, n3, L, c[out],
                               v[out]);
        } else {
            const unsigned blocks = nbx * (unsigned)((H + kTileY - 1) / kTileY);
            hipLaunchKernelGGL(vdenoise_pass_kernel, dim3(blocks), dim3(kTileX, kTileY), 0, st, W, H, step, sn2, sa2,
                               c[in], v[in], a3, n3, L, c[out], v[out]);
        }
    }
    if (rounds)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(vdenoise_finish_kernel<const int* __restrict__, int>), dim3(grid_1d(npx)),
                           dim3(256), 0, st, npx, c[iterations & 1], sums_a, sums_b, rounds, spp_half, canva, albedo, normal, radiance);
    else
        hipLaunchKernelGGL(vdenoise_finish_kernel<double>, dim3(grid_1d(npx)), dim3(256), 0, st, npx, c[iterations & 1],
                           sums_a, sums_b, 1.0 / (2.0 * n), canva, albedo, normal, radiance);
    return (int)hipGetLastError();
}

}  // namespace rt
