// rt_denoise.hip — the built-in denoiser's kernels: the edge-avoiding a-trous
// wavelet filter rt.h specifies operation by operation ("built-in denoiser").
// Not OIDN.  Every + - * / below is one IEEE binary32 rounding in rt.h's
// order (-ffp-contract=off; the kernels' float mode keeps f32 subnormals and
// the divisions are correctly rounded), so a float32 restatement of rt.h
// equals these kernels bit for bit.
//
// Private workspace (rt_denoise_workspace_bytes): four planes of float3 per
// pixel, each denoise_plane_floats(npx) floats: colour ping | colour pong |
// albedo | normal.
#include <hip/hip_runtime.h>

#include "rt_denoise_tile.h"
#include "rt_internal.h"

namespace rt {

namespace {

// k(x) = 1 / (1 + x)
__device__ __forceinline__ float kern(const float x) { return 1.0f / (1.0f + x); }

// planes -> the workspace's float3 planes (the pack's operations)
__global__ __launch_bounds__(256) void denoise_prepare_kernel(long long n, const double* __restrict__ canva,
                                                              const double* __restrict__ albedo,
                                                              const double* __restrict__ normal,
                                                              float* __restrict__ c3, float* __restrict__ a3,
                                                              float* __restrict__ n3)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        c3[i] = (float)canva[i] / 255.0f;
        if (albedo) a3[i] = (float)albedo[i];
        if (normal) n3[i] = (float)normal[i];
    }
}

// One pixel of one a-trous pass in rt.h's operation order.  fetch(plane, dy,
// dx, qx, qy) returns plane 0 (colour) / 1 (normal) / 2 (albedo) at the tap
// (qx, qy) = (x, y) + step * (dx, dy), which lies inside the image.
template <bool ALB, bool NRM, class Fetch>
__device__ __forceinline__ void filter_pixel(int W, int H, int x, int y, int step, float sig_c, float sig_n,
                                             float sig_a, const Fetch& fetch, float* __restrict__ cout)
{
    const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const float sc2 = sig_c * sig_c, sn2 = sig_n * sig_n, sa2 = sig_a * sig_a;
    const F3 cp = fetch(0, 0, 0, x, y);
    F3 ap = {0.0f, 0.0f, 0.0f}, np = {0.0f, 0.0f, 0.0f};
    if (NRM) np = fetch(1, 0, 0, x, y);
    if (ALB) ap = fetch(2, 0, 0, x, y);
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, ws = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + step * dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + step * dx;
            if (qx < 0 || qx >= W) continue;
            const F3 cq = fetch(0, dy, dx, qx, qy);
            float w = (h[dy + 2] * h[dx + 2]) * kern(dist2(cq, cp) / sc2);
            if (NRM) w = w * kern(dist2(fetch(1, dy, dx, qx, qy), np) / sn2);
            if (ALB) w = w * kern(dist2(fetch(2, dy, dx, qx, qy), ap) / sa2);
            acc0 += w * cq.x;
            acc1 += w * cq.y;
            acc2 += w * cq.z;
            ws += w;
        }
    }
    float* o = cout + ((long long)y * W + x) * 3;
    o[0] = acc0 / ws;
    o[1] = acc1 / ws;
    o[2] = acc2 / ws;
}

// One a-trous pass, plain form: one thread per pixel, every tap a global
// load (a wave's 64 pixels read 64 contiguous float3 per tap row).  Serves
// the steps above kTiledMaxStep, and is the measuring stick of the tiled form
// (DESIGN.md "Built-in denoiser").
template <bool ALB, bool NRM>
__global__ __launch_bounds__(kTileX* kTileY) void denoise_pass_kernel(int W, int H, int step, float sig_c, float sig_n,
                                                                      float sig_a, const float* __restrict__ cin,
                                                                      const float* __restrict__ alb,
                                                                      const float* __restrict__ nrm,
                                                                      float* __restrict__ cout)
{
    const unsigned nbx = (unsigned)((W + kTileX - 1) / kTileX);
    const int x = (int)(blockIdx.x % nbx) * kTileX + (int)threadIdx.x;
    const int y = (int)(blockIdx.x / nbx) * kTileY + (int)threadIdx.y;
    if (x >= W || y >= H) return;
    const auto fetch = [=](int plane, int, int, int qx, int qy) {
        return ld3(plane == 0 ? cin : plane == 1 ? nrm : alb, (long long)qy * W + qx);
    };
    filter_pixel<ALB, NRM>(W, H, x, y, step, sig_c, sig_n, sig_a, fetch, cout);
}

// One a-trous pass, tiled form (steps up to kTiledMaxStep): a block owns 64
// contiguous x and the kTileY rows r + (m0 + j) * step, so the y-taps of its
// pixels are its own rows and their neighbours in the same residue class r:
// kTileY + 4 rows of 64 + 4 * step contiguous pixels go through LDS once
// (coalesced loads, one plane of floats per channel: conflict-free reads) and
// serve all 25 taps.  Measured at 10-15 % less time than the plain form at every
// step 1..16 (1200x900 and 3840x2880; profiles/denoise); both forms are bound
// by the 153 correctly rounded divisions per pixel, not by memory.
// kTiledMaxStep = 0 selects the plain form everywhere (the A/B of that
// measurement).  Step 16 uses 36 KiB of LDS with both guide planes.
constexpr int kTiledMaxStep = 16;
inline size_t tiled_lds_bytes(int step, int planes) { return (size_t)planes * 3 * kTiledRows * (kTileX + 4 * step) * sizeof(float); }

template <bool ALB, bool NRM>
__global__ __launch_bounds__(kTileX* kTileY) void denoise_pass_tiled_kernel(int W, int H, int step, float sig_c,
                                                                            float sig_n, float sig_a,
                                                                            const float* __restrict__ cin,
                                                                            const float* __restrict__ alb,
                                                                            const float* __restrict__ nrm,
                                                                            float* __restrict__ cout)
{
    extern __shared__ float tile[];      // [plane][channel][kTiledRows][wt]
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
        const F3 c = ld3(cin, g);
        tile[i] = c.x, tile[chan + i] = c.y, tile[2 * chan + i] = c.z;
        if (NRM) {
            const F3 n = ld3(nrm, g);
            tile[3 * chan + i] = n.x, tile[4 * chan + i] = n.y, tile[5 * chan + i] = n.z;
        }
        if (ALB) {
            const F3 a = ld3(alb, g);
            float* ta = tile + (NRM ? 6 : 3) * chan;
            ta[i] = a.x, ta[chan + i] = a.y, ta[2 * chan + i] = a.z;
        }
    }
    __syncthreads();
    const int x = x0 + (int)threadIdx.x, y = r + (m0 + (int)threadIdx.y) * step;
    if (x >= W || y >= H) return;
    const int centre = ((int)threadIdx.y + 2) * wt + (int)threadIdx.x + 2 * step;
    const auto fetch = [=](int plane, int dy, int dx, int, int) {
        const float* q = tile + (plane == 0 ? 0 : plane == 1 ? 3 : (NRM ? 6 : 3)) * chan + centre + dy * wt + dx * step;
        return F3{q[0], q[chan], q[2 * chan]};
    };
    filter_pixel<ALB, NRM>(W, H, x, y, step, sig_c, sig_n, sig_a, fetch, cout);
}

// filtered colour -> canva = (double)(int)(c * 255.0f) (denoiser.h:80-84), and
// the unquantised colour into color3 when asked for
__global__ __launch_bounds__(256) void denoise_finish_kernel(long long n, const float* __restrict__ c3,
                                                             double* __restrict__ canva, float* __restrict__ color3)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float c = c3[i];
        canva[i] = (double)(int)(c * 255.0f);
        if (color3) color3[i] = c;
    }
}

unsigned grid_1d(long long n) { return (unsigned)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192); }

template <bool ALB, bool NRM>
void launch_pass(int W, int H, int step, float sig_c, float sig_n, float sig_a, const float* cin, const float* alb,
                 const float* nrm, float* cout, hipStream_t st)
{
    const unsigned nbx = (unsigned)((W + kTileX - 1) / kTileX);
    if (step <= kTiledMaxStep) {
        // per residue class r < step: ceil(H / step) rows, kTileY per block
        const unsigned nby = (unsigned)step * (unsigned)(((H + step - 1) / step + kTileY - 1) / kTileY);
        hipLaunchKernelGGL((denoise_pass_tiled_kernel<ALB, NRM>), dim3(nbx * nby), dim3(kTileX, kTileY),
                           tiled_lds_bytes(step, 1 + ALB + NRM), st, W, H, step, sig_c, sig_n, sig_a, cin, alb, nrm,
                           cout);
        return;
    }
    const unsigned blocks = nbx * (unsigned)((H + kTileY - 1) / kTileY);
    hipLaunchKernelGGL((denoise_pass_kernel<ALB, NRM>), dim3(blocks), dim3(kTileX, kTileY), 0, st, W, H, step, sig_c,
                       sig_n, sig_a, cin, alb, nrm, cout);
}

}  // namespace

size_t denoise_plane_floats(long long npx) { return ((size_t)npx * 3 + 63) / 64 * 64; }

int launch_denoise(int W, int H, double* canva, const double* albedo, const double* normal, int iterations,
                   float sigma_color, float sigma_normal, float sigma_albedo, float* workspace, float* color3_out,
                   void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    const long long npx = (long long)W * H, n = npx * 3;
    const size_t plane = denoise_plane_floats(npx);
    float* c[2] = {workspace, workspace + plane};
    float* a3 = albedo ? workspace + 2 * plane : nullptr;
    float* n3 = normal ? workspace + 3 * plane : nullptr;
    hipLaunchKernelGGL(denoise_prepare_kernel, dim3(grid_1d(n)), dim3(256), 0, st, n, canva, albedo, normal, c[0], a3,
                       n3);
    float sig_c = sigma_color;
    for (int i = 0; i < iterations; ++i) {
        const int step = 1 << i;
        const float* cin = c[i & 1];
        float* cout = c[(i + 1) & 1];
        if (a3 && n3) launch_pass<true, true>(W, H, step, sig_c, sigma_normal, sigma_albedo, cin, a3, n3, cout, st);
        else if (a3) launch_pass<true, false>(W, H, step, sig_c, sigma_normal, sigma_albedo, cin, a3, n3, cout, st);
        else if (n3) launch_pass<false, true>(W, H, step, sig_c, sigma_normal, sigma_albedo, cin, a3, n3, cout, st);
        else launch_pass<false, false>(W, H, step, sig_c, sigma_normal, sigma_albedo, cin, a3, n3, cout, st);
        sig_c = sig_c * 0.5f;           // sigma_color * 2^-(i+1), exact
    }
    hipLaunchKernelGGL(denoise_finish_kernel, dim3(grid_1d(n)), dim3(256), 0, st, n, c[iterations & 1], canva,
                       color3_out);
    return (int)hipGetLastError();
}

}  // namespace rt
