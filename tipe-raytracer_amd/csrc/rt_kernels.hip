// rt_kernels.hip — the per-pixel path-tracing kernel for gfx950 (CDNA4).
//
// One thread renders one pixel (or one chunk of its samples): the sample
// loop, the nbRebondMax bounce loop, closest-hit scans, shading and AO all
// run in registers; HBM traffic is the final colors per pixel (plus, with
// sample chunking, one 72-byte partial sum per pixel and chunk).
//
// Semantics follow main.c (the authoritative CPU path), not main_cuda.cu
// (reference lines -> function, file; this file includes the headers in
// definition order and keeps the small kernels and the launchers, which execute
// the host's plan, rt_launch_plan.cpp plan_render; the queue kernel's (QB, OPQ)
// instantiations are rt_queue_variants.h's table, shared with that plan, and
// rt_queue.h QVariant holds what the device derives from a row):
//   fill_canva        main.c:245-284      -> render_kernel_q (task queue; decode_task is its one
//                                            task decoder), rt_queue.h / render_kernel (fixed
//                                            grid; tile_row: local tile row -> frame row),
//                                            rt_fixed_grid.h; combine_kernel, here
//   tracer            main.c:118-242      -> QPath (queue kernel), rt_queue.h; LanePath
//                                            (fixed grid), rt_fixed_grid.h
//   closest_hit       main.c:52-92        -> closest_hit(), rt_triangles.h
//   ambient_occlusion main.c:94-116       -> ao_factor() / ao_tail(), rt_shading.h
//   hit_sphere        sphere.h:13-47      -> sphere_exact() (+ candidate pass), rt_spheres.h
//   hit_triangle      mesh.h:70-94        -> tri_test(), rt_triangles.h; the BVH node visit
//                                            bvh_visit() (bvh_step: a lane's own walk;
//                                            samples_coop, rt_fixed_grid.h: the wave's)
//   tri_uvmapping     texture.h:44-90     -> tri_texel(), rt_shading.h
//   get_ray           camera.h:42-55      -> camera_ray_raw(), rt_fixed_grid.h (camera_ray: its
//                                            normalize; render_kernel_q's next-ray step shares
//                                            the bounce lanes' normalize)
//   shading           main.c:208-234      -> LanePath::resolve, rt_fixed_grid.h;
//                                            QPath::shade_with, rt_queue.h
//   random_dir_no_norm / refracted_vec / hsl   rtutility.h:81-231 -> rt_shading.h
//   write_color_canva rtutility.h:56-71   -> resolve() / write_pixel(), rt_fixed_grid.h
//   vec3.h                                -> V3, normalize(), rt_vec.h
// (rt_verify.h: the rt_verify_* kernels that check device fast paths.)
// Every floating-point value that reaches an output is produced by the
// reference's IEEE operations in its association order, one rounding each
// (-ffp-contract=off): results are bit-identical to the CPU restatement in
// RT_RNG_PHILOX mode.
//
// MI355X mapping (DESIGN.md "Kernel"):
//  * geometry is scanned in the same order by every lane of a wave: sphere
//    records come through the scalar unit (SMEM -> SGPRs, broadcast to the
//    64 lanes for free), two per s_load_dwordx16;
//  * closest hit = a cheap candidate pass (hardware rsq + one Newton step,
//    reciprocal multiply, rigorous error intervals) followed by the exact
//    reference arithmetic for the single winner; any interval overlap or
//    threshold ambiguity falls back to the exact scan for that ray, so the
//    result never depends on the approximation;
//  * per-lane divergent data (the winner's material, texels) is fetched once
//    per bounce from L1/L2;
//  * the IOR stack of pile.h reduces to one register (top n2), see QPath::finish_bounce;
//  * albedo/normal are final once the primary chain (camera ray through
//    alpha holes) ends, so they are added to the accumulators there instead
//    of being carried through the bounce loop;
//  * 256-thread blocks = four 8x8-pixel waves (ray coherence); grid.z splits
//    each pixel's samples into `chunks` fixed slices for load balance, summed
//    in chunk order by combine_kernel (a deterministic, GPU-count-independent
//    grouping that the oracle reproduces).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt/rt.h"
#include "rt_internal.h"
#include "rt_bvh.h"
#include "rt_launch_plan.h"
#include "rt_device_math.h"

// Build-time tunables and diagnostic switches (shared with rt_adaptive.hip).
#include "rt_tunables.h"

// The device code by concern, in definition order (one translation unit).
#include "rt_vec.h"
#include "rt_spheres.h"
#include "rt_triangles.h"
#include "rt_shading.h"
#include "rt_fixed_grid.h"
#include "rt_queue.h"
#include "rt_queue_launch.h"

namespace rt {

// Sum the chunk partials of each pixel in chunk order, then resolve.
__global__ __launch_bounds__(256) void combine_kernel(const KParams kp)
{
    const int rows = min(kp.band_rows, kp.local_rows - kp.band_y0);
    const long long npx = (long long)kp.band_rows * kp.W;      // partial plane stride
    const long long nb = (long long)rows * kp.W;
    for (long long bi = (long long)blockIdx.x * blockDim.x + threadIdx.x; bi < nb;
         bi += (long long)gridDim.x * blockDim.x) {
        const int ly = kp.band_y0 + (int)(bi / kp.W);
        const long long li = (long long)kp.band_y0 * kp.W + bi;
        const int lt = ly / kp.tile_rows, yy = ly - lt * kp.tile_rows;
        const int g = tile_row(kp, lt, yy);
        if (g >= kp.row_end) continue;
        double a[9];
        int c0 = 0;
        if (kp.sums) {                                   // accumulate: running sums + slices in order
#pragma unroll
            for (int j = 0; j < 9; ++j) a[j] = kp.sums[li * 9 + j];
        } else {
            const double* p = kp.partial + bi * 9;
#pragma unroll
            for (int j = 0; j < 9; ++j) a[j] = p[j];
            c0 = 1;
        }
        for (int c = c0; c < kp.chunks; ++c) {
            const double* q = kp.partial + ((long long)c * npx + bi) * 9;
#pragma unroll
            for (int j = 0; j < 9; ++j) a[j] = a[j] + q[j];
        }
        if (kp.sums) {
#pragma unroll
            for (int j = 0; j < 9; ++j) kp.sums[li * 9 + j] = a[j];
        } else {
            write_pixel(kp, li, v3(a[0], a[1], a[2]), v3(a[3], a[4], a[5]), v3(a[6], a[7], a[8]));
        }
    }
}

// Un-permute a rank-major gather of cyclic row tiles into the full frame.
__global__ __launch_bounds__(256) void assemble_kernel(const double* __restrict__ gathered, long long rank_stride,
                                                       int world, int tile_rows, int rows_per_rank, int W, int H,
                                                       double* __restrict__ out)
{
    const long long n = (long long)W * H * 3;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n;
         e += (long long)gridDim.x * blockDim.x) {
        const long long px = e / 3;
        const int c = (int)(e - px * 3);
        const int g = (int)(px / W), i = (int)(px - (long long)g * W);
        const int t = g / tile_rows, y = g - t * tile_rows;
        const int r = t % world, lt = t / world;
        const long long src = (long long)r * rank_stride + ((long long)lt * tile_rows + y) * W + i;
        out[e] = gathered[src * 3 + c];
    }
}

// Per-launch uniform block: the values travel as this kernel's by-value
// argument (captured at enqueue), so the copy is stream-ordered without a
// pageable host staging buffer.
// The camera's (W-1) and (H-1) reciprocals are refined here on the device
// (rcp_refined is the device's own sequence) so camera_ray divides with
// div_core; 0 (W or H of 1, a zero divisor) selects the plain division.
__global__ void set_uniforms_kernel(const UniBlock u, double* __restrict__ dst)
{
    const int i = threadIdx.x;
    if (i < U_COUNT) {
        double v = u.v[i];
        if (i == U_RC_WM1 || i == U_RC_HM1) {
            const double d = u.v[i == U_RC_WM1 ? U_WM1 : U_HM1];
            v = (d >= 1.0 && d <= 0x1p400) ? rcp_refined(d) : 0.0;
        }
        dst[i] = v;
    }
}

int launch_set_uniforms(const UniBlock& u, double* d_uni, void* stream)
{
    hipLaunchKernelGGL(set_uniforms_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, u, d_uni);
    return (int)hipGetLastError();
}

// Device-math self test (rt_selftest_math).
__global__ void selftest_kernel(int op, const double* __restrict__ in, double* __restrict__ out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    switch (op) {
    case 0: out[i] = pm_acos(in[i]); break;
    case 1: {
        float s, c;
        pm_sincosf((float)in[i], s, c);
        out[i] = (double)s;
        break;
    }
    case 2: {
        float s, c;
        pm_sincosf((float)in[i], s, c);
        out[i] = (double)c;
        break;
    }
    case 3: out[i] = pm_pow(in[2 * i], in[2 * i + 1]); break;
    case 4: out[i] = sqrt(in[i]); break;
    case 5: out[i] = in[2 * i] / in[2 * i + 1]; break;
    case 6: out[i] = (double)sqrtf((float)in[i]); break;
    case 7: {
        const double* q = in + 6 * i;
        const Philox p = philox4x32_10<false>((uint32_t)q[0], (uint32_t)q[1], (uint32_t)q[2], (uint32_t)q[3],
                                       (uint32_t)q[4], (uint32_t)q[5]);
        out[4 * i + 0] = p.w0;
        out[4 * i + 1] = p.w1;
        out[4 * i + 2] = p.w2;
        out[4 * i + 3] = p.w3;
        break;
    }
    case 9: out[i] = pm_atan2(in[2 * i], in[2 * i + 1]); break;
    case 8: {                                   // normalize (fast lanes and generic lanes)
        const V3 v = normalize(v3(in[3 * i], in[3 * i + 1], in[3 * i + 2]));
        out[3 * i + 0] = v.x;
        out[3 * i + 1] = v.y;
        out[3 * i + 2] = v.z;
        break;
    }
    default: out[i] = 0.0;
    }
}

// OIDN input planes from a device frame, denoiser.h:44-60 (IEEE f32 ops).
__global__ __launch_bounds__(256) void denoise_pack_kernel(long long n, const double* __restrict__ canva,
                                                           const double* __restrict__ albedo,
                                                           const double* __restrict__ normal, float* __restrict__ c3,
                                                           float* __restrict__ a3, float* __restrict__ n3)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        c3[i] = (float)canva[i] / 255.0f;
        if (a3) a3[i] = (float)albedo[i];
        if (n3) n3[i] = (float)normal[i];
    }
}

// Blocks of 256 threads for n elements of a grid-stride kernel, at most cap.
static unsigned grid_1d(long long n, long long cap) { return (unsigned)std::min((n + 255) / 256, cap); }

int launch_denoise_pack(long long npx, const double* canva, const double* albedo, const double* normal, float* color3,
                        float* albedo3, float* normal3, void* stream)
{
    const long long n = npx * 3;
    hipLaunchKernelGGL(denoise_pack_kernel, dim3(grid_1d(n, 8192)), dim3(256), 0, (hipStream_t)stream, n, canva,
                       albedo ? albedo : nullptr, normal, color3, albedo ? albedo3 : nullptr,
                       normal ? normal3 : nullptr);
    return (int)hipGetLastError();
}

// rt_resolve_async: running sums -> frame planes for kp.S total samples
// (write_color_canva / divide_scalar, main.c:275-279).
__global__ __launch_bounds__(256) void resolve_kernel(const KParams kp)
{
    const long long npx = (long long)kp.local_rows * kp.W;
    for (long long li = (long long)blockIdx.x * blockDim.x + threadIdx.x; li < npx;
         li += (long long)gridDim.x * blockDim.x) {
        const int ly = (int)(li / kp.W);
        const int lt = ly / kp.tile_rows, yy = ly - lt * kp.tile_rows;
        const int g = tile_row(kp, lt, yy);
        if (g >= kp.row_end) continue;
        const double* a = kp.sums + li * 9;
        write_pixel(kp, li, v3(a[0], a[1], a[2]), v3(a[3], a[4], a[5]), v3(a[6], a[7], a[8]));
    }
}

int launch_resolve(const KParams& kp, void* stream)
{
    const long long npx = (long long)kp.local_rows * kp.W;
    hipLaunchKernelGGL(resolve_kernel, dim3(std::max(1u, grid_1d(npx, 8192))), dim3(256), 0, (hipStream_t)stream, kp);
    return (int)hipGetLastError();
}

static dim3 grid_for(const KParams& kp)
{
    return dim3((unsigned)((kp.W + 15) / 16), (unsigned)((kp.band_rows + 15) / 16), (unsigned)kp.chunks);
}

// Kernel instantiation per scene features: BVH traversal and the sky branch
// are compiled only into the variants that use them, so a sphere-only scene
// runs a kernel without their registers.  (A wide tree, rt_bvh.h: the
// instantiations with uint32 stack entries.)
template <bool COUNT>
static void launch_variant(const KParams& kp, const RenderPlan& pl, void* stream)
{
    using K = void (*)(const KParams);
    const K kernel =
        pl.wide   ? (pl.cuda ? K(render_kernel_cuda_w<COUNT>) : pl.sky ? K(render_kernel_w<COUNT, true>) : K(render_kernel_w<COUNT, false>))
        : pl.cuda ? (pl.bvh ? K(render_kernel_cuda<COUNT, true>) : K(render_kernel_cuda<COUNT, false>))
        : pl.bvh  ? (pl.sky ? K(render_kernel<COUNT, true, true>) : K(render_kernel<COUNT, true, false>))
                  : (pl.sky ? K(render_kernel<COUNT, false, true>) : K(render_kernel<COUNT, false, false>));
    hipLaunchKernelGGL(kernel, grid_for(kp), dim3(256), 0, (hipStream_t)stream, kp);
}

static thread_local const char* t_last_kernel = "none";
const char* last_render_kernel() { return t_last_kernel; }

// One band of a render, as plan_render (rt_launch_plan.cpp) decided it.
int launch_render(const KParams& kp, const RenderPlan& pl, void* stream)
{
    t_last_kernel = pl.name;
    if (pl.queue) {
        const hipStream_t st = (hipStream_t)stream;
        // the dense form of render_kernel_q, its instantiation picked by
        // rt_queue_launch.h's table walk (with_queue_variant hands over the plan's QVariant)
        QueueKernel<> kernel = nullptr;
        unsigned nb = 0;
        const bool listed = with_queue_variant(pl, [&](auto v) {
            kernel = queue_kernel<>(v);
            nb = queue_grid(v, kernel, "render_kernel_q");
        });
        if (!listed) return (int)hipErrorInvalidValue;       // a (qb, opq) that plan_render cannot give
        (void)hipMemsetAsync(kp.task_ctr, 0, sizeof(unsigned), st);
        unsigned long long* tr = nullptr;
        const char* tf = std::getenv("RT_QUEUE_TRACE");
        if (tf) (void)hipMalloc((void**)&tr, (size_t)nb * 256 * RT_TRACE_WORDS * sizeof(unsigned long long));
        KParams k2 = kp;
        k2.trace = tr;
        const int rows_here = std::max(0, std::min(kp.band_rows, kp.local_rows - kp.band_y0));
        k2.npx_here = (unsigned)rows_here * (unsigned)kp.W;
        k2.qm_npx = qdiv_magic(k2.npx_here);
        k2.qm_tile = qdiv_magic((unsigned)kp.tile_rows);
        set_queue_magics(k2);
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, st, k2);
        if (tr) {
            std::vector<unsigned long long> h((size_t)nb * 256 * RT_TRACE_WORDS);
            (void)hipStreamSynchronize(st);
            (void)hipMemcpy(h.data(), tr, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
            (void)hipFree(tr);
            if (FILE* f = std::fopen(tf, "ab")) {
                std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
                std::fclose(f);
            }
        }
    } else {
        launch_variant<false>(kp, pl, stream);
    }
    if (kp.chunks > 1) {
        const long long npx = (long long)kp.band_rows * kp.W;
        hipLaunchKernelGGL(combine_kernel, dim3(grid_1d(npx, 8192)), dim3(256), 0, (hipStream_t)stream, kp);
    }
    return (int)hipGetLastError();
}

int launch_count(const KParams& kp, const RenderPlan& pl, void* stream)
{
    launch_variant<true>(kp, pl, stream);
    return (int)hipGetLastError();
}

int launch_assemble(const double* gathered, long long rank_stride, int world, int tile_rows, int rows_per_rank, int W,
                    int H, double* out, void* stream)
{
    const long long n = (long long)W * H * 3;
    hipLaunchKernelGGL(assemble_kernel, dim3(grid_1d(n, 4096)), dim3(256), 0, (hipStream_t)stream, gathered,
                       rank_stride, world, tile_rows, rows_per_rank, W, H, out);
    return (int)hipGetLastError();
}

}  // namespace rt

#include "rt_verify.h"
