// rt_queue_list.hip — render_kernel_ql: the task-queue kernel (rt_queue.h
// render_kernel_q) over a compacted list of pixels (rt_accumulate_list_async
// with rt_set_accumulate_queue on), and its launcher.
//
// A band [e0, e1) of a list launch holds n = min(*count, e1) - e0 entries and
// n * P tasks, chunk-major (the tapered short slices come last): task t is
// slice t / n of entry e0 + t % n, and its partial goes to index
// (t / n) * stride + t % n of the band's partials -- the layout
// combine_list_kernel (rt_adaptive.hip) reads, which runs behind this kernel
// unchanged.  The count is a device word that the host never reads, so n, n * P
// and the division magic floor((2^32 - 1) / n) come from a one-wave prologue
// kernel, which also zeroes the task counter; the render kernel reads the three
// words through the scalar unit where a batch of tasks is decoded.  With n = 0
// every lane finds "past the last task" on its first grab and the grid drains.
//
// The round loop is render_kernel_q's, restated here: sharing one body between
// the two kernels (a function template over the decoder) changed the register
// allocation of render_kernel_q's instantiations, and their machine code is
// pinned (tools/isa_same.py; rt_vdenoise.hip's px kernels are the precedent).
// QPath, QVariant and every step's helpers are rt_queue.h's own; only the
// kernel function is a second text.  It leaves out render_kernel_q's build-time
// diagnostics (RT_PHASE_CLOCK, RT_DIAG_*).  A translation unit
// of its own: the kernels of rt_kernels.hip and rt_adaptive.hip keep theirs.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

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
#include "rt_queue.h"
#include "rt_queue_launch.h"

namespace rt {

// The kernel's second by-value argument, behind KParams in the kernarg segment,
// through an address the compiler cannot see through (rt_vec.h kp_here).
typedef const __attribute__((address_space(4))) ListArgs* ListArgsK;
__device__ __forceinline__ ListArgsK la_here()
{
    static_assert(sizeof(KParams) % alignof(ListArgs) == 0, "ListArgs follows KParams without padding");
    const __attribute__((address_space(4))) char* p =
        (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(KParams);
    asm volatile("" : "+s"(p));
    return (ListArgsK)p;
}

// The band's task words: written by the prologue before this kernel starts and
// by nothing afterwards, so they are read as constants (scalar loads).
enum : int { LT_TASKS = 0, LT_ENTRIES = 1, LT_MAGIC = 2 };
static_assert(LT_MAGIC + 1 == kListTaskWords, "the prologue's words");

// One wave; its first lane writes.  n <= band and band * chunks < 2^31 (plan_list).
__global__ __launch_bounds__(64) void list_tasks_kernel(const ListArgs la, unsigned chunks, unsigned* __restrict__ ctr)
{
    if (threadIdx.x != 0) return;
    const unsigned end = min(*la.count, la.e1);
    const unsigned n = end > la.e0 ? end - la.e0 : 0u;
    unsigned* w = ctr + kListTaskOffset;
    ctr[0] = 0u;
    w[LT_TASKS] = n * chunks;
    w[LT_ENTRIES] = n;
    w[LT_MAGIC] = n ? 0xffffffffu / n : 0u;
}

// decode_task (rt_queue.h) for the tasks of a list band: e[0] the partial index
// (~0: past the last task), e[1] the listed pixel (~0: an index at or beyond
// W * H, a task without work, as in list_body), e[2] its row, e[3], e[4] the
// slice's first and end sample.  The lanes of a wave decode consecutive tasks,
// so list[] is read in one coalesced load unless the batch crosses a slice.
__device__ __forceinline__ void decode_list_task(KParamsK K, unsigned t, uint32_t e[kTaskWords])
{
    const ListArgsK A = la_here();
    const __attribute__((address_space(4))) unsigned* w =
        (const __attribute__((address_space(4))) unsigned*)(K->task_ctr + kListTaskOffset);
    // (every word is assigned once, by selects: an entry filled behind early
    // returns kept a dead 20-byte stack object, and with it a scratch
    // allocation, in the sphere-only instantiations)
    const bool task = t < w[LT_TASKS];
    unsigned r;
    const unsigned q = udiv_q(t, w[LT_ENTRIES], w[LT_MAGIC], r);
    const unsigned chunk = task ? q : 0u;
    unsigned pixel = 0xffffffffu;                        // never a pixel: W * H <= 2^32 - 1 (validate_params)
    if (task) pixel = A->list[A->e0 + r];
    const bool work = pixel < (unsigned)K->W * (unsigned)K->H;
    unsigned xr;
    const unsigned row = udiv_q(pixel, (unsigned)K->W, K->qm_w, xr);
    e[0] = task ? chunk * A->stride + r : 0xffffffffu;
    e[1] = work ? pixel : 0xffffffffu;
    e[2] = work ? row : 0xffffffffu;
    e[3] = (uint32_t)chunk_start(K->S, K->chunks, K->chunk_taper, K->chunk_den, K->qm_chunks, chunk);
    e[4] = (uint32_t)chunk_start(K->S, K->chunks, K->chunk_taper, K->chunk_den, K->qm_chunks, chunk + 1u);
}

// render_kernel_q (rt_queue.h; the steps' comments are there) with step 3's
// tasks decoded by decode_list_task.  kp.partial is the band's partials.
template <bool SKY, int AOM, int QB, bool OPQ = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(QVariant<SKY, AOM, QB, OPQ>::WAVES)))
void render_kernel_ql(const KParams kp, const ListArgs la)
{
    using V = QVariant<SKY, AOM, QB, OPQ>;
    constexpr bool PD = V::PD, TTAB = V::TTAB;
    constexpr int NTOP = V::NTOP, HN = V::HN;
    __shared__ double acc_lds[(ACC_SLOTS + 3 * V::IR) * 256];
    __shared__ uint32_t rng_lds[4 * 256];
    double* acc = acc_lds + threadIdx.x;
    uint32_t* rng = rng_lds + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned qb = 0, qe = 0;         // the wave's batch of tasks [qb, qe) (wave-uniform)
    QPath<V> L;
    L.init(acc);
    uint32_t kw2 = 0, kw3 = 0;       // (PD) the kept words of the sample's current block
    // (PD) the head of the task's Philox blocks, made from the listed pixel when the lane takes the task
    __shared__ uint32_t head_lds[PD ? 3 * 256 : 1];
    uint32_t* head = head_lds + (PD ? threadIdx.x : 0);
    int x = 0, g = 0, s1 = 0;
    int node = 0, sp = 0, win_orig = 0;      // BVH walk in flight (state SM_TRAV)
    unsigned pixel = 0, qidx = 0;    // the lane's task: its pixel and its partial index (decode_list_task e[1], e[0])
    bool owns = false;               // the lane's LDS sums belong to that task
    __shared__ uint32_t ttab_lds[TTAB ? 4 * kTaskWords * 64 : 1];
    Stream st;                       // draw stream of the sample in flight (next31 for refraction / AO)
    st.start(0u, 0u, kp.key0, kp.key1, rng);
    if (NTOP > 0) {                          // the tree's top nodes into LDS, once per block
        float4* dst = (float4*)bvh_top_q<NTOP>();
        const float4* src = (const float4*)kp.bvh;
        const int n = min(NTOP, kp.bvh_nodes) * (int)(sizeof(BvhNode4) / sizeof(float4));
        for (int i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
        __syncthreads();
    }
    // render_kernel_q's per-lane trace (kp.trace; a list launch passes none).  Kept
    // with the kernel: without these counters the sphere-only instantiations came
    // out with a 20-byte private segment that no instruction touches, and so with
    // a scratch allocation per launch (make resource-usage).
    const long long t_start = kp.trace ? wall_clock64() : 0;
    unsigned rounds = 0, ntasks = 0;
    while (true) {
        ++rounds;
        // ---- 1. closest hit for every lane with a ray ----------------------
        if constexpr (V::BVH) {
            if (L.state == SM_CAST) {
                Cnt cnt;
                L.win = cast_spheres<V::CAST>(kp, L.o, L.cast_dir(), L.best, cnt);
                L.kind = L.win >= 0 ? HIT_SPHERE : HIT_NONE;
                win_orig = 0;
                node = 0;
                sp = 0;
                L.state = SM_TRAV;
            }
            if (__ballot(L.state == SM_TRAV) != 0ull) {
#if RT_WALK_PRIO
                __builtin_amdgcn_s_setprio(RT_WALK_PRIO);
#endif
                const V3 dd = L.cast_dir();
                const Ray32 r32 = ray32<V::FAR>(kp, L.o, dd);
                const auto stk = bvh_stack_for_q<QB, OPQ>();
                const BvhNode4* top = NTOP > 0 ? bvh_top_q<NTOP>() : nullptr;
#pragma unroll 1
                for (int j = 0; j < V::JMAX; ++j) {
                    if (L.state == SM_TRAV) {
                        Cnt cnt;
                        if (!bvh_step<false, false, NTOP, HN>(kp, L.o, dd, r32, stk, node, sp, L.best, L.kind, L.win,
                                                           win_orig, cnt, top))
                            L.state = SM_RESOLVE;
                    }
                    const unsigned long long wm = __ballot(L.state == SM_TRAV);
                    if (wm == 0ull || (j + 1 >= V::JMIN && __popcll(wm) < RT_QW_LANES)) break;
                }
#if RT_WALK_PRIO
                __builtin_amdgcn_s_setprio(0);
#endif
            }
        } else if (V::NT && L.state == SM_CAST) {          // sphere-only scenes: no triangle scan
            Cnt cnt;
            L.win = cast_spheres<V::CAST>(kp, L.o, L.cast_dir(), L.best, cnt);
            L.kind = L.win >= 0 ? HIT_SPHERE : HIT_NONE;
            L.state = SM_RESOLVE;
        } else if (L.state == SM_CAST) {
            Cnt cnt;
            L.kind = closest_hit<V::CAST>(kp, L.o, L.cast_dir(), L.best, L.win, cnt);
            L.state = SM_RESOLVE;
        }
        // ---- 2. the hit, up to the next direction --------------------------
        int role = ROLE_NONE;
        QHit H;
        if (PD) {
            // (rt_queue.h: the four values defined here without an instruction)
            asm volatile("" : "=v"(H.hn.x), "=v"(H.hn.y), "=v"(H.hn.z), "=v"(H.rs));
        } else {
            H.hn = v3(0, 0, 0);
            H.rs = 0.0;
        }
        H.refr = H.hole = false;
        if (L.state == SM_RESOLVE) role = L.resolve_hit(kp, acc, H, st.n);
        // ---- 3. lanes whose task is done take the next one -----------------
        const bool need = L.state == SM_CAM && L.s >= s1;
        const unsigned long long nm = __ballot(need);
        if (nm) {                    // wave-uniform: tasks for the lanes that need one
            const KParamsK K = kp_here();
            const unsigned nn = (unsigned)__popcll(nm), avail = qe - qb;
            const unsigned rank = (unsigned)__popcll(nm & ((1ull << lane) - 1ull));
            const bool old = rank < avail;
            uint32_t* tw = ttab_lds + (threadIdx.x >> 6) * (kTaskWords * 64);
            unsigned t = qb + rank;
            uint32_t e[kTaskWords];
            if (TTAB && need && old) {
                const unsigned slot = (qb - (qe - kQueueBatch)) + rank;
#pragma unroll
                for (int j = 0; j < kTaskWords; ++j) e[j] = tw[j * 64 + slot];
            }
            if (avail < nn) {            // a new batch (nn <= 64)
                unsigned nb = 0;
                if (lane == __ffsll((long long)nm) - 1) nb = atomicAdd(K->task_ctr, (unsigned)kQueueBatch);
                nb = __shfl(nb, __ffsll((long long)nm) - 1, 64);
                if constexpr (TTAB) {
                    uint32_t d[kTaskWords];
                    decode_list_task(K, nb + (unsigned)lane, d);
#pragma unroll
                    for (int j = 0; j < kTaskWords; ++j) tw[j * 64 + lane] = d[j];
                    if (need && !old) {
#pragma unroll
                        for (int j = 0; j < kTaskWords; ++j) e[j] = tw[j * 64 + (rank - avail)];
                    }
                } else if (!old) {
                    t = nb + (rank - avail);
                }
                qb = nb + (nn - avail);
                qe = nb + kQueueBatch;
            } else {
                qb += nn;
            }
            if (need) {
                if constexpr (!TTAB) decode_list_task(K, t, e);
                ++ntasks;
                if (owns) {              // task done: its sums to the band's partials
                    double* q = K->partial + (size_t)qidx * 9;
#pragma unroll
                    for (int j = 0; j < 9; ++j) q[j] = acc[j * 256];
                    owns = false;
                }
                if (e[0] == 0xffffffffu) {
                    L.state = SM_DONE;
                } else if (e[1] != 0xffffffffu) {  // else not a pixel: the lane takes its next task next round
                    qidx = e[0];
                    if constexpr (PD) {
                        const PhiloxHead h = philox_head(e[1], K->key0);
                        head[0] = h.c1;
                        head[256] = h.hi;
                        head[512] = h.lo;
                    } else {
                        pixel = e[1];
                    }
                    g = (int)e[2];
                    x = (int)(e[1] - e[2] * (unsigned)K->W);
                    L.s = (int)e[3];
                    s1 = (int)e[4];
#pragma unroll
                    for (int j = 0; j < 9; ++j) acc[j * 256] = 0.0;
                    owns = true;
                }
            }
        }
        if (__ballot(L.state != SM_DONE) == 0ull) break;     // every lane of the wave is done
        // tracer with nbRebondMax <= 0 returns (0, 0, 0) albedo/normal/colour
        if (kp.B <= 0 && L.state == SM_CAM && L.s < s1) {
            acc_add(acc, ACC_ALB, v3(0, 0, 0));
            acc_add(acc, ACC_NRM, v3(0, 0, 0));
            acc_add(acc, ACC_RAD, v3(0, 0, 0));
            ++L.s;
            continue;
        }
        if (L.state == SM_CAM && L.s < s1) role = ROLE_CAMERA;
        // ---- 4. next ray: bounce direction or camera ray (shared work) ----
        if (role != ROLE_NONE) {
            const bool cam = role == ROLE_CAMERA;
            const bool aor = AOM == AO_ON && role == ROLE_AO, pbr = AOM == AO_ON && role == ROLE_PBOUNCE;
            const uint32_t nd = cam ? 0u : st.n;
            const uint32_t sa = nd & 3u, sb = (nd + 1u) & 3u;
            uint32_t wa = 0, wb = 0;
            Philox blk{0, 0, 0, 0};
            Philox pblk;                 // (PD) its block: read by camera lanes alone, which make it
            if constexpr (PD) {
                if (cam || (L.i & 1) == 0) {
                    const uint32_t bi = cam ? 0u : 1u + ((uint32_t)L.i >> 1);
                    const PhiloxHead h{head[0], head[256], head[512]};
                    pblk = philox4x32_10(bi, h, (uint32_t)(kp.s_base + L.s), kp.key0, kp.key1);
                    wa = pblk.w0;
                    wb = pblk.w1;
                    kw2 = pblk.w2;
                    kw3 = pblk.w3;
                } else {
                    wa = kw2;
                    wb = kw3;
                }
            } else if (pbr) {
                wa = rng[0];
                wb = rng[256];
            } else {
                if (!cam && !aor && sa != 0u) wa = rng[sa * 256];          // cached word of the current block
                if (!cam && !aor && sb != 0u && sa != 0u) wb = rng[sb * 256];
                const bool rpre = !cam && !aor && !pbr && H.refr && sa == 2u;
                if (cam || aor || sa == 0u || sb == 0u || rpre) {         // a new block: one Philox for every role
                    const uint32_t bi = cam ? 0u : ((nd + (sa == 0u ? 0u : rpre ? 2u : 1u)) >> 2);
                    blk = philox4x32_10(bi, 0u, pixel, (uint32_t)(kp.s_base + L.s), kp.key0, kp.key1);
                    if (aor) {                                      // the bounce's draws, for ROLE_PBOUNCE
                        rng[0] = blk.w0;
                        rng[256] = blk.w1;
                    } else if (!cam) {                              // keep the rest of the block
                        if (rpre) rng[0] = blk.w0;
                        rng[256] = blk.w1;
                        rng[512] = blk.w2;
                        rng[768] = blk.w3;
                    }
                }
                if (aor) {
                    wa = blk.w2;
                    wb = blk.w3;
                } else if (!cam) {
                    if (sa == 0u) wa = blk.w0;
                    if (sb == 0u) wb = blk.w0;
                    else if (sa == 0u) wb = blk.w1;
                }
            }
            V3 X;
            V3 no = v3(0, 0, 0);
            if (cam) {
                CamDraws w{PD ? pblk : blk, 0};
                X = camera_ray_raw<false>(kp, x, g, w, kp.cam_pin != 0, PD ? L.o : no);
            } else {
                X = H.hn + normalize_unit(sampler_vec(wa >> 1, wb >> 1));
                if (!PD) st.n += aor ? 0u : pbr ? 4u : 2u;
            }
            const V3 dn = normalize(X);
            if (cam) {                                         // the new sample's primary ray
                if (!PD) L.o = no;
                L.d = dn;
                if (AOM == AO_ON) L.cd = dn;
                L.inc_set(v3(0, 0, 0));
                L.rc_set(v3(1, 1, 1));
                L.top_n2 = 1.0;
                L.i = 0;
                L.chain = true;
                L.ao_cast = false;
                L.state = SM_CAST;
                if (!PD) {
                    st.start(pixel, (uint32_t)(kp.s_base + L.s), kp.key0, kp.key1, rng);
                    st.n = 4;                                  // draws 0-3 were the camera's
                }
            } else if (aor) {                                  // ambient_occlusion's cast
                L.cd = dn;
                L.ao_cast = true;
                L.state = SM_CAST;
            } else if (pbr) {                                  // the bounce after the AO cast
                const V3 reflected_dir = L.d - muls(H.hn, 2 * dot(L.d, H.hn));
                L.d = dn + muls(reflected_dir - dn, H.rs);
                L.cd = L.d;
                L.state = SM_CAST;
            } else {
                L.finish_bounce(kp, dn, st, acc, H);
            }
        }
    }
    if (kp.trace) {                  // per lane start, end, rounds, tasks
        unsigned long long* q = kp.trace + ((size_t)blockIdx.x * 256 + threadIdx.x) * RT_TRACE_WORDS;
        q[0] = (unsigned long long)t_start;
        q[1] = (unsigned long long)wall_clock64();
        q[2] = rounds;
        q[3] = ntasks;
    }
}

using ListQueueKernel = void (*)(const KParams, const ListArgs);
template <class V>
constexpr ListQueueKernel list_queue_kernel(V) { return render_kernel_ql<V::SKY, V::AOM, V::QB, V::OPQ>; }

// One entry band [la.e0, la.e1) on the queue kernel of the plan's variant: the
// prologue, the resident grid, the combine.
int launch_render_list_queue(const KParams& kp, const RenderPlan& pl, const ListArgs& la, void* stream)
{
    const hipStream_t st = (hipStream_t)stream;
    ListQueueKernel kernel = nullptr;
    unsigned nb = 0;
    const bool listed = pl.queue && with_queue_variant(pl, [&](auto v) {
        kernel = list_queue_kernel(v);
        nb = queue_grid(v, kernel, "render_kernel_ql");
    });
    if (!listed || !kp.task_ctr || kp.chunks <= 1 || !la.partial) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(list_tasks_kernel, dim3(1), dim3(64), 0, st, la, (unsigned)kp.chunks, kp.task_ctr);
    KParams k2 = kp;
    k2.partial = la.partial;
    k2.trace = nullptr;
    set_queue_magics(k2);
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, st, k2, la);
    return launch_combine_list(kp, la, stream);
}

}  // namespace rt
