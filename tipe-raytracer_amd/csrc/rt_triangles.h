// rt_triangles.h -- hit_triangle (mesh.h:70-94), the triangle BVH walk, and closest_hit (main.c:52-92).
// Part of the single translation unit rt_kernels.hip (included there, in this order).
#pragma once

namespace rt {

// hit_triangle, mesh.h:70-94, exact reference arithmetic, folded into the
// running closest hit.  Acceptance is the reference's `dst >= 1e-7 && dst <
// best` plus its in-order tie-break: when the triangles are not scanned in
// the caller's order (BVH leaf order), an equal dst replaces a triangle
// winner with a larger caller index (orig).  det >= 1e-6 >= 2^-400 puts
// 1/det on the exact fast division (div_core).
// O32 (BVH leaves: a tree holds at most 2^24 triangles, so k * sizeof(TriGeo) < 2^32):
// the records are read at 32-bit byte offsets from the array's scalar base.
// UNI (the brute-force scan, k wave-uniform): the record through the scalar
// unit (s_load into SGPRs, read by the VALU as scalar operands), no vector
// memory instructions per triangle.
template <bool COUNT, bool CU = false, bool O32 = false, bool UNI = false>
__device__ __forceinline__ void tri_test(const KParams& kp, int k, const V3 o, const V3 d, double& best, int& kind,
                                         int& win, int& win_orig)
{
    const double eps = CU ? 0.00001 : 0.0000001;     // triangle.hu:262 / mesh.h:88
    TriGeo g;
    if (UNI) {
        const cdptr t = (cdptr)kp.tri + 12 * k;
        g.ax = t[0]; g.ay = t[1]; g.az = t[2];
        g.abx = t[3]; g.aby = t[4]; g.abz = t[5];
        g.acx = t[6]; g.acy = t[7]; g.acz = t[8];
        g.nx = t[9]; g.ny = t[10]; g.nz = t[11];
    } else if (O32) {
        // the whole record in six 16-byte loads and ONE wait: left to itself
        // the compiler sinks the A/AB/AC loads below the det test, a second
        // dependent round trip per leaf test
        g = *(const TriGeo*)((const char*)kp.tri + (uint32_t)k * (uint32_t)sizeof(TriGeo));
        asm volatile("" : "+v"(g.ax), "+v"(g.ay), "+v"(g.az), "+v"(g.abx), "+v"(g.aby), "+v"(g.abz), "+v"(g.acx),
                     "+v"(g.acy), "+v"(g.acz), "+v"(g.nx), "+v"(g.ny), "+v"(g.nz));
    } else {
        g = kp.tri[k];
    }
    const double det = -(d.x * g.nx + d.y * g.ny + d.z * g.nz);
    if (det >= 1E-6) {
        const V3 ao = v3(o.x - g.ax, o.y - g.ay, o.z - g.az);
        const V3 dao = cross(ao, d);
        double invDet;
        if (det <= 0x1p400) invDet = div_core(1.0, det, rcp_refined(det));
        else invDet = 1 / det;
        const double dst = (ao.x * g.nx + ao.y * g.ny + ao.z * g.nz) * invDet;
        if (dst >= eps && dst <= best) {
            const int orig = !kp.tri_orig ? k
                             : O32 ? *(const int*)((const char*)kp.tri_orig + (uint32_t)k * 4u) : kp.tri_orig[k];
            if (dst < best || (kind == HIT_TRI && orig < win_orig)) {
                const double u = (g.acx * dao.x + g.acy * dao.y + g.acz * dao.z) * invDet;
                const double v = -(g.abx * dao.x + g.aby * dao.y + g.abz * dao.z) * invDet;
                const double w = 1 - u - v;
                if (u >= eps && v >= eps && w >= eps) {
                    best = dst;
                    kind = HIT_TRI;
                    win = k;
                    win_orig = orig;
                }
            }
        }
    }
}

// tri_test for the brute-force scan in the caller's order (kp.tri_orig null:
// no tie rule, `dst < best` is mesh.h's and main.c:82's strict test), with
// no branches: every lane evaluates det, dst and the barycentrics with the
// reference operations and one combined condition picks the hit.  The
// branchy form ran these in nested divergent regions whose exec-mask
// bookkeeping cost more than the work they skipped: in a wave of
// incoherent rays some lane almost always passes the culling tests.  Lanes
// with det < 1e-6 compute a garbage 1/det (the fast reciprocal of a small,
// zero or negative value) that no condition lets through.
template <bool CU>
__device__ __forceinline__ void tri_test_bf(const KParams& kp, int k, const V3 o, const V3 d, double& best, int& kind,
                                            int& win)
{
    const double eps = CU ? 0.00001 : 0.0000001;     // triangle.hu:262 / mesh.h:88
    const cdptr t = (cdptr)kp.tri + 12 * k;
    const double ax = t[0], ay = t[1], az = t[2], abx = t[3], aby = t[4], abz = t[5];
    const double acx = t[6], acy = t[7], acz = t[8], nx = t[9], ny = t[10], nz = t[11];
    const double det = -(d.x * nx + d.y * ny + d.z * nz);
    const V3 ao = v3(o.x - ax, o.y - ay, o.z - az);
    const V3 dao = cross(ao, d);
    double invDet;
    if (det <= 0x1p400) invDet = div_core(1.0, det, rcp_refined(det));
    else invDet = 1 / det;
    const double dst = (ao.x * nx + ao.y * ny + ao.z * nz) * invDet;
    const double u = (acx * dao.x + acy * dao.y + acz * dao.z) * invDet;
    const double v = -(abx * dao.x + aby * dao.y + abz * dao.z) * invDet;
    const double w = 1 - u - v;
    // every lane evaluates the whole test: the empty asm keeps the compiler
    // from sinking the barycentrics under a branch on det and dst
    double uu = u, vv = v;
    asm volatile("" : "+v"(uu), "+v"(vv));
    const bool hit = (det >= 1E-6) & (dst >= eps) & (dst < best) & (uu >= eps) & (vv >= eps) & (w >= eps);
    if (hit) {
        best = dst;
        kind = HIT_TRI;
        win = k;
    }
}

// Triangle BVH traversal (rt_bvh.h: 4-wide nodes collapsed from the binary
// SAH tree, host build rt_bvh.cpp).  One 128-byte node holds four child
// boxes (float storage rounded outward; the slab math runs in double); leaf
// children are tested on the spot, the nearest hit internal child is entered
// next and the others are pushed on a per-lane LDS stack (uint16
// [kStack4][256], conflict-free; uint32 for a wide tree, rt_bvh.h).  A box is skipped only when no triangle in
// it can win or tie (rt_bvh.cpp): the ray misses the padded box, leaves it
// behind the origin (tmax < -sabs), or enters it beyond best*(1+srel)+sabs.
// Slab reciprocals use |d_i| >= 2^-200, which keeps the products finite
// without changing any decision for unit-length directions.
// The per-lane stack: one LDS allocation per kernel ([kStack4][256]).
__device__ __forceinline__ unsigned short* bvh_stack()
{
    __shared__ unsigned short stk_lds[kStack4 * 256];
    return stk_lds + threadIdx.x;
}
// The queue kernel's per-lane stack (BVH scenes): uint16 [entries][256], entries
// from the pair's row of rt_queue_variants.h -- the number plan_render gives the
// host as stack_cap.  Why these capacities (rt_bvh.h): QB_DEEP gets kStackQ = 24
// entries (12 KiB) when every material is opaque (OPQ: incomingLight also lives
// in LDS) and kStackQN = 32 (16 KiB) otherwise, which keeps both at <= 40 KiB,
// i.e. 4 blocks (16 waves) per CU.  QB_TOP has kStackQ4 = 14 entries, so its
// top-node cache and the task table fit the same 40 KiB.
template <int QB, bool OPQ>
__device__ __forceinline__ unsigned short* bvh_stack_q()
{
    constexpr int entries = queue_variant(QB, OPQ).stack;
    static_assert(entries > 0 && !queue_variant(QB, OPQ).stack24, "a BVH kernel with uint16 stack entries");
    __shared__ unsigned short stkq_lds[entries * 256];
    return stkq_lds + threadIdx.x;
}
// Stack access by element type: a column of uint16 (narrow trees) or uint32
// (wide trees on the fixed grid) entries, 256 lanes apart.
template <class T>
__device__ __forceinline__ void stk_put(T* stk, int sp, int v) { stk[sp * 256] = (T)v; }
template <class T>
__device__ __forceinline__ int stk_get(const T* stk, int sp) { return (int)stk[sp * 256]; }
// Wide trees (rt_bvh.h BvhBuild::wide; node indices < 2^24) on the fixed grid:
// uint32 [kStack4][256], 48 KiB with the 22 KiB of sums and draws, two blocks per CU.
__device__ __forceinline__ uint32_t* bvh_stack32()
{
    __shared__ uint32_t stk32_lds[kStack4 * 256];
    return stk32_lds + threadIdx.x;
}
template <class SE>
__device__ __forceinline__ SE* bvh_stack_of()
{
    if constexpr (sizeof(SE) == 4) return bvh_stack32();
    else return bvh_stack();
}
// ... in the queue kernel (QB_WIDE, the one stack24 row of rt_queue_variants.h):
// kStackQW = 32 entries of 24 bits, split into a
// uint16 column and a uint8 column, 24 KiB: with the 22 KiB of sums and draws
// 46 KiB per block, three blocks (12 waves) per CU.  (32 uint32 entries would
// make it 54 KiB: two blocks.)
struct Stack24 {
    unsigned short* lo;
    unsigned char* hi;
};
__device__ __forceinline__ Stack24 bvh_stack_qw()
{
    constexpr int entries = queue_variant(QB_WIDE, false).stack;
    __shared__ unsigned short stkw_lo_lds[entries * 256];
    __shared__ unsigned char stkw_hi_lds[entries * 256];
    return Stack24{stkw_lo_lds + threadIdx.x, stkw_hi_lds + threadIdx.x};
}
__device__ __forceinline__ void stk_put(Stack24 stk, int sp, int v)
{
    stk.lo[sp * 256] = (unsigned short)((unsigned)v & 0xffffu);
    stk.hi[sp * 256] = (unsigned char)((unsigned)v >> 16);
}
__device__ __forceinline__ int stk_get(Stack24 stk, int sp)
{
    return (int)((unsigned)stk.lo[sp * 256] | ((unsigned)stk.hi[sp * 256] << 16));
}
// the stack of a queue-kernel instantiation: size and kind from its table row
template <int QB, bool OPQ>
__device__ __forceinline__ auto bvh_stack_for_q()
{
    if constexpr (queue_variant(QB, OPQ).stack24) return bvh_stack_qw();      // (QB_WIDE is the one such row)
    else return bvh_stack_q<QB, OPQ>();
}
// ... and the QB_TOP block's copy of the tree's top nodes (RT_QB_TOP x 128 B)
template <int N>
__device__ __forceinline__ BvhNode4* bvh_top_q()
{
    __shared__ BvhNode4 top_lds[N > 0 ? N : 1];
    return top_lds;
}
// Conservative single-precision slab test (the culling only has to be a
// superset of the double test on the padded boxes).  Per ray
// and axis: inv = rcp((float)d) (|d| clamped to >= 2^-60; <= 2 ulp of 1/d),
// and the offsets a = -(float)o * inv - E, b = -(float)o * inv + E with
//   E = 2^-19 (rbox + |(float)o|) |inv|,
// rbox >= every |bound| of the tree.  The entry plane of an axis is the lo
// bound when inv >= 0 and the hi bound when inv < 0 (the other is the exit
// plane), so with P the entry and Q the exit bound, fma(P, inv, a) and
// fma(Q, inv, b) lie below / above the exact (P - o) / d and (Q - o) / d:
// the rounding of d, o, inv, o*inv, the offsets and the fma together stay
// within 6 u (rbox + |o|) |inv| + 2 u E < E / 5 (u = 2^-24).  (These are the
// min and max of the two plane distances: lo <= hi and a < b order them.)
// The cull thresholds are rounded outward in the same way.
// Rays whose origin lies beyond the radius R_b the tree's padding assumed
// (kp.bvh_rb: the triangles' coordinate bound, raised over the spheres that
// cost the padding little, rt_bvh.cpp bvh_origin_radius) -- the camera, hit
// points on main.c:346's radius-1e5 sky sphere -- get the rest of the slack
// per ray: with R' = max(R_b, |o|_inf) every triangle's padding delta(R) grows
// by at most kdelta (R' - R_b) (delta is affine in R with slope 4 2^-44 1e6
// (e1+e2)^2 + 2^-48 <= kdelta, host), i.e. the ray's entry (exit) plane
// distances move down (up) by that over |d| per axis, and the distance slack
// S_abs = s_rel R grows by s_rel (R' - R_b), which lowers every entry distance
// and raises every exit distance by as much (the box test max(tmin, -S_abs)
// <= min(tmax, best (1 + s_rel) + S_abs) then holds for the larger S_abs).
// Both fold into the offsets a, b once per ray; the per-node test is unchanged.
struct Ray32 {
    float ix, iy, iz;            // ~1/d
    float ax, ay, az;            // offsets of the entry planes (lower bounds)
    float bx, by, bz;            // offsets of the exit planes (upper bounds)
};
__device__ __forceinline__ void ray32_axis(double oc, double dc, float rbox, float& inv, float& a, float& b)
{
    const double lim = 0x1p-60;
    const float df = (float)(fabs(dc) < lim ? copysign(lim, dc) : dc);
    inv = __builtin_amdgcn_rcpf(df);
    const float of = (float)oc;
    const float oi = of * inv;
    const float E = 0x1p-19f * ((rbox + fabsf(of)) * fabsf(inv));
    a = -oi - E;
    b = -oi + E;
}
// FAR: compiled into the kernels that may meet such origins (the non-opaque
// deep-tree queue kernel and the fixed-grid ones); plan_render gives the
// others (C4's OPQ kernel, QB 4) only launches with kp.bvh_far 0.
template <bool FAR = true>
__device__ __forceinline__ Ray32 ray32(const KParams& kp, const V3 o, const V3 d)
{
    Ray32 r;
    ray32_axis(o.x, d.x, kp.bvh_rbox, r.ix, r.ax, r.bx);
    ray32_axis(o.y, d.y, kp.bvh_rbox, r.iy, r.ay, r.by);
    ray32_axis(o.z, d.z, kp.bvh_rbox, r.iz, r.az, r.bz);
    // |(float)o| <= rb_f (host: rb_f (1 + 2^-23) <= R_b) puts o inside R_b;
    // the others take the exact excess (NaN origins miss every box anyway).
    // The float roundings of the widened offsets stay inside E's slack.
    // kp.bvh_far 0 (host: the camera and every sphere lie inside R_b, so every
    // ray origin does): one scalar branch per ray instead of the test.
    if (!FAR || !kp.bvh_far) return r;
    const float omf = fmaxf(fabsf((float)o.x), fmaxf(fabsf((float)o.y), fabsf((float)o.z)));
    if (!(omf <= kp.bvh_rb_f)) {
        const double ex = fmax(fmax(fabs(o.x), fmax(fabs(o.y), fabs(o.z))) - kp.bvh_rb, 0.0);
        const float dpad = (float)(kp.bvh_kdelta * ex) * (1.0f + 0x1p-20f);
        const float sx = (float)(kp.bvh_srel * ex) * (1.0f + 0x1p-20f);
        const float px = fmaf(dpad, fabsf(r.ix), sx), py = fmaf(dpad, fabsf(r.iy), sx),
                    pz = fmaf(dpad, fabsf(r.iz), sx);
        r.ax -= px; r.bx += px;
        r.ay -= py; r.by += py;
        r.az -= pz; r.bz += pz;
    }
    return r;
}
// float(best * srel + sabs) rounded up (the triangle test's distance cull)
__device__ __forceinline__ float cull32(const KParams& kp, double best)
{
    return (float)fma(best, 1.0 + kp.bvh_srel, kp.bvh_sabs) * (1.0f + 0x1p-22f);
}
// The four child boxes of a node: hit flags and near distances.  The entry
// and exit planes of each axis are picked by the sign of inv (one 16-byte
// row of lo or hi per axis: BvhNode4 stores lo[3][4] then hi[3][4]).
// Node rows of the HBM tree at 32-bit byte offsets from the tree's
// wave-uniform base: the loads take the scalar-base + 32-bit vector-offset
// form, one v_add_u32 per row instead of 64-bit address arithmetic.
__device__ __forceinline__ float4 bvh_row(const KParams& kp, uint32_t off)
{
    return *(const float4*)((const char*)kp.bvh + off);
}
// nd: the node (an LDS or generic pointer); or, with nd == nullptr, the HBM
// node at byte offset nb (C4 +2.3 %, sweep +1.2 % over 64-bit addresses)
__device__ __forceinline__ void box4(const KParams& kp, const BvhNode4* nd, const Ray32& r, float cull, bool h[4],
                                     float tn[4], int Ch[4], int Cn[4], uint32_t nb = 0)
{
    const float nsabs = (float)(-kp.bvh_sabs) * (1.0f + 0x1p-22f);
    const float4* rows = (const float4*)nd;             // rows 0-2: lo x/y/z, rows 3-5: hi x/y/z
    const int sx = (int)(__float_as_uint(r.ix) >> 31) * 3, sy = (int)(__float_as_uint(r.iy) >> 31) * 3,
              sz = (int)(__float_as_uint(r.iz) >> 31) * 3;
    float4 px, py, pz, qx, qy, qz;
    int4 cnt4;
    if (nd == nullptr) {
        px = bvh_row(kp, nb + (uint32_t)(sx * 16));
        py = bvh_row(kp, nb + (uint32_t)((1 + sy) * 16));
        pz = bvh_row(kp, nb + (uint32_t)((2 + sz) * 16));
        qx = bvh_row(kp, nb + (uint32_t)((3 - sx) * 16));
        qy = bvh_row(kp, nb + (uint32_t)((4 - sy) * 16));
        qz = bvh_row(kp, nb + (uint32_t)((5 - sz) * 16));
        const float4 c4 = bvh_row(kp, nb + (uint32_t)offsetof(BvhNode4, count));
        const float4 h4 = bvh_row(kp, nb + (uint32_t)offsetof(BvhNode4, child));
        cnt4 = make_int4(__float_as_int(c4.x), __float_as_int(c4.y), __float_as_int(c4.z), __float_as_int(c4.w));
        Ch[0] = __float_as_int(h4.x); Ch[1] = __float_as_int(h4.y); Ch[2] = __float_as_int(h4.z); Ch[3] = __float_as_int(h4.w);
    } else {
        px = rows[sx]; py = rows[1 + sy]; pz = rows[2 + sz];
        qx = rows[3 - sx]; qy = rows[4 - sy]; qz = rows[5 - sz];
        cnt4 = make_int4(nd->count[0], nd->count[1], nd->count[2], nd->count[3]);
        for (int c = 0; c < 4; ++c) Ch[c] = nd->child[c];
    }
    Cn[0] = cnt4.x; Cn[1] = cnt4.y; Cn[2] = cnt4.z; Cn[3] = cnt4.w;
    const float Px[4] = {px.x, px.y, px.z, px.w}, Py[4] = {py.x, py.y, py.z, py.w}, Pz[4] = {pz.x, pz.y, pz.z, pz.w};
    const float Qx[4] = {qx.x, qx.y, qx.z, qx.w}, Qy[4] = {qy.x, qy.y, qy.z, qy.w}, Qz[4] = {qz.x, qz.y, qz.z, qz.w};
    // box4h's slab loop, with the ray's own offsets
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float tmin = fmaxf(fmaxf(fmaf(Px[c], r.ix, r.ax), fmaf(Py[c], r.iy, r.ay)), fmaf(Pz[c], r.iz, r.az));
        const float tmax = fminf(fminf(fmaf(Qx[c], r.ix, r.bx), fmaf(Qy[c], r.iy, r.by)), fmaf(Qz[c], r.iz, r.bz));
        h[c] = Cn[c] >= 0 && fmaxf(tmin, nsabs) <= fminf(tmax, cull);     // (see box4h)
        tn[c] = tmin;
    }
}

// box4 on the 64-byte node (BvhNodeH, the queue kernel's): each plane is
// org + rel with binary16 org and rel (rt_bvh.h), so the entry distance is
// fma(rel, inv, A) with A = fma(org, inv, a) per axis and node, the halves
// read straight into v_fma_mix_f32.  Against box4's single fma the extra
// rounding of A adds at most u(|org| + |o|)|inv| + uE (u = 2^-24), and
// with rbox >= |org| + |rel| (host) the total stays below E / 3.
__device__ __forceinline__ float h16lo(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)); }
__device__ __forceinline__ float h16hi(uint32_t w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
// WIDE: the node is a BvhNodeW (rt_bvh.h) read from kp.bvhw: the same planes,
// origin and counts, and the children from the two 32-bit bases -- internal
// child c is node_base + (internal slots before c), leaf child c starts at
// tri_base + (counts of the leaf slots before c).
template <bool WIDE = false>
__device__ __forceinline__ void box4h(const KParams& kp, const BvhNodeH* nd, uint32_t nb, const Ray32& r, float cull,
                                      bool h[4], float tn[4], int Ch[4], int Cn[4])
{
    const float nsabs = (float)(-kp.bvh_sabs) * (1.0f + 0x1p-22f);
    const uint32_t sx = (__float_as_uint(r.ix) >> 31) * 3u, sy = (__float_as_uint(r.iy) >> 31) * 3u,
                   sz = (__float_as_uint(r.iz) >> 31) * 3u;
    uint2 px, py, pz, qx, qy, qz;
    uint4 t;
    {                                                    // the whole node in four 16-byte loads (HBM at
        const uint4* q = WIDE ? (const uint4*)((const char*)kp.bvhw + nb)
                         : nd ? (const uint4*)nd                       // 32-bit offsets, or the LDS copy),
                            : (const uint4*)((const char*)kp.bvhh + nb);   // rows selected by sign
        const uint4 r0 = q[0], r1 = q[1], r2 = q[2];
        t = q[3];
        const uint2 lx = make_uint2(r0.x, r0.y), ly = make_uint2(r0.z, r0.w), lz = make_uint2(r1.x, r1.y);
        const uint2 hx = make_uint2(r1.z, r1.w), hy = make_uint2(r2.x, r2.y), hz = make_uint2(r2.z, r2.w);
        px = sx ? hx : lx; qx = sx ? lx : hx;
        py = sy ? hy : ly; qy = sy ? ly : hy;
        pz = sz ? hz : lz; qz = sz ? lz : hz;
    }
    const float Ax = fmaf(h16lo(t.x), r.ix, r.ax), Ay = fmaf(h16hi(t.x), r.iy, r.ay), Az = fmaf(h16lo(t.y), r.iz, r.az);
    const float Bx = fmaf(h16lo(t.x), r.ix, r.bx), By = fmaf(h16hi(t.x), r.iy, r.by), Bz = fmaf(h16lo(t.y), r.iz, r.bz);
    const uint32_t cn = t.y >> 16;
    if constexpr (WIDE) {
        uint32_t nn = t.z, kk = t.w;                     // next internal child, next leaf's first triangle
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t nib = (cn >> (4 * c)) & 15u;
            Ch[c] = (int)(nib == 0u ? nn : kk);
            nn += nib == 0u ? 1u : 0u;
            kk += nib == 15u || nib == 0u ? 0u : nib;
        }
    } else {
        Ch[0] = (int)(t.z & 0xffffu); Ch[1] = (int)(t.z >> 16); Ch[2] = (int)(t.w & 0xffffu); Ch[3] = (int)(t.w >> 16);
    }
    const float Px[4] = {h16lo(px.x), h16hi(px.x), h16lo(px.y), h16hi(px.y)};
    const float Py[4] = {h16lo(py.x), h16hi(py.x), h16lo(py.y), h16hi(py.y)};
    const float Pz[4] = {h16lo(pz.x), h16hi(pz.x), h16lo(pz.y), h16hi(pz.y)};
    const float Qx[4] = {h16lo(qx.x), h16hi(qx.x), h16lo(qx.y), h16hi(qx.y)};
    const float Qy[4] = {h16lo(qy.x), h16hi(qy.x), h16lo(qy.y), h16hi(qy.y)};
    const float Qz[4] = {h16lo(qz.x), h16hi(qz.x), h16lo(qz.y), h16hi(qz.y)};
    // box4's slab loop, with the node origin folded into the offsets
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int nib = (int)((cn >> (4 * c)) & 15u);
        Cn[c] = nib == 15 ? -1 : nib;
        const float tmin = fmaxf(fmaxf(fmaf(Px[c], r.ix, Ax), fmaf(Py[c], r.iy, Ay)), fmaf(Pz[c], r.iz, Az));
        const float tmax = fminf(fminf(fmaf(Qx[c], r.ix, Bx), fmaf(Qy[c], r.iy, By)), fmaf(Qz[c], r.iz, Bz));
        // tmin <= tmax && tmax >= -sabs && tmin <= cull as max(tmin, -sabs) <=
        // min(tmax, cull): the same three tests (-sabs < 0 <= cull), one comparison
        h[c] = nib != 15 && fmaxf(tmin, nsabs) <= fminf(tmax, cull);
        tn[c] = tmin;
    }
}

// One node visit (bvh_visit): the four child boxes, the triangles of the hit
// leaves, then the next node (nearest hit internal child, else the stack top).
// Returns false when the traversal is over.  Every other hit internal child goes
// to the caller's sink other(node, its entry distance): bvh_step pushes it on
// the lane's stack (bvh_push); the fixed grid's cooperative walk (samples_coop,
// rt_fixed_grid.h) hands it to the wave's LIFO while that has room.  tris_bvh
// loops bvh_step to the end; the queue kernel (render_kernel_q) and samples_coop
// run a bounded number of visits per round.
__device__ __forceinline__ float* diag_lds()
{
    __shared__ float dg_lds[RT_DIAG_STALE ? 17 * 256 : 1];
    return dg_lds + threadIdx.x;
}
__device__ __forceinline__ unsigned* diag_cnt()
{
    __shared__ unsigned dc_lds[RT_DIAG_STALE == 2 ? 2 * 256 : 1];
    return dc_lds + threadIdx.x;
}
// H: 0 the 128-byte nodes, 1 BvhNodeH, 2 BvhNodeW; STK: the lane's stack (a
// uint16 or uint32 column, or the QB 5 kernel's Stack24; stk_put / stk_get);
// DG: the RT_DIAG_STALE bookkeeping of a lane's own walk (entry distances of the
// node in hand, slot 16, and of the stack entries below depth 16)
template <bool COUNT, bool CU, int NTOP, int H, bool DG, class STK, class SINK>
__device__ __forceinline__ bool bvh_visit(const KParams& kp, const V3 o, const V3 d, const Ray32& r32,
                                          STK stk, int& node, int& sp, double& best, int& kind,
                                          int& win, int& win_orig, Cnt& cnt, const void* top, SINK other)
{
    if constexpr (DG) {
        float* dg = diag_lds();
        if (node == 0) dg[16 * 256] = -__builtin_huge_valf();          // the root: a new walk
        const bool stale = dg[16 * 256] > cull32(kp, best);
        if (COUNT && stale) cnt.c[RT_CNT_BVH_STACK_OVER] += 1;
        if (!COUNT) {                                                  // queue kernel: per-lane sums
            unsigned* dc = diag_cnt();
            dc[0] += 1u;
            dc[256] += stale ? 1u : 0u;
        }
    }
    // NTOP > 0: the first NTOP nodes (breadth-first: the top levels) are read
    // from the block's LDS copy `top`, the rest from HBM/L2; H: 64-byte nodes
    if (COUNT) {
        cnt.c[RT_CNT_BVH_NODES] += 1;
        wave_slots(cnt, RT_CNT_BVH_LANE_SLOTS);
    }
    bool h[4];
    float tn[4];
    int Ch[4], Cn[4];
    const bool in_top = NTOP > 0 && node < NTOP;
    if (H == 2)
        box4h<true>(kp, nullptr, (uint32_t)node * (uint32_t)sizeof(BvhNodeW), r32, cull32(kp, best), h, tn, Ch, Cn);
    else if (H)
        box4h(kp, in_top ? (const BvhNodeH*)top + node : nullptr, (uint32_t)node * (uint32_t)sizeof(BvhNodeH), r32,
              cull32(kp, best), h, tn, Ch, Cn);
    else
        box4(kp, in_top ? (const BvhNode4*)top + node : nullptr, r32, cull32(kp, best), h, tn, Ch, Cn,
             (uint32_t)node * (uint32_t)sizeof(BvhNode4));
    int next = -1;
    float tnext = 0.0f;
    unsigned lm = 0;                                     // hit leaf slots
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (!h[c]) continue;
        const int ch = Ch[c], n = Cn[c];
        if (n > 0) {
            lm |= 1u << c;
        } else if (next < 0) {
            next = ch;
            tnext = tn[c];
        } else {
            int push = ch;
            float tpush = tn[c];
            if (tn[c] < tnext) {                         // nearer: enter it, push the previous pick
                push = next;
                tpush = tnext;
                next = ch;
                tnext = tn[c];
            }
            other(push, tpush);
        }
    }
    // The triangles of every hit leaf in one loop, one triangle per lane and
    // iteration: the wave runs max-over-lanes iterations instead of one
    // divergent loop per child slot.
    int k = 0, kend = 0;
    while (lm != 0u || k < kend) {
        if (COUNT) wave_slots(cnt, RT_CNT_LEAF_LANE_SLOTS);
        if (k >= kend) {
            const int c = __ffs(lm) - 1;
            lm &= lm - 1u;
            k = c == 0 ? Ch[0] : c == 1 ? Ch[1] : c == 2 ? Ch[2] : Ch[3];
            kend = k + (c == 0 ? Cn[0] : c == 1 ? Cn[1] : c == 2 ? Cn[2] : Cn[3]);
            if (COUNT) cnt.c[RT_CNT_BVH_TRI_TESTS] += (unsigned long long)(kend - k);
        }
        tri_test<COUNT, CU, true>(kp, k, o, d, best, kind, win, win_orig);
        ++k;
    }
    if (next >= 0) {
        node = next;
        if (DG) diag_lds()[16 * 256] = tnext;
        return true;
    }
    if (sp == 0) return false;
    --sp;
    node = stk_get(stk, sp);
    if (DG) diag_lds()[16 * 256] = sp < 16 ? diag_lds()[sp * 256] : -__builtin_huge_valf();
    return true;
}

// A hit internal child that is not entered next, onto the lane's stack (tpush:
// its entry distance).  COUNT walks use the fixed grid's stack and check every
// push against the stack of the kernel the launch would take (kp.stack_cap).
template <bool COUNT, bool DG, class STK>
__device__ __forceinline__ void bvh_push(const KParams& kp, STK stk, int& sp, int push, float tpush, Cnt& cnt)
{
    if (!RT_DIAG_STALE && COUNT && sp >= kp.stack_cap) cnt.c[RT_CNT_BVH_STACK_OVER] += 1;
    if (!COUNT || sp < kStack4) {
        if (DG && sp < 16) diag_lds()[sp * 256] = tpush;
        stk_put(stk, sp, push);
        ++sp;
    }
}

// A node visit of a lane's own walk: the other children go on its stack.
template <bool COUNT, bool CU, int NTOP = 0, int H = 0, class STK>
__device__ __forceinline__ bool bvh_step(const KParams& kp, const V3 o, const V3 d, const Ray32& r32,
                                         STK stk, int& node, int& sp, double& best, int& kind,
                                         int& win, int& win_orig, Cnt& cnt, const void* top = nullptr)
{
    constexpr bool DG = RT_DIAG_STALE && (COUNT || RT_DIAG_STALE == 2);
    return bvh_visit<COUNT, CU, NTOP, H, DG>(kp, o, d, r32, stk, node, sp, best, kind, win, win_orig, cnt, top,
                                            [&](int push, float tpush) __attribute__((always_inline)) {
                                                bvh_push<COUNT, DG>(kp, stk, sp, push, tpush, cnt);
                                            });
}

template <bool COUNT, bool CU, class SE = unsigned short>
__device__ __forceinline__ void tris_bvh(const KParams& kp, const V3 o, const V3 d, double& best, int& kind,
                                         int& win, int& win_orig, Cnt& cnt)
{
    SE* stk = bvh_stack_of<SE>();
    const Ray32 r32 = ray32(kp, o, d);
    int node = 0, sp = 0;
    while (bvh_step<COUNT, CU>(kp, o, d, r32, stk, node, sp, best, kind, win, win_orig, cnt)) {
    }
}

// closest_hit, main.c:52-92: spheres, then triangles; a strictly closer hit
// replaces the record.  Returns the winner (kind, index, t).
// hit_BBox, triangle.hu:42-59 (CU mode): IEEE divisions, CUDA's double
// min/max = fmin/fmax; the triangles are skipped when it fails.
__device__ __forceinline__ bool cuda_bbox(const KParams& kp, const V3 o, const V3 d)
{
    const double t1x = (kp.cbb[0] - o.x) / d.x, t2x = (kp.cbb[3] - o.x) / d.x;
    const double t1y = (kp.cbb[1] - o.y) / d.y, t2y = (kp.cbb[4] - o.y) / d.y;
    const double t1z = (kp.cbb[2] - o.z) / d.z, t2z = (kp.cbb[5] - o.z) / d.z;
    const double tmax = fmin(fmin(fmax(t1x, t2x), fmax(t1y, t2y)), fmax(t1z, t2z));
    const double tmin = fmax(fmax(fmin(t1x, t2x), fmin(t1y, t2y)), fmin(t1z, t2z));
    return tmax - tmin > 0;
}

// The sphere half of closest_hit (and the cast counters): the winner index
// or -1, its t in best (+inf when none).
// HB: the exact tests in half-b units (rt_shared_math.h sphere_halfb), which read a where the
// reference form reads 2a and 4a
template <unsigned F>
__device__ __forceinline__ int cast_spheres(const KParams& kp, const V3 o, const V3 d, double& best, Cnt& cnt)
{
    constexpr bool COUNT = (F & CF_COUNT) != 0, HB = (F & CF_HALFB) != 0;
    const double a = dot(d, d);          // sphere.h:20 (same for every sphere)
    const double two_a = HB ? a : 2 * a; // sphere.h:27,36
    const double four_a = 4 * a;         // sphere.h:24
    const bool fast = HB ? halfb_fast_a(a) : two_a >= 0x1p-100 && two_a <= 0x1p100;
    const double rc2a = rcp_refined(two_a);
    if (COUNT) {
        cnt.c[RT_CNT_CASTS] += 1;
        cnt.c[RT_CNT_SPHERE_TESTS] += (unsigned long long)kp.ns;
        cnt.c[RT_CNT_TRI_TESTS] += (unsigned long long)kp.nt;
        wave_slots(cnt, RT_CNT_CAST_LANE_SLOTS);
    }
    int win = spheres_closest<F>(kp, o, d, a, two_a, four_a, fast, rc2a, best, cnt);
    return win;
}

// F: CF_COUNT, CF_CUDA, CF_AMGM, CF_BVH; SE: the BVH stack's element type (uint32_t for a wide tree, rt_bvh.h)
template <unsigned F, class SE = unsigned short>
__device__ __forceinline__ int closest_hit(const KParams& kp, const V3 o, const V3 d, double& t_best, int& idx,
                                           Cnt& cnt)
{
    constexpr bool COUNT = (F & CF_COUNT) != 0, BVH = (F & CF_BVH) != 0, CU = (F & CF_CUDA) != 0;
    double best;
    // the flagged-pair loop (spheres_closest MG) wherever no BVH walk follows
    int win = cast_spheres<(F & ~CF_BVH) | cf(!BVH, CF_PAIRS)>(kp, o, d, best, cnt);
    int kind = win >= 0 ? HIT_SPHERE : HIT_NONE;
    int win_orig = 0;
    if (CU && kp.nt > 0 && !cuda_bbox(kp, o, d)) {
        // main_cuda.cu:40-45: the ray misses the mesh box, no triangle tested
        // (cast_spheres counted main.c's every-triangle scan: taken back)
        if (COUNT) cnt.c[RT_CNT_TRI_TESTS] -= (unsigned long long)kp.nt;
    } else if (BVH) {
        tris_bvh<COUNT, CU, SE>(kp, o, d, best, kind, win, win_orig, cnt);
    } else if (!COUNT && !kp.tri_orig) {
        for (int k = 0; k < kp.nt; ++k) tri_test_bf<CU>(kp, k, o, d, best, kind, win);
    } else {
        for (int k = 0; k < kp.nt; ++k) tri_test<COUNT, CU, false, true>(kp, k, o, d, best, kind, win, win_orig);
    }
    t_best = best;
    idx = win;
    return kind;
}

}  // namespace rt
