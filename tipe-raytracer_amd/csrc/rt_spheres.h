// rt_spheres.h -- hit_sphere (sphere.h:13-47) and the sphere candidate pass (spheres_closest).
// Part of the single translation unit rt_kernels.hip (included there, in this order).
#pragma once

namespace rt {

// hit_sphere, sphere.h:13-47, exact reference arithmetic.  two_a = 2*a and
// four_a = 4*a with a = dot(d, d) (`4*a*c` == (4*a)*c).  A negative
// numerator decides t < 1e-4 without the division (2a > 0).
//
// With fast (two_a in [2^-100, 2^100], rc2a = rcp_refined(two_a)) the
// divisions run div_core: a hit needs n >= 1e-4*two_a >> 2^-900, and
// disc <= 2^760 bounds |n| by 2^512, so every quotient that can decide or
// become t is exact; smaller n give t < 1e-4 on both paths.
// CU: main_cuda.cu's hit_sphere (sphere.hu:27-45), t1 >= 0 then t2 >= 0.001;
// its t1 may be tiny, so the fast division also needs |n| >= 2^-900 there.
template <bool CU>
__device__ __forceinline__ bool sphere_exact(double cx, double cy, double cz, double r2, const V3 o, const V3 d,
                                             double two_a, double four_a, bool fast, double rc2a, double& t)
{
    const double e1 = CU ? 0.0 : 0.0001, e2 = CU ? 0.001 : 0.0001;
    const double ocx = o.x - cx, ocy = o.y - cy, ocz = o.z - cz;
    const double b = 2.0 * (ocx * d.x + ocy * d.y + ocz * d.z);
    const double c = (ocx * ocx + ocy * ocy + ocz * ocz) - r2;
    const double disc = b * b - four_a * c;
    if (!(disc > 0)) return false;
    const bool f = fast && disc >= 0x1p-760 && disc <= 0x1p760;
    double sq;
    if (f) sq = sqrt_core(disc);
    else sq = sqrt(disc);
    const double n1 = -b - sq;
    if (!(n1 < 0.0)) {
        if (f && (!CU || n1 >= 0x1p-900)) t = div_core(n1, two_a, rc2a);
        else t = n1 / two_a;
        if (t >= e1) return true;
    }
    const double n2 = -b + sq;
    if (!(n2 < 0.0)) {
        if (f && (!CU || n2 >= 0x1p-900)) t = div_core(n2, two_a, rc2a);
        else t = n2 / two_a;
        if (t >= e2) return true;
    }
    return false;
}

// (HB: the sphere-only queue kernel's paired-draw form) sphere_exact in half-b
// units, rt_shared_math.h sphere_halfb with the exact cores above: fast is
// halfb_fast_a(a) and rca = rcp_refined(a).  A lane outside its windows runs
// the reference form as it stands, and without its fast path.
struct HalfbCores {
    __device__ __forceinline__ static double sqrt_in(double x) { return sqrt_core(x); }
    __device__ __forceinline__ static double div_in(double x, double d, double rc) { return div_core(x, d, rc); }
    __device__ __forceinline__ static bool reference(double cx, double cy, double cz, double r2, const V3 o, const V3 d,
                                                     double a, double& t)
    {
        return sphere_exact<false>(cx, cy, cz, r2, o, d, 2 * a, 4 * a, false, 0.0, t);
    }
};
__device__ __forceinline__ bool sphere_exact_hb(double cx, double cy, double cz, double r2, const V3 o, const V3 d,
                                                double a, bool fast, double rca, double& t)
{
    return sphere_halfb<HalfbCores>(cx, cy, cz, r2, o, d, a, fast, rca, t);
}

// The reference's discriminant sign (sphere.h:24-25): COUNT statistics only.
__device__ __forceinline__ bool disc_positive(const SphGeo& s, const V3 o, const V3 d, double four_a)
{
    const double ocx = o.x - s.cx, ocy = o.y - s.cy, ocz = o.z - s.cz;
    const double b = 2.0 * (ocx * d.x + ocy * d.y + ocz * d.z);
    const double c = (ocx * ocx + ocy * ocy + ocz * ocz) - s.r2;
    return b * b - four_a * c > 0;
}

// What a cast is compiled for: the one template parameter of cast_spheres,
// spheres_closest, spheres_exact_scan and closest_hit (rt_triangles.h), or-ed
// from these bits, so that a call site names what it switches on.  (In
// brackets: the names the functions give the bits; each explains its own.)
enum : unsigned {
    CF_NONE = 0u,         // main.c's thresholds, no counters, the plain candidate loop, no BVH
    CF_COUNT = 1u << 0,   // [COUNT] the RT_CNT_* counters
    CF_CUDA = 1u << 1,    // [CU] main_cuda.cu's thresholds
    CF_AMGM = 1u << 2,    // [AMGM] Hs from sqrt(a) <= (1 + a)/2; takes CF_PAIRS with it
    CF_PAIRS = 1u << 3,   // [MG] the candidate pass's pair loops
    CF_HALFB = 1u << 4,   // [HB] the exact tests in half-b units; without CF_COUNT and CF_CUDA
    CF_BVH = 1u << 5,     // [BVH] closest_hit alone: the triangles by the BVH walk
};
constexpr unsigned cf(bool on, unsigned bits) { return on ? bits : CF_NONE; }

// Exact reference scan over every sphere (main.c:59-78 with hit_sphere).
// HB: sphere_exact_hb, with a in two_a's place and rcp_refined(a) in rc2a's (cast_spheres).
template <unsigned F>
__device__ __forceinline__ int spheres_exact_scan(const KParams& kp, const V3 o, const V3 d, double two_a,
                                                  double four_a, bool fast, double rc2a, double& t_best)
{
    constexpr bool CU = (F & CF_CUDA) != 0, HB = (F & CF_HALFB) != 0;
    const cdptr sg = (cdptr)kp.sph;
    double t = dinf();
    int win = -1;
    for (int k = 0; k < kp.ns_pad; ++k) {
        double tk;
        bool hit;
        const double cx = sg[4 * k], cy = sg[4 * k + 1], cz = sg[4 * k + 2], r2 = sg[4 * k + 3];
        if constexpr (HB) hit = sphere_exact_hb(cx, cy, cz, r2, o, d, two_a, fast, rc2a, tk);
        else hit = sphere_exact<CU>(cx, cy, cz, r2, o, d, two_a, four_a, fast, rc2a, tk);
        if (hit && tk < t) {
            t = tk;
            win = k;
        }
    }
    t_best = t;
    return win;
}

// ---- The pieces of the sphere candidate pass (spheres_closest, below) ----

// The candidate's n with its low 16 mantissa bits replaced by sphere slot k:
// one v_and_or_b32 with the mask in a VGPR (msk, loop-invariant; a literal
// would split it into v_and + v_or) and the wave-uniform slot as its one
// scalar operand.  Host: ns_cand <= 65534; |nt - n| < 2^-36 |n| <= 2^-34.4 Hs,
// inside M's slack.
__device__ __forceinline__ double cand_tag(double n, int k, uint32_t msk)
{
    uint32_t lo;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(lo) : "v"((uint32_t)__double2loint(n)), "v"(msk), "s"(k));
    return __hiloint2double(__double2hiint(n), (int)lo);
}

// min(a, |b|) with an abs source modifier (a >= 0; a NaN b drops out, which
// only happens for a NaN D: non-finite inputs are already ambiguous)
__device__ __forceinline__ double dmin_abs2(double a, double b)
{
    double r;
    asm("v_min_f64 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// v_min_f64 / v_max_f64 of two finite, non-NaN operands (the candidate
// pass's tagged values): fmin/fmax would first canonicalize the bit-built
// operand (an extra v_max_f64 x, x each).
__device__ __forceinline__ double dmin_raw(double a, double b)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double dmax_raw(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a = min(a, b) in a's own register: a loop-carried minimum that is updated on
// two sides of a branch otherwise ends in a v_mov_b64 per side at the latch
__device__ __forceinline__ void dmin_acc(double& a, double b)
{
    asm("v_min_f64 %0, %0, %1" : "+v"(a) : "v"(b));
}

// a = min(a, |b|) in a's own register (dmin_abs2's conditions, dmin_acc's reason)
__device__ __forceinline__ void dmin_abs_acc(double& a, double b)
{
    asm("v_min_f64 %0, %0, |%1|" : "+v"(a) : "v"(b));
}

// main.c:214's `r.x > 0.5 || r.y > 0.5 || r.z > 0.5` as max(x, y, z) > 0.5
// (a NaN component drops out of v_max_f64 exactly as it fails its own
// comparison; the throughputs are arithmetic results, never signalling
// NaNs).  The compiler makes the same fold itself, but through fmax, which
// canonicalizes all three operands first: 6 VALU instead of 3.
__device__ __forceinline__ bool any_above_half(V3 r)
{
    return dmax_raw(dmax_raw(r.x, r.y), r.z) > 0.5;
}

// tools/merge_share.py (RT_DIAG_MERGE builds): the per-wave counters of the pair
// loops' wave-casts that ran one root tail or two; render_kernel_q (rt_queue.h)
// clears them and writes them into its trace record.
enum DiagMerge { DM_FLAGGED_ONE = 0, DM_FLAGGED_TWO = 4, DM_FORWARD_ONE = 8, DM_FORWARD_TWO = 12 };
#if RT_DIAG_MERGE
// one counter per wave of the block (every active lane adds the same
// wave-uniform step)
__device__ __forceinline__ unsigned* diag_merge()
{
    __shared__ unsigned dm_lds[16];
    return dm_lds + (threadIdx.x >> 6);
}
#endif

// A sphere that is no candidate enters the two minima as a sentinel: finite,
// above 2^1000 (this high word), its low word the tag it would have had.  The
// decisions after the scan only ask whether a minimum is a sentinel, which is
// whether it is above kCandNone (every candidate's n is below: Hs^2 <= 2^1000).
constexpr int kSentinelHi = 0x7fefffff;
constexpr double kCandNone = 0x1p600;

// What one ray's scan keeps per sphere record g = {C, k} (k = |C|^2 - r2 from
// the host), in the half-b form of spheres_closest's header:
//   h  = od - C.d                       (3 fma; od = o.d per ray)
//   ca = a|o|^2 - 2a o.C + a*k          (4 fma)
// and D = fma(h, h, -ca); thrM and msk are what a root tail reads.
struct CandRay {
    V3 d;
    double od, a, aoo, oax, oay, oaz;    // o.d, |d|^2, a|o|^2, -2a o
    double thrM;                         // thr1 - M: a root at or above it may reach the threshold
    uint32_t msk;                        // cand_tag's mask
    __device__ __forceinline__ double h(const double* g) const
    {
        return fma(-g[2], d.z, fma(-g[1], d.y, fma(-g[0], d.x, od)));
    }
    __device__ __forceinline__ double ca(const double* g) const
    {
        return fma(g[2], oaz, fma(g[1], oay, fma(g[0], oax, fma(a, g[3], aoo))));
    }
};

// The root of one sphere from h and D, chosen as hit_sphere chooses: n1 if it
// may reach the threshold (r1), else n2.
template <bool AMGM>
__device__ __forceinline__ double cand_root(double h, double D, double thrM, bool& r1)
{
    // sa ~ sqrt(D): v_rsq_f64 + one Newton step (sa = t + t*e/2)
    const double r0 = __builtin_amdgcn_rsq(D);
    const double tt = D * r0;
    const double sa = fma(tt * 0.5, fma(-tt, r0, 1.0), tt);
    const double n1 = -h - sa;
    r1 = n1 >= thrM;                                // n1 may reach 1e-4: hit_sphere takes t1
    // the chosen root: n1 = -h - sa, or n2 = -h + sa; in the sphere-scene queue
    // kernel (AMGM) as one fma with a selected sign (s * sa is exact; C2
    // +0.7 %), elsewhere a select (the fma's constants cost the BVH
    // instantiations registers: sweep -1.4 %)
    return AMGM ? fma(r1 ? -1.0 : 1.0, sa, -h) : (r1 ? n1 : sa - h);
}

// (MN) The root tail of one sphere of the candidate scan: its tagged
// candidate from h and D, or the sentinel with that tag.
// Candidates: every chosen root that may reach 1e-4 (n >= thr - M),
// straddling ones included -- they are below any sure root, so the winner's
// own test after the scan (bn < thrP) catches them.
// A sphere with !(D > 0) gives the sentinel: rsq of a non-positive D is NaN or
// inf, D * r0 and with it n is NaN, and n >= thrM fails.
template <bool AMGM>
__device__ __forceinline__ double cand_tail(const CandRay& r, double h, double D, int k)
{
    bool r1;
    const double n = cand_root<AMGM>(h, D, r.thrM, r1);
    const double nt = cand_tag(n, k, r.msk);
    return __hiloint2double(n >= r.thrM ? __double2hiint(nt) : kSentinelHi, __double2loint(nt));
}

// (MN) bn and bn2 stay the smallest and the second-smallest tagged candidate
// with nc among them.
__device__ __forceinline__ void cand_keep(double& bn, double& bn2, double nc)
{
    bn2 = dmin_raw(bn2, dmax_raw(bn, nc));
    bn = dmin_raw(bn, nc);
}
// ... in their own registers (dmin_acc): the update on one side of a branch
__device__ __forceinline__ void cand_keep_acc(double& bn, double& bn2, double nb)
{
    dmin_acc(bn2, dmax_raw(bn, nb));
    dmin_acc(bn, nb);
}

// A pair's second tail, sphere k + 1's, which runs only when the wave does not
// merge: updating bn and bn2 in place, so nothing has two definitions that
// meet at the latch (a v_mov_b64 each).
template <bool AMGM>
__device__ __forceinline__ void cand_second_tail(const CandRay& r, double h1, double D1, int k, double& bn,
                                                 double& bn2)
{
    cand_keep_acc(bn, bn2, cand_tail<AMGM>(r, h1, D1, k + 1));
}

// Closest sphere (main.c:59-78): an FMA candidate pass with rigorous error
// intervals picks the winner, whose exact reference test then runs alone;
// any ambiguity reruns the exact scan for that ray (DESIGN.md "Exact closest
// hit").  Half-b form: h = (o-C).d, D = h^2 - a*c, roots n1,2 = -h -/+ sqrt(D)
// with t = n/a (the reference's t1,2 = (-b -/+ sqrt(disc))/(2a) scale
// exactly: b = 2h, disc = 4D).  Intervals are kept in n = a*t units, one
// per-ray half-width M for every sphere (CandRay: h, ca and D per record).
// Error bound: with Hs >= (|o| + L) sqrt(a), L >= |C_k| + R_k,
// |D - D_ref| <= 52.5u*Hs^2 <= 2^-47.3 Hs^2 (u = 2^-53), where D_ref =
// disc_ref/4.  Rays with D >= T1 = 2^-36 Hs^2 are resolved: the reference's
// disc > 0, and sa (v_rsq_f64 + one Newton step, <= 2^-45 relative) is within
// 2^-29.3 Hs of its rounded sqrt, so |n - n_ref| <= 2^-29.29 Hs; a*t_ref lies
// within u|n| of n_ref.  M = 2^-26 Hs (+ thr*2^-48 for the rounding of
// thr = a*1e-4) leaves a factor 9.8 of slack.  D < -T2 = -2^-44 Hs^2 is a sure
// miss; in between (grazing rays) the ray is ambiguous.  Root choice follows
// hit_sphere: n1 if it may reach 1e-4 (a straddle is ambiguous), else n2.
// Two winners closer than 2M are ambiguous, so a strictly smaller interval is
// a strictly smaller t_ref (the reference keeps the first of equal t).
// Non-finite o, d or Hs^2 > 2^1000 make the ray ambiguous up front.
// CU (main_cuda.cu's thresholds): t1 >= 0, t2 >= 0.001, one interval pair each.
//
// The pass: the per-ray set-up; the scan over the records, which are in the
// host's order (rt_scene_prep.cpp pair_candidates) -- the first ns_merge are
// flagged pairs, the next ns_fwd forward pairs, each with a loop that shares
// one root tail per pair where its rule allows, the rest take the plain loop;
// one decision after the scan.  The tag is the record's slot, and kp.sph_slot /
// kp.cand_orig give the winner's sphere.  The order and the two counts are a
// hint: every order and every ns_merge and ns_fwd give the same winner
// (tests/test_gpu_merged_tail.py, tests/test_gpu_forward_pairs.py, RT_CAND_MERGE).
// MN (every instantiation but CUDA semantics): the scan keeps the smallest and
// second-smallest tagged candidate (bn, bn2; cand_keep) and the smallest |D|
// (gmin), and ambiguity is decided once after the scan.
// MG: the pair loops are compiled in (every kernel whose cast is not
// followed by a BVH walk, and rt_verify_sphere_pass; the BVH instantiations
// keep the plain loop, which is right for any ns_merge -- with the flagged
// loop their register allocation lost 0.7 % on C4)
// HB: the winner's test and the rescan in half-b units (sphere_exact_hb): the
// caller passes a for two_a, rcp_refined(a) for rc2a and halfb_fast_a(a) for
// fast, whose window implies the one the comments here assume (2a in 2^+-100).
template <unsigned F>
__device__ __forceinline__ int spheres_closest(const KParams& kp, const V3 o, const V3 d, double a, double two_a,
                                               double four_a, bool fast, double rc2a, double& t_best, Cnt& cnt)
{
    constexpr bool COUNT = (F & CF_COUNT) != 0, CU = (F & CF_CUDA) != 0, AMGM = (F & CF_AMGM) != 0;
    constexpr bool MG = (F & (CF_PAIRS | CF_AMGM)) != 0, HB = (F & CF_HALFB) != 0;
    static_assert(!HB || (!COUNT && !CU), "half-b units: the reference thresholds, no counters");
    const cdptr sc = (cdptr)kp.sph_cand;
    const double INF = dinf();
    const double od = fma(o.z, d.z, fma(o.y, d.y, o.x * d.x));
    const double aoo = a * fma(o.z, o.z, fma(o.y, o.y, o.x * o.x));
    const double m2a = -2.0 * a;
    const double oax = m2a * o.x, oay = m2a * o.y, oaz = m2a * o.z;
    // Hs >= (|o| + L) sqrt(a): |o|_1 >= |o|_2.  AMGM (the sphere/brute-force
    // queue kernels without AO or sky): sqrt(a) <= (1 + a)/2, equal at a = 1 (the unit directions
    // of camera, bounce and AO rays; shorter lerped directions get a looser bound,
    // more rescans: 1.7e-4 per sample on C2), with 2^-50 for the fma's rounding
    // for every a >= 0 -- C2 +0.35 %; elsewhere v_rsq_f64 (within 2^-24), which
    // the BVH instantiations keep (their register allocation lost 1.9 % on C4
    // with the fma)
    const double sqa = AMGM ? fma(a, 0.5, 0.5 + 0x1p-50) : (a * __builtin_amdgcn_rsq(a)) * (1.0 + 0x1p-20);
    const double Hs = ((fabs(o.x) + fabs(o.y)) + fabs(o.z) + kp.cand_lmax) * sqa;
    const double Hs2 = Hs * Hs;
    const double T1 = Hs2 * RT_CAND_T1, nT2 = Hs2 * -0x1p-44;
    const double thr = a * 0.0001;
    const double thr1 = CU ? 0.0 : thr, thr2 = CU ? a * 0.001 : thr;
    const double M = fma(thr2, 0x1p-48, Hs * RT_CAND_M);
    const double thrP = thr1 + M, thrM = thr1 - M, M2 = 2.0 * M;
    const double thrP2 = thr2 + M, thrM2 = thr2 - M;
    double bn = INF;
    int bk;
    // finite o, d, Hs^2 keep every D below finite; anything else takes the exact scan
    bool amb = !(fast && Hs2 <= 0x1p1000);
    uint32_t msk = 0xffff0000u;
    asm volatile("" : "+v"(msk));
    const CandRay r{d, od, a, aoo, oax, oay, oaz, thrM, msk};
    constexpr bool MN = !CU;
    double bn2 = __hiloint2double(kSentinelHi, -1);
    if (MN) bn = bn2;
    double gmin = bn2;                   // (MN) min |D| over the scan
    int k = 0;
    if (MN && MG) {
        // Flagged pairs: spheres that a line rarely crosses both of.  A sphere
        // with !(D > 0) only adds a sentinel (cand_tail).  Leaving that update
        // out changes only the low bits of a sentinel in bn or bn2, which the
        // decisions after the scan (any, bn2 - bn > M2, bk) do not read
        // (kCandNone); gmin takes both D either way.  So when no lane of the wave
        // has both D > 0, one tail on each lane's own positive sphere (the
        // first when neither is) gives what the two tails give; otherwise the two
        // tails run.  The sign test reads D's high word: a positive D below 2^-1042
        // counts as not positive, and is below T1 (>= 2^-177 on a fast ray: Hs >=
        // 2^-20 sqrt(a), a >= 2^-101), where gmin makes the ray ambiguous.
        // The first tail runs on each lane's choice (sphere 0 unless the wave
        // merges and the lane's D1 > 0) and the second only when the wave does
        // not merge.  C2: 96 % of the flagged pairs' wave-casts merge, +1.6 %
        // (profiles/r07_merge/).
        for (; k < kp.ns_merge; k += 2) {
            double g[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = sc[4 * k + j];
            const double h0 = r.h(g);
            const double D0 = fma(h0, h0, -r.ca(g));
            double h1 = r.h(g + 4);
            double D1 = fma(h1, h1, -r.ca(g + 4));
            // (opaque to the compiler: paired up as two-element vectors, the two
            // spheres cost a copy of every loop-invariant operand per cast)
            asm("" : "+v"(h1), "+v"(D1));
            gmin = dmin_abs2(dmin_abs2(gmin, D0), D1);
            const int s0 = __double2hiint(D0), s1 = __double2hiint(D1);
            const bool merged = __builtin_amdgcn_ballot_w64(min(s0, s1) > 0) == 0;
#if RT_DIAG_MERGE
            diag_merge()[merged ? DM_FLAGGED_ONE : DM_FLAGGED_TWO] += 1u;
#endif
            const bool sel = merged && s1 > 0;
            double nc = cand_tail<AMGM>(r, sel ? h1 : h0, sel ? D1 : D0, k);
            // the lane's choice into the tag's low bit (k is even)
            nc = __hiloint2double(__double2hiint(nc), __double2loint(nc) + (sel ? 1 : 0));
            cand_keep(bn, bn2, nc);
            if (!merged) cand_second_tail<AMGM>(r, h1, D1, k, bn, bn2);
        }
        // Forward pairs: two spheres that a ray starting
        // between them moves towards at most one of (the README
        // box's opposite walls: D > 0 for both on almost every ray, so the test
        // above never merges them).  A lane's sphere is dead when
        //   h > hmin  and  ca > -cmin        (the computed h and ca of this scan)
        // and live otherwise, whatever its D; the wave merges when no lane is
        // live for both, and the one tail runs on the lane's live sphere (sphere
        // 0 when neither is).  With hmin = 2^-16 Hs and cmin = 2^-44 Hs^2, and on rays with thrM >= 2^-26 Hs only
        // (else hthr lets no lane certify; that covers thrM < 0), a dead
        // sphere's tail only writes a sentinel: D =
        // fl(h^2 - ca) <= (h^2 + cmin)(1 + u); D <= 0 or NaN gives the sentinel
        // (cand_tail); else sa <= sqrt(D)(1 + 2^-45) <= (h + cmin / 2h)(1 + 2^-44), and
        // with hmin < h <= 1.01 Hs
        //   n1 = -h - sa < -hmin < 0 < thrM                  (r1 is false: n = n2)
        //   n2 = fl(sa - h) <= cmin / 2hmin + 2^-43 Hs = (2^-29 + 2^-43) Hs,
        // which with the scan's whole root error 2^-29.29 Hs on top stays below
        // 2^-27 Hs < thrM, so n >= thrM fails.  cmin is 9.8 x the 2^-47.3 Hs^2 error
        // of ca: a ray leaving the wall it sits on, its ca rounding noise around
        // 0, certifies.  Both tests read high words only, and the thresholds
        // are the high words of Hs and Hs^2 with the exponent field lowered (Hs
        // >= 2^-71 on a fast ray, so nothing borrows out of it; other rays are
        // ambiguous up front, as are those with a NaN or infinite h or ca, which
        // can pass): hi(h) > hi(hmin) as signed ints -- a negative h has a
        // negative high word and fails, and two positive doubles with different
        // high words order as those do, so it implies h > hmin; (unsigned) hi(ca)
        // < 2^31 + hi(cmin) -- every ca >= 0 has a high word below 2^31 and
        // passes, and a negative ca has 2^31 + hi(|ca|), which grows with |ca|
        // (signed order reverses below zero, unsigned order of the magnitudes
        // does not), so it passes only with hi(|ca|) < hi(cmin), which implies
        // |ca| < cmin.
        // A dead sphere is dropped altogether, its D from the grazing test too
        // (the chosen sphere's h and ca are selected, and D follows): the
        // reference itself cannot hit it.  Its own h and D are within 16u Hs and
        // 2^-47.3 Hs^2 of the ones here (the bound above, which does not ask for
        // D >= T1), so D_ref <= h^2 + (2^-44 + 2^-47.2) Hs^2, its first root is
        // negative, and its second, sqrt(D_ref) - h_ref <= 1.11 x 2^-44 Hs^2 /
        // (2 x 2^-16 Hs) + 2^-48 Hs < 2^-28 Hs, is below thr - M: t2 < 1e-4.  So
        // fewer rays rescan than with both D in gmin; the winner is the same.
        constexpr double fwd_h = 1.0 / (double)(1ull << RT_FWD_HEXP), fwd_c = 1.0 / (double)(1ull << RT_FWD_CEXP);
        static_assert(RT_FWD_HEXP >= 8 && RT_FWD_HEXP <= 24 && fwd_c >= 0x1p-46 &&
                          fwd_c / (2.0 * fwd_h) + 0x1p-29 + 0x1p-43 <= RT_CAND_M / 2,
                      "forward pairs: cmin must exceed 2 x ca's error 2^-47.3 Hs^2 and the dead root stay below thrM / 2");
        const int hthr = thrM >= Hs * RT_CAND_M ? (int)((uint32_t)__double2hiint(Hs) - ((uint32_t)RT_FWD_HEXP << 20))
                                                : 0x7fffffff;
        const uint32_t cthr = (uint32_t)__double2hiint(Hs2) + (0x80000000u - ((uint32_t)RT_FWD_CEXP << 20));
        for (const int kf = kp.ns_merge + kp.ns_fwd; k < kf; k += 2) {
            double g[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = sc[4 * k + j];
            const double h0 = r.h(g), ca0 = r.ca(g);
            double h1 = r.h(g + 4), ca1 = r.ca(g + 4);
            asm("" : "+v"(h1), "+v"(ca1));               // (as in the flagged loop)
            // (a ballot per comparison: one ballot of the combined predicate goes
            // through a v_cndmask and a v_cmp_ne)
            const bool lh0 = __double2hiint(h0) <= hthr, lc0 = (uint32_t)__double2hiint(ca0) >= cthr;
            const bool lh1 = __double2hiint(h1) <= hthr, lc1 = (uint32_t)__double2hiint(ca1) >= cthr;
            const uint64_t l1 = __builtin_amdgcn_ballot_w64(lh1) | __builtin_amdgcn_ballot_w64(lc1);
            const bool merged = ((__builtin_amdgcn_ballot_w64(lh0) | __builtin_amdgcn_ballot_w64(lc0)) & l1) == 0;
#if RT_DIAG_MERGE
            diag_merge()[merged ? DM_FORWARD_ONE : DM_FORWARD_TWO] += 1u;
#endif
            const bool sel = merged && (lh1 || lc1);
            // D and the grazing test of the chosen sphere only
            const double hs = sel ? h1 : h0, cas = sel ? ca1 : ca0;
            const double Ds = fma(hs, hs, -cas);
            dmin_abs_acc(gmin, Ds);
            double nc = cand_tail<AMGM>(r, hs, Ds, k);
            // the choice into the tag's low bit, here as the carry-in of one add
            // (the wave's mask of such lanes is there already)
            uint32_t lo;
            asm("v_addc_co_u32_e64 %0, vcc, 0, %1, %2"
                : "=v"(lo)
                : "v"((uint32_t)__double2loint(nc)), "s"(merged ? l1 : (uint64_t)0)
                : "vcc");
            nc = __hiloint2double(__double2hiint(nc), (int)lo);
            cand_keep(bn, bn2, nc);
            if (!merged) {
                const double D1 = fma(h1, h1, -ca1);
                dmin_abs_acc(gmin, D1);
                cand_second_tail<AMGM>(r, h1, D1, k, bn, bn2);
            }
        }
    }
    for (; k < kp.ns_cand; k += 2) {
        double g[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = sc[4 * k + j];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double h = r.h(g + 4 * e);
            const double D = fma(h, h, -r.ca(g + 4 * e));
            // D finite here.
            // MN: one |D| < T1 test (grazing band widened from [-T2, T1) to
            // (-T1, T1)), once, after the scan; D <= -T1 gives a NaN root in
            // cand_tail, which no comparison accepts, so `valid` is implied by
            // the candidate test
            if (MN) {
                gmin = dmin_abs2(gmin, D);
                cand_keep(bn, bn2, cand_tail<AMGM>(r, h, D, k + e));
            } else {
                // CU: ambiguity is decided sphere by sphere, bn the one running
                // winner.  The tests use xor of nested conditions (a implies b:
                // b && !a == a ^ b) so each comparison is issued once.
                const bool valid = D >= T1;
                amb = amb || (valid != (D >= nT2));             // -T2 <= D < T1: grazing
                bool r1;
                const double n = cand_root<AMGM>(h, D, thrM, r1);
                const double tP = r1 ? thrP : thrP2, tM = r1 ? thrM : thrM2;
                const bool sure = n >= tP;
                amb = amb || (valid && (sure != (n >= tM)));    // the chosen root straddles the threshold
                const bool cand = valid && sure;
                const double nt = cand_tag(n, k + e, msk);
                const double diff = nt - bn;
                const bool closer = cand && diff < -M2;
                amb = amb || (cand && fabs(diff) <= M2);        // (closer implies |diff| > M2)
                bn = closer ? nt : bn;
            }
        }
    }
    if (MN) {
        // the winner is sure (its tagged value, within 2^-36 |n| of n, clears
        // thr + M with that margin) and every other candidate lies more than
        // 2M above it; no candidate: bn is the sentinel
        const bool any = bn < kCandNone;
        amb = amb || gmin < T1;
        amb = amb || (any && (bn < thrP * (1.0 + 0x1p-34) || !(bn2 - bn > M2)));
        bk = any ? (int)((uint32_t)__double2loint(bn) & 0xffffu) : -1;
    } else {
        bk = bn < INF ? (int)((uint32_t)__double2loint(bn) & 0xffffu) : -1;
    }
    if (COUNT)
        for (int k = 0; k < kp.ns; ++k) cnt.c[RT_CNT_SPHERE_DISC] += disc_positive(kp.sph[k], o, d, four_a) ? 1 : 0;
    double t = INF;
    int win = -1;
    if (!amb && bk >= 0) {
        const SphGeo s = kp.sph_slot[bk];    // the slot's sphere, and its index in the caller's list
        const int orig = kp.cand_orig[bk];
        bool hit;
        if constexpr (HB) hit = sphere_exact_hb(s.cx, s.cy, s.cz, s.r2, o, d, two_a, fast, rc2a, t);
        else hit = sphere_exact<CU>(s.cx, s.cy, s.cz, s.r2, o, d, two_a, four_a, fast, rc2a, t);
        if (hit) win = orig;
        else amb = true;     // cannot happen within the bound; stay exact anyway
    }
    if (amb) {               // exact reference scan for this ray
        if (COUNT) cnt.c[RT_CNT_EXACT_RESCANS] += 1;
        win = spheres_exact_scan<F>(kp, o, d, two_a, four_a, fast, rc2a, t);
    }
    t_best = t;
    return win;
}

}  // namespace rt
