// rt_shared_math.h -- arithmetic that the kernels run and a CPU check can
// compile as it stands (tools/probes/round_trims_check.cpp, tests/test_exact_scaling.py):
// the Philox4x32-10 block and its per-task head, and the winner's sphere test
// in half-b units.  Plain C++ but for xor3_s's one gfx950 instruction; no HIP
// header.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RT_HD __host__ __device__ inline __attribute__((always_inline))
#define RT_UNROLL _Pragma("unroll")
#else
#define RT_HD inline
#define RT_UNROLL
#endif

namespace rt {

// ---- Philox4x32-10 (Random123 / rocrand_philox4x32_10 engine) -------------
struct Philox {
    uint32_t w0, w1, w2, w3;
};

// a ^ b ^ k in one VALU op: gfx950's v_bitop3_b32 with truth table 0x96
// (three-input xor; k a wave-uniform SGPR)
RT_HD uint32_t xor3_s(uint32_t a, uint32_t b, uint32_t k)
{
#if defined(__gfx950__)
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "s"(k));
    return r;
#else
    return a ^ b ^ k;                  // other targets: the compiler's own xor chain
#endif
}

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

template <bool UNIFORM_KEY = true>
RT_HD Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#if defined(__gfx950__)
    if (UNIFORM_KEY) asm volatile("" : "+s"(k0), "+s"(k1));   // key schedule in place (SALU), not hoisted
#endif
    RT_UNROLL
    for (int r = 0; r < 10; ++r) {
        // one v_mad_u64_u32 yields both halves of each 32x32 product; the
        // round's two xors with the key are one v_bitop3_b32 each
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        uint32_t n0, n2;
        if (UNIFORM_KEY) {
            n0 = xor3_s((uint32_t)(p1 >> 32), c1, k0);
            n2 = xor3_s((uint32_t)(p0 >> 32), c3, k1);
        } else {
            n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
            n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        }
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
    return Philox{c0, c1, c2, c3};
}

// The head of a block with counter {c0, 0, pixel, c3}: what pixel and the key
// alone decide, so it is the same for every block of a pixel's task.  Round 1
// multiplies M1 by pixel: its low half is round 2's c1, its high half gives
// n0 = hi ^ 0 ^ k0, round 2's c0, which round 2 multiplies by M0: the high half
// goes into round 2's n2 and the low half is round 3's c3.  n0 and the high
// half of M1 * pixel are read by nothing else.
struct PhiloxHead {
    uint32_t c1;             // lo(M1 * pixel)
    uint32_t hi, lo;         // the halves of M0 * n0
};
RT_HD PhiloxHead philox_head(uint32_t pixel, uint32_t k0)
{
    const uint64_t p1 = (uint64_t)kPhiloxM1 * pixel;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ k0;
    const uint64_t p0 = (uint64_t)kPhiloxM0 * n0;
    return PhiloxHead{(uint32_t)p1, (uint32_t)(p0 >> 32), (uint32_t)p0};
}
// philox4x32_10(c0, 0, pixel, c3, k0, k1) from h = philox_head(pixel, k0):
// rounds 1 and 2 without the products h holds (one v_mad_u64_u32 each instead
// of two, and round 1 without its first xor), rounds 3 to 10 as above.
RT_HD Philox philox4x32_10(uint32_t c0, const PhiloxHead& h, uint32_t c3, uint32_t k0, uint32_t k1)
{
#if defined(__gfx950__)
    asm volatile("" : "+s"(k0), "+s"(k1));
#endif
    const uint64_t q0 = (uint64_t)kPhiloxM0 * c0;                             // round 1: c0 = n0 is in h
    uint32_t c2 = xor3_s((uint32_t)(q0 >> 32), c3, k1);
    k0 += kPhiloxW0; k1 += kPhiloxW1;
    const uint64_t q1 = (uint64_t)kPhiloxM1 * c2;                             // round 2
    c0 = xor3_s((uint32_t)(q1 >> 32), h.c1, k0);
    c2 = xor3_s(h.hi, (uint32_t)q0, k1);
    uint32_t c1 = (uint32_t)q1;
    c3 = h.lo;
    k0 += kPhiloxW0; k1 += kPhiloxW1;
    RT_UNROLL
    for (int r = 2; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = xor3_s((uint32_t)(p1 >> 32), c1, k0), n2 = xor3_s((uint32_t)(p0 >> 32), c3, k1);
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
    return Philox{c0, c1, c2, c3};
}

// ---- hit_sphere (sphere.h:13-47) in half-b units ---------------------------
// The reference computes b = 2 s (s = oc.d), disc = b b - (4a) c, sq =
// sqrt(disc), n = -b -+ sq, t = n / (2a).  Scaling by 2 and 4 is exact, so
// without overflow or underflow its values are
//   disc = 4 dh,  dh = fl(fl(s s) - fl(a c));   sq = 2 fl(sqrt(dh));
//   n = 2 nh,  nh = fl(-s -+ sqrt(dh));         t = fl(nh / a)
// and the sign tests and the 1e-4 threshold compare the same values.  This
// form leaves out 2 s, 2 a and 4 a.  It answers only inside windows that
// imply the guards of the reference form's fast path (rt_spheres.h
// sphere_exact: 2a in [2^-100, 2^100], disc in [2^-760, 2^760]) and that rule
// overflow and underflow out; every other lane runs the reference form.
//   a in [2^-100, 2^99]: 2a is in [2^-99, 2^100].
//   dh in [2^-760, 2^758]: disc = 4 dh is in [2^-758, 2^760].  With p = fl(s s)
//   and q = fl(a c), dh = fl(p - q) <= 2^758 bounds p and |q| by 2^812 (a
//   non-zero difference of two doubles is at least an ulp of the larger, 2^759
//   from 2^812 on), so 4p, 4q and s itself (|s| < 2^407) do not overflow; and
//   dh >= 2^-760 leaves one of p, |q| at 2^-761 or more, the other, if it
//   underflowed (below 2^-1022, where fl(4x) and 4 fl(x) may differ), below a
//   quarter ulp of it in either form, so both differences round to the larger.
//   A sum of doubles is exact when it is subnormal: nh scales exactly.
//   !(dh > 0) with q in [2^-1000, 2^1000] is the reference's miss: q and 4q are
//   exact scalings, and p <= q (or p NaN, and then disc is NaN) either scales
//   exactly too or, underflowed, stays below 2^-1019 <= q / 2 in both forms.
// Mth::sqrt_in and Mth::div_in: sqrt and x / a, exact for dh in the window and
// for every x = nh that can decide or become t -- a hit needs nh >= 1e-4 a >=
// 2^-114, and |nh| <= |s| + sqrt(dh) < 2^408; smaller nh give t < 1e-4 with
// any quotient near nh / a <= 2^-799 (rt_device_math.h div_core's range, and
// its argument in sphere_exact with a for 2a).  Mth::reference: the reference
// form for the lanes outside the windows, in the one block they alone enter.
RT_HD bool halfb_fast_a(double a) { return a >= 0x1p-100 && a <= 0x1p99; }
template <class Mth, class V>
RT_HD bool sphere_halfb(double cx, double cy, double cz, double r2, const V& o, const V& d, double a, bool fast,
                        double rca, double& t)
{
    const double ocx = o.x - cx, ocy = o.y - cy, ocz = o.z - cz;
    const double s = ocx * d.x + ocy * d.y + ocz * d.z;
    const double c = (ocx * ocx + ocy * ocy + ocz * ocz) - r2;
    const double q = a * c;
    const double dh = s * s - q;
    if (!(fast && dh >= 0x1p-760 && dh <= 0x1p758)) {
        if (fast && !(dh > 0) && q >= 0x1p-1000 && q <= 0x1p1000) return false;
        return Mth::reference(cx, cy, cz, r2, o, d, a, t);
    }
    const double sq = Mth::sqrt_in(dh);
    const double n1 = -s - sq;
    if (!(n1 < 0.0)) {
        t = Mth::div_in(n1, a, rca);
        if (t >= 0.0001) return true;
    }
    const double n2 = -s + sq;
    if (!(n2 < 0.0)) {
        t = Mth::div_in(n2, a, rca);
        if (t >= 0.0001) return true;
    }
    return false;
}

}  // namespace rt
