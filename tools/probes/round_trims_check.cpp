// Host checks of rt_shared_math.h, the arithmetic the paired-draw kernels run
// (tests/test_exact_scaling.py builds and runs this; link with liboracle.so,
// -ffp-contract=off):
//
//   halfb N SEED    sphere_halfb against oracle_hit_sphere (sphere.h:13-47 as
//                   rt_oracle.c states it) on N random rays and spheres and on
//                   edge cases: origin on the surface, grazing rays, lerped
//                   directions with a far from 1, coordinates scaled by 2^+-20,
//                   and magnitudes that leave the windows.  sqrt_in and div_in
//                   are IEEE sqrt and division here (the kernel's cores are
//                   those operations inside the windows).  A case must give
//                   the oracle's didHit and dst bit for bit, or go to Mth::reference
//                   (counted as not fast).
//   philox N SEED   philox_head + the block started from it against the full
//                   philox4x32_10 of this header and against oracle_philox.
// Each prints one line of counts; "bad 0" is a pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rt_shared_math.h"
#include "../../oracle/rt_oracle.h"
using namespace rt;

struct V {
    double x, y, z;
};
static bool g_reference;              // the last sphere_halfb left its case to the reference form
struct Ieee {
    static double sqrt_in(double x) { return std::sqrt(x); }
    static double div_in(double x, double d, double) { return x / d; }
    template <class V>
    static bool reference(double, double, double, double, const V&, const V&, double, double&)
    {
        g_reference = true;
        return false;
    }
};

static uint64_t g_s;
static uint64_t rnd()                  // splitmix64
{
    uint64_t u = (g_s += 0x9E3779B97F4A7C15ull);
    u = (u ^ (u >> 30)) * 0xBF58476D1CE4E5B9ull;
    u = (u ^ (u >> 27)) * 0x94D049BB133111EBull;
    return u ^ (u >> 31);
}
static double uni(double lo, double hi) { return lo + (hi - lo) * ((double)(rnd() >> 11) * 0x1p-53); }
static V unit()
{
    for (;;) {
        const V v{uni(-1, 1), uni(-1, 1), uni(-1, 1)};
        const double n = std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
        if (n > 0.1 && n <= 1.0) return V{v.x / n, v.y / n, v.z / n};
    }
}
static uint64_t bits(double d)
{
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}

static long g_n, g_fast, g_notfast, g_hits, g_bad;

static void one(V c, double radius, V o, V d)
{
    const double a = d.x * d.x + d.y * d.y + d.z * d.z;       // dot(r.dir, r.dir)
    const rt_point3 C{{c.x, c.y, c.z}};
    const rt_ray R{{{o.x, o.y, o.z}}, {{d.x, d.y, d.z}}};
    const oracle_hit h = oracle_hit_sphere(C, radius, R);
    ++g_n;
    double t = -1.0;
    g_reference = false;
    const bool hit = sphere_halfb<Ieee>(c.x, c.y, c.z, radius * radius, o, d, a, halfb_fast_a(a), 0.0, t);
    if (g_reference) {
        ++g_notfast;
        return;
    }
    ++g_fast;
    g_hits += hit;
    const bool same = hit == (h.didHit != 0) && (!hit || bits(t) == bits(h.dst));
    if (!same && g_bad++ < 8)
        std::printf("halfb: c %a %a %a r %a o %a %a %a d %a %a %a: got %d %a, oracle %d %a\n", c.x, c.y, c.z, radius, o.x,
                    o.y, o.z, d.x, d.y, d.z, (int)hit, t, h.didHit, h.dst);
}

static int halfb(long n)
{
    for (long i = 0; i < n; ++i) {
        const V c{uni(-4, 4), uni(-4, 4), uni(-6, 1)};
        const double radius = i % 7 == 0 ? uni(100, 1000) : uni(0.05, 2.0);
        const V nrm = unit();
        V o{uni(-2, 2), uni(-2, 2), uni(-5, 1)}, d = unit();
        const int kind = (int)(i % 8);
        if (kind >= 1 && kind <= 3) {              // origin on the surface, as a bounce leaves it
            o = V{c.x + radius * nrm.x, c.y + radius * nrm.y, c.z + radius * nrm.z};
            if (kind >= 2) {                       // ... leaving it at a grazing angle
                const V w = unit();
                const V tn{nrm.y * w.z - nrm.z * w.y, nrm.z * w.x - nrm.x * w.z, nrm.x * w.y - nrm.y * w.x};
                const double e = (i & 8 ? 1e-9 : 1e-14) * (i & 16 ? 1.0 : -1.0);
                d = V{tn.x + e * nrm.x, tn.y + e * nrm.y, tn.z + e * nrm.z};
                if (kind == 3) {                   // ... or touching it from a distance: disc within a few ulp of 0
                    const double L = uni(0.5, 4.0), e3 = (double)((long)(rnd() % 9) - 4) * 0x1p-53;
                    o = V{o.x - L * tn.x, o.y - L * tn.y, o.z - L * tn.z};
                    d = V{tn.x + e3 * nrm.x, tn.y + e3 * nrm.y, tn.z + e3 * nrm.z};
                }
            }
        } else if (kind == 4) {                    // lerped directions: a far from 1
            const double s = std::exp2(uni(-30, 30));
            d = V{d.x * s, d.y * s, d.z * s};
        }
        if (kind == 5 || kind == 6) {              // the scene scaled by 2^20 / 2^-20
            const double s = kind == 5 ? 0x1p20 : 0x1p-20;
            one(V{c.x * s, c.y * s, c.z * s}, radius * s, V{o.x * s, o.y * s, o.z * s}, d);
        } else {
            one(c, radius, o, d);
        }
    }
    const long random_fast = g_fast;
    // magnitudes at and beyond the windows: a (through |d|) around 2^-100 and 2^99,
    // the discriminant around 2^-760 and 2^758 and into overflow and underflow
    for (int e = -540; e <= 540; e += 1) {
        const double s = std::exp2((double)e);
        for (int j = 0; j < 40; ++j) {
            const V c{uni(-4, 4), uni(-4, 4), uni(-6, 1)}, o{uni(-2, 2), uni(-2, 2), uni(-5, 1)};
            const V u = unit();
            const double radius = uni(0.5, 3.0);
            one(c, radius, o, V{u.x * s, u.y * s, u.z * s});                                     // a = s^2
            one(V{c.x * s, c.y * s, c.z * s}, radius * s, V{o.x * s, o.y * s, o.z * s}, u);      // disc ~ s^2
            one(V{c.x * s, c.y * s, c.z * s}, radius * s, V{o.x * s, o.y * s, o.z * s}, V{u.x / s, u.y / s, u.z / s});
        }
    }
    const double special[] = {0.0, -0.0, HUGE_VAL, -HUGE_VAL, std::nan(""), 0x1p-1074, 0x1p1023};
    for (double x : special)
        for (int j = 0; j < 6; ++j) {
            V c{0.5, 0.25, -3.0}, o{0.1, 0.2, 0.3}, d{0.0, 0.0, -1.0};
            double* slot[] = {&c.x, &o.y, &d.z, &d.x, &o.z, &c.z};
            *slot[j] = x;
            one(c, 1.0, o, d);
        }
    std::printf("halfb n %ld fast %ld random_fast %ld notfast %ld hits %ld bad %ld\n", g_n, g_fast, random_fast, g_notfast,
                g_hits, g_bad);
    return g_bad != 0;
}

static int philox(long n)
{
    long bad = 0;
    for (long i = 0; i < n; ++i) {
        uint32_t block = (uint32_t)rnd(), pixel = (uint32_t)rnd(), sample = (uint32_t)rnd();
        const uint32_t k0 = (uint32_t)rnd(), k1 = (uint32_t)rnd();
        if (i % 16 == 1) pixel = 0u;
        if (i % 16 == 2) pixel = 0xffffffffu;
        if (i % 4 == 3) block = (uint32_t)(i % 13);            // the kernel's blocks: 0 and 1 + i / 2
        if (i % 32 == 5) sample = 0u;
        const Philox full = philox4x32_10(block, 0u, pixel, sample, k0, k1);
        const PhiloxHead h = philox_head(pixel, k0);
        const Philox got = philox4x32_10(block, h, sample, k0, k1);
        const unsigned ctr[4] = {block, 0u, pixel, sample}, key[2] = {k0, k1};
        unsigned ref[4];
        oracle_philox(ctr, key, ref);
        const bool same = got.w0 == full.w0 && got.w1 == full.w1 && got.w2 == full.w2 && got.w3 == full.w3 &&
                          full.w0 == ref[0] && full.w1 == ref[1] && full.w2 == ref[2] && full.w3 == ref[3];
        if (!same && bad++ < 8) std::printf("philox: block %u pixel %u sample %u key %u %u differs\n", block, pixel, sample, k0, k1);
    }
    std::printf("philox n %ld bad %ld\n", n, bad);
    return bad != 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    const long n = argc > 2 ? std::atol(argv[2]) : 0;
    g_s = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 1;
    if (mode == "halfb") return halfb(n);
    if (mode == "philox") return philox(n);
    std::fprintf(stderr, "usage: round_trims_check halfb|philox N SEED\n");
    return 2;
}
