// rt_vec.h -- Vectors, normalize, the kernarg window, Mat, the LDS sums and the COUNT counters.
// Part of the single translation unit rt_kernels.hip (included there, in this order).
#pragma once

namespace rt {

struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 v3(double a, double b, double c) { return V3{a, b, c}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 mulv(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 muls(V3 a, double t) { return v3(a.x * t, a.y * t, a.z * t); }
__device__ __forceinline__ V3 divs(V3 a, double t) { return v3(a.x / t, a.y / t, a.z / t); }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

__device__ __forceinline__ V3 cross(V3 u, V3 v)
{
    return v3(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
}

// normalize(a) = a / sqrt(dot(a, a)), vec3.h:137-139, bit-exact: fast lanes
// need dot(a,a) in [2^-760, 2^760] and every |component| >= 2^-900 (so zero
// components, NaN and extreme lengths take the generic path).
// min(|a|, |b|, |c|) as two v_min_f64 with abs source modifiers: fmin would
// first canonicalize each operand (one v_max_f64 x, x per component) under
// IEEE mode.  Only compared against a positive bound; a NaN component makes
// dot(a, a) NaN, which fails normalize's range test whatever this returns.
__device__ __forceinline__ double dmin_abs3(double a, double b, double c)
{
    double r;
    asm("v_min_f64 %0, |%1|, |%2|\n\tv_min_f64 %0, %0, |%3|" : "=&v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// max(|a|, |b|, |c|) (a NaN operand drops out: callers test the values it
// bounds for NaN themselves)
__device__ __forceinline__ double dmax_abs3(double a, double b, double c)
{
    double r;
    asm("v_max_f64 %0, |%1|, |%2|\n\tv_max_f64 %0, %0, |%3|" : "=&v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__device__ __forceinline__ V3 normalize(V3 a)
{
    const double n2 = dot(a, a);
    const double mn = dmin_abs3(a.x, a.y, a.z);
    if (n2 >= 0x1p-760 && n2 <= 0x1p760 && mn >= 0x1p-900) {
        double L, rc;                    // 1/L from the sqrt sequence's own rsq (rt_device_math.h)
        sqrt_rcp_core(n2, L, rc);
        return v3(div_core(a.x, L, rc), div_core(a.y, L, rc), div_core(a.z, L, rc));
    }
    return divs(a, sqrt(n2));
}

// normalize() of random_dir_no_norm's vector (rtutility.h:198-202): the
// components are float products, each nonzero (cos/sin of a float are never 0)
// or a signed zero (theta = 0: sin = +0), and |a|^2 is within 6 * 2^-24 of 1,
// so no range guard: sqrt_rcp_near1 and div_core0 on every lane.
__device__ __forceinline__ V3 normalize_unit(V3 a)
{
    double L, rc;
    sqrt_rcp_near1(dot(a, a), L, rc);
    return v3(div_core0(a.x, L, rc), div_core0(a.y, L, rc), div_core0(a.z, L, rc));
}

// The kernel's by-value parameters (kernarg segment) through an address the
// compiler cannot see through: fields read via it are loaded (s_load) where
// they are used instead of being held in SGPRs -- and spilled to VGPR lanes,
// one v_readlane per reload -- across a long loop.
// (KParams is the only argument of the kernels that use this: offset 0.)
typedef const __attribute__((address_space(4))) KParams* KParamsK;
__device__ __forceinline__ KParamsK kp_here()
{
    KParamsK p = (KParamsK)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}


// (int) of a double as the reference's x86-64 build executes it (cvttsd2si):
// NaN and out-of-range values give INT_MIN, the "integer indefinite".  C
// leaves this undefined; gfx950's v_cvt_i32_f64 saturates instead (NaN -> 0),
// so NaN radiance (e.g. AO_intensity truncated to 0, main.c:43/115) would
// otherwise resolve differently.
__device__ __forceinline__ int cvt_i32_x86(double x)
{
    return (x > -2147483649.0 && x < 2147483648.0) ? (int)x : (int)0x80000000u;
}

struct Mat {
    V3 diff, emis;
    double es, rs, alpha, ior;
};
__device__ __forceinline__ Mat load_mat(const DevMat* m)
{
    const DevMat r = *m;
    return Mat{v3(r.dr, r.dg, r.db), v3(r.er, r.eg, r.eb), r.es, r.rs, r.alpha, r.ior};
}

// Per-pixel sums (radiance, albedo, normal) live in LDS, one 9-double column
// per thread ([9][256], conflict-free), so they occupy no VGPRs across the
// bounce loop.  Only the owning thread touches its column: plain
// read-add-write, same IEEE adds in the same order as fill_canva's sums.
__device__ __forceinline__ void acc_add(double* acc, int base, V3 v)
{
    acc[(base + 0) * 256] = acc[(base + 0) * 256] + v.x;
    acc[(base + 1) * 256] = acc[(base + 1) * 256] + v.y;
    acc[(base + 2) * 256] = acc[(base + 2) * 256] + v.z;
}

enum : int { ACC_RAD = 0, ACC_ALB = 3, ACC_NRM = 6, ACC_SLOTS = 9 };

// Per-thread event counters (COUNT instantiation only).
struct Cnt {
    unsigned long long c[RT_NCOUNTERS];
};

// COUNT diagnostics: one lane per wave-level execution adds 64 lane slots.
__device__ __forceinline__ void wave_slots(Cnt& cnt, int k)
{
    if ((int)(threadIdx.x & 63) == __ffsll((unsigned long long)__ballot(1)) - 1) cnt.c[k] += 64;
}

enum : int { HIT_NONE = 0, HIT_SPHERE = 1, HIT_TRI = 2 };

__device__ __forceinline__ double dinf() { return __longlong_as_double(0x7ff0000000000000ll); }

}  // namespace rt
