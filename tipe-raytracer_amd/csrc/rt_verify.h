// rt_verify.h -- The rt_verify_* kernels and their launchers: device code paths against their exact forms.
// Part of the single translation unit rt_kernels.hip (included there, in this order).
#pragma once

namespace rt {

// Every sampler input r in [r0, r0 + n): phi_sincosf_fast against the full
// path pm_sincosf((float)pm_acos(2 r/2^31 - 1)).  counts[0] += inputs that
// fall back, counts[1] += inputs whose fast result differs (must stay 0).
__global__ __launch_bounds__(256) void verify_phi_kernel(unsigned long long r0, unsigned long long n,
                                                        unsigned long long* counts)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    bool fb = false, bad = false;
    if (i < n) {
        const double xv = 2 * unit31((uint32_t)(r0 + i)) - 1;
        float sp, cp, s2, c2;
        const bool ok = phi_sincosf_fast(xv, sp, cp);
        pm_sincosf((float)pm_acos(xv), s2, c2);
        fb = !ok;
        bad = ok && (__float_as_uint(sp) != __float_as_uint(s2) || __float_as_uint(cp) != __float_as_uint(c2));
    }
    const unsigned long long nf = __popcll(__ballot(fb)), nb = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0) {
        if (nf) atomicAdd(counts, nf);
        if (nb) atomicAdd(counts + 1, nb);
    }
}

// Sphere closest hit of arbitrary rays (o, d: 6 doubles each): the candidate
// pass (spheres_closest, with its own exact fallback) against the plain exact
// scan.  counts[0] += rays the candidate pass sent to the exact scan,
// counts[1] += rays whose winner or t differs (must stay 0).
__global__ __launch_bounds__(256) void verify_spheres_kernel(const KParams kp, const double* __restrict__ rays,
                                                            long long n, unsigned long long* counts)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool fb = false, bad = false;
    if (i < n) {
        const V3 o = v3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]);
        const V3 d = v3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
        const double a = dot(d, d), two_a = 2 * a, four_a = 4 * a;
        const bool fast = two_a >= 0x1p-100 && two_a <= 0x1p100;
        const double rc2a = rcp_refined(two_a);
        Cnt cnt;
        cnt.c[RT_CNT_EXACT_RESCANS] = 0;
        double t1, t2;
        const int w1 = spheres_closest<CF_COUNT | CF_PAIRS>(kp, o, d, a, two_a, four_a, fast, rc2a, t1, cnt);
        const int w2 = spheres_exact_scan<CF_NONE>(kp, o, d, two_a, four_a, fast, rc2a, t2);
        fb = cnt.c[RT_CNT_EXACT_RESCANS] != 0;
        bad = w1 != w2 || (w1 >= 0 && __double_as_longlong(t1) != __double_as_longlong(t2));
    }
    const unsigned long long nf = __popcll(__ballot(fb)), nb = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0) {
        if (nf) atomicAdd(counts, nf);
        if (nb) atomicAdd(counts + 1, nb);
    }
}

// normalize() (fast lanes: sqrt_rcp_core / rcp_refined + div_core) and its
// seeded forms against IEEE a / sqrt(a.a) on n pseudo-random vectors (Philox,
// key = seed), by q.w2 & 7:
//   0-3  normalize(): unit-scale vectors, n + dir sums, one common scale 2^e
//        (e in [-400, 400)), a scale per component
//   4-5  normalize_unit() on the sampler's vectors (sampler_vec of two 31-bit
//        draws, as random_dir makes them)
//   6-7  normalize() on hit-point offsets hp - C: C with components
//        scaled by 2^[-8, 12), |r| = 2^[-10, 10) times [1, 2), hp = C + r u for a
//        random unit u (rounded, as a hit point is), seeded as the host does
// counts[0] += vectors on a fast path, counts[1] += results that differ.
__device__ __forceinline__ double vn_comp(uint32_t hi, uint32_t lo)
{
    const unsigned long long m = ((unsigned long long)hi << 21) ^ (unsigned long long)(lo >> 11);
    const double u = (double)(m & ((1ull << 53) - 1)) * 0x1p-53;             // [0, 1)
    return (hi & 0x80000000u) ? -u : u;
}
__global__ __launch_bounds__(256) void verify_normalize_kernel(unsigned long long seed, unsigned long long i0,
                                                               unsigned long long n, unsigned long long* counts)
{
    const unsigned long long i = i0 + (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    bool fp = false, bad = false;
    if (i < i0 + n) {
        const Philox p = philox4x32_10<false>((uint32_t)i, (uint32_t)(i >> 32), 0x6e6f726du, 0u, (uint32_t)seed,
                                              (uint32_t)(seed >> 32));
        const Philox q = philox4x32_10<false>((uint32_t)i, (uint32_t)(i >> 32), 0x6e6f726du, 1u, (uint32_t)seed,
                                              (uint32_t)(seed >> 32));
        V3 a = v3(vn_comp(p.w0, p.w1), vn_comp(p.w2, p.w3), vn_comp(q.w0, q.w1));
        const uint32_t cls = q.w2 & 7u;
        V3 got;
        if (cls >= 4u) {                            // the sampler's unit vectors
            a = sampler_vec(p.w0 >> 1, p.w1 >> 1);
            fp = true;
            got = normalize_unit(a);
        } else {
            if (cls == 1u) {                               // n + dir: unit normal plus a unit vector
                const V3 nn = divs(a, sqrt(dot(a, a)));
                a = nn + v3(vn_comp(q.w3, p.w0), vn_comp(p.w1 ^ q.w3, p.w2), vn_comp(p.w3, q.w0 ^ p.w1));
            } else if (cls == 2u) {                        // one scale for the vector
                const int e = (int)(q.w3 % 800u) - 400;
                a = v3(ldexp(a.x, e), ldexp(a.y, e), ldexp(a.z, e));
            } else if (cls == 3u) {                        // a scale per component
                a = v3(ldexp(a.x, (int)(q.w3 % 900u) - 450), ldexp(a.y, (int)((q.w3 >> 10) % 900u) - 450),
                       ldexp(a.z, (int)((q.w3 >> 20) % 900u) - 450));
            }
            const double n2 = dot(a, a);
            const double mn = fmin(fmin(fabs(a.x), fabs(a.y)), fabs(a.z));
            fp = n2 >= 0x1p-760 && n2 <= 0x1p760 && mn >= 0x1p-900;
            got = normalize(a);
        }
        const V3 want = divs(a, sqrt(dot(a, a)));
        bad = __double_as_longlong(got.x) != __double_as_longlong(want.x) ||
              __double_as_longlong(got.y) != __double_as_longlong(want.y) ||
              __double_as_longlong(got.z) != __double_as_longlong(want.z);
        bad = bad && !(got.x != got.x && want.x != want.x);   // NaN == NaN
    }
    const unsigned long long nf = __popcll(__ballot(fp)), nb = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0) {
        if (nf) atomicAdd(counts, nf);
        if (nb) atomicAdd(counts + 1, nb);
    }
}

int launch_verify_normalize(unsigned long long seed, unsigned long long n, unsigned long long* d_counts)
{
    const unsigned long long per = 1ull << 30;          // launches of at most 2^30 vectors
    for (unsigned long long i0 = 0; i0 < n; i0 += per) {
        const unsigned long long m = std::min(per, n - i0);
        hipLaunchKernelGGL(verify_normalize_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, seed,
                           i0, m, d_counts);
    }
    return hipGetLastError();
}

// rt_verify_texel_map: point i (3 doubles) on triangle tri[i] through the
// affine texel map and through the exact path; counts[0] += certain,
// counts[1] += certain but a different texel
__global__ __launch_bounds__(256) void verify_texel_kernel(const KParams kp, const double* __restrict__ pts,
                                                           const int* __restrict__ tri, long long n,
                                                           unsigned long long* counts)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool fast = false, bad = false;
    if (i < n) {
        const int k = tri[i];
        const V3 P = v3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
        const TexRef e = tri_texel_exact(kp, k, P, tri_normal(kp, k));
        TexRef f{0, 0};
        fast = tri_texel_affine(kp, k, P, f);
        bad = fast && (f.index != e.index || f.m != e.m);
    }
    const unsigned long long nf = __popcll(__ballot(fast)), nb = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0) {
        if (nf) atomicAdd(counts, nf);
        if (nb) atomicAdd(counts + 1, nb);
    }
}

int launch_verify_texel(const KParams& kp, const double* d_pts, const int* d_tri, long long n,
                        unsigned long long* d_counts)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(verify_texel_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, kp, d_pts,
                       d_tri, n, d_counts);
    return hipGetLastError();
}

int launch_verify_spheres(const KParams& kp, const double* d_rays, long long n, unsigned long long* d_counts)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(verify_spheres_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, kp, d_rays,
                       n, d_counts);
    return hipGetLastError();
}

int launch_verify_phi(unsigned long long r0, unsigned long long n, unsigned long long* d_counts)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(verify_phi_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, r0, n, d_counts);
    return hipGetLastError();
}

int launch_selftest(int op, const double* d_in, double* d_out, int n, void* stream)
{
    hipLaunchKernelGGL(selftest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, op,
                       d_in, d_out, n);
    return (int)hipGetLastError();
}

}  // namespace rt
