// rt_fixed_grid.h -- The fixed-grid integrators (trace_cuda, LanePath) and their kernels render_kernel / render_kernel_cuda.
// Part of the single translation unit rt_kernels.hip (included there, in this order).
#pragma once

namespace rt {

// tracer, main_cuda.cu:86-141 (rt.h RT_SEM_CUDA).  A pre-pass cast returns
// emitters (HSL round trip, L and S x1.20) and misses (zeros); the bounce
// loop starts again from the same ray, so its first cast reuses the pre-pass
// hit (the COUNT build recasts it, to count what main_cuda.cu casts); no
// alpha holes, refraction, textures or x1.3 brightening; a triangle's
// material is its own (kp.tri_mat); albedo/normal are the pre-pass hit's.
template <bool COUNT, bool BVH, class SE = unsigned short>
__device__ __forceinline__ bool cuda_hit(const KParams& kp, const V3 o, const V3 d, V3& hp, V3& hn, Mat& mat,
                                         Cnt& cnt)
{
    double t;
    int idx;
    const int kind = closest_hit<cf(COUNT, CF_COUNT) | cf(BVH, CF_BVH) | CF_CUDA, SE>(kp, o, d, t, idx, cnt);
    if (kind == HIT_NONE) return false;
    hp = o + muls(d, t);                                 // ray_at
    if (kind == HIT_SPHERE) {
        const SphGeo s = kp.sph[idx];
        hn = normalize(hp - v3(s.cx, s.cy, s.cz));   // sphere.hu:31,40
        mat = load_mat(kp.sph_mat + idx);
    } else {
        hn = tri_normal(kp, idx);                        // triangle.hu:266
        mat = load_mat(kp.tri_mat + idx);
    }
    return true;
}

template <bool COUNT, bool BVH, class SE = unsigned short>
__device__ __forceinline__ void trace_cuda(const KParams& kp, V3 o, V3 d, Stream& st, double* acc, Cnt& cnt)
{
    V3 hp, hn;
    Mat mat;
    if (!cuda_hit<COUNT, BVH, SE>(kp, o, d, hp, hn, mat, cnt)) {    // return BLACK
        acc_add(acc, ACC_RAD, v3(0, 0, 0));
        acc_add(acc, ACC_ALB, v3(0, 0, 0));
        acc_add(acc, ACC_NRM, v3(0, 0, 0));
        return;
    }
    if (mat.es > 0) {
        const V3 col = hsl_roundtrip<true>(mat.emis);
        acc_add(acc, ACC_RAD, col);
        acc_add(acc, ACC_ALB, col);
        acc_add(acc, ACC_NRM, hn);
        return;
    }
    acc_add(acc, ACC_ALB, mat.diff);                     // the outer hitInfo, main_cuda.cu:140
    acc_add(acc, ACC_NRM, hn);
    V3 inc = v3(0, 0, 0), rc = v3(1, 1, 1);
    for (int i = 0; i < kp.B; i++) {
        if ((i > 0 || COUNT) && !cuda_hit<COUNT, BVH, SE>(kp, o, d, hp, hn, mat, cnt)) break;
        o = hp;
        const V3 diffuse_dir = normalize(hn + random_dir<COUNT>(st, cnt));
        const V3 reflected_dir = d - muls(hn, 2 * dot(d, hn));
        d = diffuse_dir + muls(reflected_dir - diffuse_dir, mat.rs);   // vec3_lerp, rtutility.hu:31-35
        if (kp.useAO) {
            const double AO = ((cdptr)kp.uni)[opq0() + U_AO];
            const V3 em = muls(mat.emis, mat.es * 1.5 * AO);
            inc = inc + mulv(em, rc);
            rc = mulv(mat.diff, rc);
            const double occ = ao_factor<COUNT, BVH, true, SE>(kp, hp, hn, AO, st, cnt);
            rc = mulv(rc, v3(occ, occ, occ));
        } else {
            const V3 em = muls(mat.emis, mat.es);
            inc = inc + mulv(em, rc);
            rc = mulv(mat.diff, rc);
        }
    }
    acc_add(acc, ACC_RAD, inc);
}

// write_color_canva, rtutility.h:56-71 (sqrtf of the float-rounded product)
__device__ __forceinline__ double resolve(double sum, double rapport)
{
    double r = (double)sqrtf((float)(rapport * sum));
    r = r < 0.0 ? 0.0 : (r > 0.999 ? 0.999 : r);
    return (double)cvt_i32_x86(256 * r);
}

__device__ __forceinline__ void store3(double* base, long long i, V3 v)
{
    base[3 * i + 0] = v.x;
    base[3 * i + 1] = v.y;
    base[3 * i + 2] = v.z;
}

// The frame planes of one pixel's sums over S samples (main.c:275-279); albedo,
// normal and radiance may be null.
__device__ __forceinline__ void write_planes(double* canva, double* albedo, double* normal, double* radiance,
                                             long long li, double S, V3 srad, V3 salb, V3 snrm)
{
    const double rapport = 1.0 / S;
    store3(canva, li, v3(resolve(srad.x, rapport), resolve(srad.y, rapport), resolve(srad.z, rapport)));
    if (albedo) store3(albedo, li, divs(salb, S));
    if (normal) store3(normal, li, divs(snrm, S));
    if (radiance) store3(radiance, li, divs(srad, S));
}

__device__ __forceinline__ void write_pixel(const KParams& kp, long long li, V3 srad, V3 salb, V3 snrm)
{
    write_planes(kp.canva, kp.albedo, kp.normal, kp.radiance, li, (double)kp.S, srad, salb, snrm);
}

// Primary ray of sample st (main.c:258-270; camera.h:42-55 get_ray).
// The four camera draws of a sample (draws 0-3: word n of Philox block 0)
// from registers, for a camera ray computed ahead of its path
// (render_kernel_q): the lane's LDS block cache stays with the path in flight.
struct CamDraws {
    Philox b;
    int n;
    __device__ __forceinline__ uint32_t next31()
    {
        const uint32_t w = n == 0 ? b.w0 : n == 1 ? b.w1 : n == 2 ? b.w2 : b.w3;
        ++n;
        return w >> 1;
    }
};

// The ray before its normalize: the origin no and (returned) dest - no.  st: the
// sample's draws (Stream, or CamDraws), taken in the order ju, jv, jx, jy; pin
// (kp.cam_pin: zero aperture, host-checked): the origin is the camera's own and
// the last two draws are not made.
template <bool CU, class ST>
__device__ __forceinline__ V3 camera_ray_raw(const KParams& kp, int x, int g, ST& st, bool pin, V3& no)
{
    const double ju = rand_m05(st.next31());     // randomDouble(-0.5, 0.5)
    const double jv = rand_m05(st.next31());
    const int b = opq0();
    const cdptr U = (cdptr)kp.uni;
    // main.c:265-266; main_cuda.cu:152-153 adds 0.5 first
    // (x + ju) / (W - 1): the numerators are 0 or of magnitude >= 2^-31 and
    // the divisors in [1, 2^31], inside div_core's exact range
    const double nu = CU ? (double)x + 0.5 + ju : (double)x + ju;
    const double nv = CU ? (double)g + 0.5 + jv : (double)g + jv;
    const double rcw = U[b + U_RC_WM1], rch = U[b + U_RC_HM1];
    const double u = rcw != 0.0 ? div_core(nu, U[b + U_WM1], rcw) : nu / U[b + U_WM1];
    const double v = rch != 0.0 ? div_core(nv, U[b + U_HM1], rch) : nv / U[b + U_HM1];
    // get_ray, camera.h:42-55
    const V3 co = v3(U[b + U_CAM_O], U[b + U_CAM_O + 1], U[b + U_CAM_O + 2]);
    const V3 ch = v3(U[b + U_CAM_H], U[b + U_CAM_H + 1], U[b + U_CAM_H + 2]);
    const V3 cv = v3(U[b + U_CAM_V], U[b + U_CAM_V + 1], U[b + U_CAM_V + 2]);
    const V3 cc = v3(U[b + U_CAM_C], U[b + U_CAM_C + 1], U[b + U_CAM_C + 2]);
    const V3 dir = cc + (muls(ch, u) + (muls(cv, v) - co));
    const V3 dest = co + muls(dir, U[b + U_FOCUS]);
    if (pin) {
        no = co;
    } else {
        const double jx = rand_m05(st.next31());
        const double jy = rand_m05(st.next31());
        const double dx = jx * U[b + U_OX], dy = jy * U[b + U_OY];
        no = co + v3(dx, dy, 0);
    }
    return dest - no;
}
template <bool CU, class ST>
__device__ __forceinline__ void camera_ray(const KParams& kp, int x, int g, ST& st, V3& no, V3& rd)
{
    rd = normalize(camera_ray_raw<CU>(kp, x, g, st, false, no));
}

// Resumable trace for the BVH kernel: the same tracer and
// ambient_occlusion arithmetic (main.c:94-242), as a per-lane state
// machine (LanePath).  A lane in
//   SM_RESOLVE shades the hit of its finished cast (a bounce or an AO cast),
//   SM_CAM     starts its next sample (or is done),
//   SM_CAST    runs the sphere half of the next cast and sets up traversal,
//   SM_TRAV    visits nodes of the triangle BVH,
// and a lane's casts, draws and sums happen in the same order as in tracer,
// so results are bit-identical.  samples_coop runs it (the fixed-grid BVH
// kernel: spp_chunks 1, trees too deep for the queue kernel's stacks); the
// queue kernel (render_kernel_q<.., QB>) resumes its walks round by round with
// the same states.
enum : int { SM_RESOLVE = 0, SM_CAM = 1, SM_CAST = 2, SM_TRAV = 3, SM_DONE = 4 };

// QPath's AOM: AO compiled out (0) or always on (1): the queue kernel is
// instantiated per AO setting so a sphere scene without AO carries neither the
// AO cast's state nor its code.  LanePath reads kp.useAO.
enum : int { AO_OFF = 0, AO_ON = 1 };

template <bool COUNT, bool SKY>
struct LanePath {
    Stream st;
    V3 o, d, cd;                                 // ray, next bounce direction, current cast's direction
    V3 inc, rc;
    Ray32 r32;                                   // the cast's single-precision slab set-up (BVH)
    double top_n2, best;
    int i, kind, win, win_orig, node, sp, s, state;
    bool chain, ao_cast;

    // Zero-throughput exit (kp.zero_exit, set by the host only when it is
    // exact): once rayColor is (0, 0, 0) every later bounce adds em * 0 = +-0
    // to incomingLight (x + +-0 == x: incomingLight starts at +0 and is never
    // -0), multiplies rayColor by a finite diffuse colour or AO factor (still
    // 0), and chain (albedo/normal) is already off, since rayColor only
    // changes after it is cleared.  Draws are counter-based per sample, so
    // skipping the rest of the path changes no other sample.  The host
    // requires every emission, strength and diffuse value finite with
    // |x| <= 2^100 (no em overflow), and with AO 0 < AO_intensity <= 1000
    // and every coordinate within 2^20 (the AO factor pow(distance/dst, AO)/AO
    // then stays finite: distance/dst <= 1.02).
    __device__ __forceinline__ bool zero_rc(const KParams& kp) const
    {
        return kp.zero_exit && rc.x == 0.0 && rc.y == 0.0 && rc.z == 0.0;
    }

    __device__ __forceinline__ void init(int s0, int s1)
    {
        o = d = cd = inc = rc = v3(0, 0, 0);
        r32 = Ray32{0, 0, 0, 0, 0, 0, 0, 0, 0};
        top_n2 = 1.0;
        best = 0.0;
        i = 0; kind = HIT_NONE; win = -1; win_orig = 0; node = 0; sp = 0;
        chain = true;
        ao_cast = false;
        s = s0;
        state = s0 < s1 ? SM_CAM : SM_DONE;
    }

    // tracer's bounce body after the cast (main.c:127-241), or
    // ambient_occlusion's tail (main.c:104-115) for an AO cast
    __device__ __forceinline__ void resolve(const KParams& kp, double* acc, Cnt& cnt)
    {
        if (COUNT) wave_slots(cnt, RT_CNT_SHADE_LANE_SLOTS);
        bool more = true;                    // the path goes on to bounce i + 1
        bool add_inc = true;                 // false: direct view of a light (tracer returns early)
        st.k0 = kp.key0;                     // the key from the kernel argument (uniform), not
        st.k1 = kp.key1;                     // a loop-carried copy
        const bool use_ao = kp.useAO != 0;
        if (ao_cast) {
            const double AO = ((cdptr)kp.uni)[opq0() + U_AO];
            const double occ = ao_tail(kind != HIT_NONE, o, cd, best, AO);
            rc = mulv(rc, v3(occ, occ, occ));
            ao_cast = false;
            if (zero_rc(kp)) more = false;   // an AO miss zeroes rayColor: nothing more to add
        } else if (kind == HIT_NONE) {       // miss: the path ends, main.c:236-238
            if (chain) {
                acc_add(acc, ACC_ALB, v3(0, 0, 0));
                acc_add(acc, ACC_NRM, v3(0, 0, 0));
            }
            more = false;
        } else {
            V3 hp, hn;
            Mat mat;
            if (kind == HIT_SPHERE) {
                const SphGeo sg = kp.sph[win];
                hp = o + muls(d, best);
                hn = normalize(hp - v3(sg.cx, sg.cy, sg.cz));
                mat = load_mat(kp.sph_mat + win);
                if (SKY && win == kp.ns - 1) sky_material(kp, win, sg, hp, mat);
            } else {
                if (COUNT) cnt.c[RT_CNT_TEX_HITS] += 1;
                hp = o + muls(d, best);
                hn = tri_normal(kp, win);
                mat = tri_material(kp, win, hp, hn);
            }
            bool lit = false;
            if (chain) {
                if (mat.es > 0) {
                    const V3 col = hsl_roundtrip(mat.emis);
                    acc_add(acc, ACC_RAD, col);
                    acc_add(acc, ACC_ALB, col);
                    acc_add(acc, ACC_NRM, hn);
                    lit = true;
                } else if (!(mat.alpha < 0.0001) || i == kp.B - 1) {
                    acc_add(acc, ACC_ALB, mat.diff);
                    acc_add(acc, ACC_NRM, hn);
                    chain = mat.alpha < 0.0001;
                }
            }
            if (lit) {
                more = false;
                add_inc = false;
            } else {
                o = hp;
                const V3 diffuse_dir = normalize(hn + random_dir<COUNT>(st, cnt));
                const V3 reflected_dir = d - muls(hn, 2 * dot(d, hn));
                const V3 dr = diffuse_dir + muls(reflected_dir - diffuse_dir, mat.rs);
                bool shade = !(mat.alpha < 0.0001);  // not an alpha hole (main.c:200-206)
                if (shade) {
                    chain = false;
                    if (mat.alpha <= 0.99) {
                        if (COUNT) cnt.c[RT_CNT_REFRACT] += 1;
                        const V3 refr = refracted_at(d, hn, mat.ior, top_n2);
                        const double rnd = rand_01(st.next31());
                        if (rnd > mat.alpha) {
                            d = refr;
                            shade = false;
                        } else {
                            d = dr;
                        }
                    } else {
                        d = dr;
                    }
                }
                if (shade) {
                    V3 r = rc;                   // (QPath::shade_with, rt_queue.h: the same shading)
                    if (use_ao) {
                        const double AO = ((cdptr)kp.uni)[opq0() + U_AO];
                        const V3 em = muls(mat.emis, mat.es * 1.5 * AO);
                        inc = inc + mulv(em, r);
                        if (any_above_half(r)) r = mulv(mat.diff, muls(r, 1.3));
                        rc = mulv(mat.diff, r);
                        // ambient_occlusion's cast (main.c:96-103): from hp along n + random;
                        // with rayColor black it could only scale 0: neither drawn nor cast
                        ao_cast = !zero_rc(kp);
                        if (ao_cast) cd = normalize(hn + random_dir<COUNT>(st, cnt));
                    } else {
                        const V3 em = muls(mat.emis, mat.es);
                        inc = inc + mulv(em, r);
                        if (any_above_half(r)) r = mulv(mat.diff, muls(r, 1.3));
                        rc = mulv(mat.diff, r);
                    }
                    if (zero_rc(kp)) more = false;   // black diffuse (a light, a green-then-red wall)
                }
            }
        }
        if (ao_cast) {
            state = SM_CAST;
        } else {
            if (more) {
                ++i;
                more = i < kp.B;
            }
            if (more) {
                cd = d;
                state = SM_CAST;
            } else {
                if (add_inc) acc_add(acc, ACC_RAD, inc);
                if (COUNT) {
                    cnt.c[RT_CNT_SAMPLES] += 1;
                    cnt.c[RT_CNT_RNG_DRAWS] += st.n;
                }
                ++s;
                state = SM_CAM;
            }
        }
    }

    // the next sample's primary ray (fill_canva's sample loop, main.c:258-270)
    __device__ __forceinline__ void start(const KParams& kp, int x, int g, uint32_t pixel, int s1, uint32_t* rng,
                                          double* acc, Cnt& cnt)
    {
        if (s >= s1) {
            state = SM_DONE;
        } else {
            st.start(pixel, (uint32_t)(kp.s_base + s), kp.key0, kp.key1, rng);
            camera_ray<false>(kp, x, g, st, o, d);
            cd = d;
            inc = v3(0, 0, 0);
            rc = v3(1, 1, 1);
            top_n2 = 1.0;
            i = 0;
            chain = true;
            ao_cast = false;
            if (kp.B <= 0) {                 // tracer returns (0, 0, 0) albedo/normal
                acc_add(acc, ACC_ALB, v3(0, 0, 0));
                acc_add(acc, ACC_NRM, v3(0, 0, 0));
                acc_add(acc, ACC_RAD, inc);
                if (COUNT) {
                    cnt.c[RT_CNT_SAMPLES] += 1;
                    cnt.c[RT_CNT_RNG_DRAWS] += st.n;
                }
                ++s;
            } else {
                state = SM_CAST;
            }
        }
    }

    // the whole cast in one go (spheres, then brute-force triangles)
    __device__ __forceinline__ void cast_flat(const KParams& kp, Cnt& cnt)
    {
        kind = closest_hit<cf(COUNT, CF_COUNT)>(kp, o, cd, best, win, cnt);
        state = SM_RESOLVE;
    }

    // closest_hit's sphere half and the traversal set-up
    __device__ __forceinline__ void cast(const KParams& kp, Cnt& cnt)
    {
        win = cast_spheres<cf(COUNT, CF_COUNT)>(kp, o, cd, best, cnt);
        kind = win >= 0 ? HIT_SPHERE : HIT_NONE;
        win_orig = 0;
        if (kp.bvh) r32 = ray32(kp, o, cd);
        node = 0;
        sp = 0;
        state = SM_TRAV;
    }

    // one node visit; RESOLVE when the traversal is over
    template <class SE>
    __device__ __forceinline__ void trav(const KParams& kp, SE* stk, Cnt& cnt)
    {
        if (!bvh_step<COUNT, false>(kp, o, cd, r32, stk, node, sp, best, kind, win, win_orig, cnt)) state = SM_RESOLVE;
    }
};


// The fixed-grid sphere kernel's sample loop as LanePath rounds: each
// round every lane with a path casts and shades one bounce; a lane whose path
// ended (a miss, a light seen directly, the bounce budget, or zero
// throughput) waits for its next sample's camera ray, which starts once
// RT_FLAT_FILL eighths of the wave's live lanes wait (the camera ray then
// costs the wave one pass for many lanes).  Same casts, draws and sums per
// sample as tracer, so bit-identical; it lets the zero-throughput exit
// save the cast instead of idling the lane until the wave's longest path.
template <bool COUNT, bool SKY>
__device__ __forceinline__ void samples_flat(const KParams& kp, int x, int g, uint32_t pixel, int s0, int s1,
                                             uint32_t* rng, double* acc, Cnt& cnt)
{
    LanePath<COUNT, SKY> L;
    L.init(s0, s1);
    while (L.state != SM_DONE) {
        const unsigned long long live = __ballot(1), wait = __ballot(L.state == SM_CAM);
        const bool go = wait == live || __popcll(wait) * 8 >= __popcll(live) * RT_FLAT_FILL;
        if (go && L.state == SM_CAM) L.start(kp, x, g, pixel, s1, rng, acc, cnt);
        if (L.state == SM_CAST) {
            L.cast_flat(kp, cnt);
            L.resolve(kp, acc, cnt);
        }
    }
}

// Wave-cooperative traversal of the deep casts (fixed-grid BVH kernel).  About 5 %
// of C4's casts go below the tree's root; walked by their own lanes they
// keep a wave at a few active lanes for ~25 node visits and ~12 triangle
// tests (leaf loop 2.6 % lane efficiency).  Here a lane runs its cast's root
// node itself; a deeper cast parks (SM_TRAV) and once RT_BVH_COOP lanes of
// the wave are parked (or nothing else can move) every live lane of the wave
// works on their subtrees: a task is (ray, node); a lane walks its task
// depth-first with its own LDS stack and hands siblings to a per-wave LIFO
// (so idle lanes pick them up) while that holds fewer than 64 entries.  The
// ray is read from its owner lane (ds_bpermute); triangle hits are merged
// into the owner's record in a wave-uniform loop with the same rule as
// tri_test (strictly closer, or an equal-dst triangle with a smaller caller
// index; a sphere keeps an equal-dst hit).  That rule is a total order, so
// the winner is the one tracer finds, whatever order the triangles are
// tested in; culling against an older `best` only tests more boxes.
__device__ __forceinline__ double rl_d(double v, int l)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double shfl_d(double v, int src)
{
    const long long b = __double_as_longlong(v);
    const int lo = __shfl((int)b, src, 64), hi = __shfl((int)(b >> 32), src, 64);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// Append each lane's n (0..4) items to the wave's LIFO (cnt: wave-uniform).
__device__ __forceinline__ void lifo_push(volatile unsigned* q, int& cnt, int n, const unsigned* it)
{
    unsigned long long b[4];
    int base = cnt, tot = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = __ballot(n > j);
    int off = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        off += __popcll(b[j] & lanes_below());
        tot += __popcll(b[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < n) q[base + off + j] = it[j];
    cnt = base + tot;
    __builtin_amdgcn_wave_barrier();
}

template <bool COUNT, bool SKY, class SE = unsigned short>
__device__ __forceinline__ void samples_coop(const KParams& kp, int x, int g, uint32_t pixel, int s0, int s1,
                                             uint32_t* rng, double* acc, Cnt& cnt)
{
    constexpr int QW = 256;                      // < 64 entries + 3 pushes x 64 lanes
    __shared__ unsigned lifo_lds[4][QW];
    volatile unsigned* q = lifo_lds[threadIdx.x >> 6];
    SE* stk = bvh_stack_of<SE>();
    const int lane = threadIdx.x & 63;
    LanePath<COUNT, SKY> L;
    L.init(s0, s1);
    while (L.state != SM_DONE) {
        if (L.state == SM_RESOLVE) L.resolve(kp, acc, cnt);
        if (L.state == SM_CAM) L.start(kp, x, g, pixel, s1, rng, acc, cnt);
        if (L.state == SM_CAST) {
            L.cast(kp, cnt);
            L.trav(kp, stk, cnt);                // the root node; SM_TRAV: parked
        }
        const unsigned long long parked = __ballot(L.state == SM_TRAV);
        const unsigned long long movable = __ballot(L.state == SM_RESOLVE || L.state == SM_CAM);
        if (parked == 0ull || (__popcll(parked) < RT_BVH_COOP && movable != 0ull)) continue;

        // ---- cooperative phase (wave-uniform) ----
        int qn = 0;
        {
            unsigned it[4];
            int n = 0;
            if (L.state == SM_TRAV) {            // next node + the root's pushes (sp <= 3)
                it[0] = (unsigned)lane | ((unsigned)L.node << 6);
                for (int j = 0; j < L.sp; ++j) it[1 + j] = (unsigned)lane | ((unsigned)stk_get(stk, j) << 6);
                n = 1 + L.sp;
            }
            lifo_push(q, qn, n, it);
        }
        bool has = false;
        int tr = 0, tnode = 0, tsp = 0;
        V3 to = v3(0, 0, 0), td = to;
        Ray32 tr32 = Ray32{0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (;;) {
            const unsigned long long idle = __ballot(!has);
            const int take = min(__popcll(idle), qn);
            bool fresh = false;
            if (!has) {
                const int rank = __popcll(idle & lanes_below());
                if (rank < take) {
                    const unsigned item = q[qn - 1 - rank];
                    tr = (int)(item & 63u);
                    tnode = (int)(item >> 6);
                    tsp = 0;
                    has = true;
                    fresh = true;
                }
            }
            qn -= take;
            __builtin_amdgcn_wave_barrier();
            if (__ballot(has) == 0ull) break;
            // the owner's ray for new tasks, its current record for every task
            // (all live lanes run the permutes; owners are live)
            if (__ballot(fresh) != 0ull) {
                const V3 ro = v3(shfl_d(L.o.x, tr), shfl_d(L.o.y, tr), shfl_d(L.o.z, tr));
                const V3 rd = v3(shfl_d(L.cd.x, tr), shfl_d(L.cd.y, tr), shfl_d(L.cd.z, tr));
                if (fresh) {
                    to = ro;
                    td = rd;
                    tr32 = ray32(kp, ro, rd);
                }
            }
            double best = shfl_d(L.best, tr);
            int kind = __shfl(L.kind, tr, 64), win = __shfl(L.win, tr, 64), win_orig = __shfl(L.win_orig, tr, 64);
            bool hit = false;
            unsigned push[3];
            int npush = 0;
            const bool to_lifo = qn < 64;
            if (has) {
                // one node visit (bvh_visit, rt_triangles.h): the other hit internal
                // children go to push[] (for the LIFO) when to_lifo, else on the
                // lane's own stack.  hit: a triangle beat the record (replacements
                // are strictly ordered, so it changed iff one did)
                const int w0 = win, k0 = kind;
                if (!bvh_visit<COUNT, false, 0, 0, false>(kp, to, td, tr32, stk, tnode, tsp, best, kind, win, win_orig,
                                                          cnt, nullptr,
                                                          [&](int pu, float tpu) __attribute__((always_inline)) {
                                                              if (to_lifo) push[npush++] = (unsigned)pu;
                                                              else bvh_push<COUNT, false>(kp, stk, tsp, pu, tpu, cnt);
                                                          }))
                    has = false;
                hit = win != w0 || kind != k0;
#pragma unroll
                for (int j = 0; j < 3; ++j) push[j] = (unsigned)tr | (push[j] << 6);
            }
            lifo_push(q, qn, npush, push);
            // merge the lanes' better triangles into their owners' records
            unsigned long long m = __ballot(hit);
            while (m != 0ull) {
                const int l = __ffsll(m) - 1;
                m &= m - 1ull;
                const int r = __builtin_amdgcn_readlane(tr, l);
                const double db = rl_d(best, l);
                const int dw = __builtin_amdgcn_readlane(win, l), dorig = __builtin_amdgcn_readlane(win_orig, l);
                if (lane == r && (db < L.best || (db == L.best && L.kind == HIT_TRI && dorig < L.win_orig))) {
                    L.best = db;
                    L.kind = HIT_TRI;
                    L.win = dw;
                    L.win_orig = dorig;
                }
            }
        }
        if (L.state == SM_TRAV) L.state = SM_RESOLVE;
    }
}

// n / d and n % d for 32-bit n by a launch-constant d with m = kp's
// floor((2^32 - 1) / d) (host, qdiv_magic): the high product is q or q - 1,
// one remainder check fixes it (5 integer ops instead of a division).
__device__ __forceinline__ unsigned udiv_q(unsigned n, unsigned d, unsigned m, unsigned& r)
{
    unsigned q = __umulhi(n, m);
    const unsigned rr = n - q * d;
    const bool up = rr >= d;
    r = up ? rr - d : rr;
    return up ? q + 1u : q;
}

// Global frame row of row yy of the launch's local tile lt (cyclic row tiles:
// local tile lt is tile tile_first + lt * tile_step of the rows from row_base).
// A row at or beyond k.row_end is a padding row of the last, partial tile: no work.
// K: KParams, by value reference or through the queue kernel's KParamsK.
template <class K>
__device__ __forceinline__ int tile_row(const K& k, int lt, int yy)
{
    return k.row_base + (k.tile_first + lt * k.tile_step) * k.tile_rows + yy;
}

// First sample of chunk c, rt.h rt_chunk_bound: w(c)*S/den with w(c) = c
// (den = P) or the tapered weights (den = (P - L) 2^L + 2^L - 1); 32-bit magic
// division when (den + 1) * S < 2^32 (qm_chunks != 0), else 64-bit.
__device__ __forceinline__ int chunk_start(int S, int chunks, int taper, unsigned den, unsigned qm_chunks, unsigned c)
{
    unsigned w = c;
    if (taper) {                     // L = taper levels: weights 2^L x E, then 2^(L-1) .. 1
        const unsigned E = (unsigned)chunks - (unsigned)taper, one = 1u << taper;
        w = c <= E ? c << taper : (E << taper) + one - (one >> (c - E));
    }
    if (qm_chunks != 0u) {
        unsigned r;
        return (int)udiv_q(w * (unsigned)S, den, qm_chunks, r);
    }
    return (int)(((long long)w * S) / den);
}

// Body of render_kernel (main.c semantics) and render_kernel_cuda
// (main_cuda.cu's): one thread = (pixel, chunk of its samples).
// SE: the BVH stack's element type (uint32_t: a wide tree, rt_bvh.h)
template <bool COUNT, bool BVH, bool SKY, bool CU, class SE = unsigned short>
__device__ __forceinline__ void render_body(const KParams& kp)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int ly = kp.band_y0 + blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    const int chunk = blockIdx.z;
    Cnt cnt;
    if (COUNT)
        for (int k = 0; k < RT_NCOUNTERS; ++k) cnt.c[k] = 0;
    bool valid = x < kp.W && ly < kp.local_rows && ly < kp.band_y0 + kp.band_rows;
    int g = 0;
    if (valid) {
        const int lt = ly / kp.tile_rows, yy = ly - lt * kp.tile_rows;
        g = tile_row(kp, lt, yy);
        valid = g < kp.row_end;
    }
    if (valid) {
        const uint32_t pixel = (uint32_t)g * (uint32_t)kp.W + (uint32_t)x;
        const int s0 = chunk_start(kp.S, kp.chunks, kp.chunk_taper, kp.chunk_den, 0u, (unsigned)chunk);
        const int s1 = chunk_start(kp.S, kp.chunks, kp.chunk_taper, kp.chunk_den, 0u, (unsigned)chunk + 1u);
        __shared__ double acc_lds[ACC_SLOTS * 256];
        __shared__ uint32_t rng_lds[4 * 256];
        double* acc = acc_lds + threadIdx.x;
        const long long li = (long long)ly * kp.W + x;
        // accumulate mode with one chunk continues the running sums in sample
        // order (fill_canva's fold, carried across launches); otherwise 0
        const bool carry = !COUNT && kp.sums && kp.chunks == 1;
#pragma unroll
        for (int j = 0; j < 9; ++j) acc[j * 256] = carry ? kp.sums[li * 9 + j] : 0.0;
        if constexpr (BVH && !CU) {
            samples_coop<COUNT, SKY, SE>(kp, x, g, pixel, s0, s1, rng_lds + threadIdx.x, acc, cnt);
        } else if constexpr (!BVH && !CU) {
            samples_flat<COUNT, SKY>(kp, x, g, pixel, s0, s1, rng_lds + threadIdx.x, acc, cnt);
        } else {                             // CU: main_cuda.cu's nested sample loop (main_cuda.cu:150-165)
            for (int s = s0; s < s1; ++s) {
                Stream st;
                st.start(pixel, (uint32_t)(kp.s_base + s), kp.key0, kp.key1, rng_lds + threadIdx.x);
                V3 no, rd;
                camera_ray<CU>(kp, x, g, st, no, rd);
                trace_cuda<COUNT, BVH, SE>(kp, no, rd, st, acc, cnt);
                if (COUNT) {
                    cnt.c[RT_CNT_SAMPLES] += 1;
                    cnt.c[RT_CNT_RNG_DRAWS] += st.n;
                }
            }
        }
        if (!COUNT) {
            const V3 srad = v3(acc[0], acc[256], acc[512]);
            const V3 salb = v3(acc[768], acc[1024], acc[1280]);
            const V3 snrm = v3(acc[1536], acc[1792], acc[2048]);
            if (carry) {
#pragma unroll
                for (int j = 0; j < 9; ++j) kp.sums[li * 9 + j] = acc[j * 256];
            } else if (kp.chunks == 1) {
                write_pixel(kp, li, srad, salb, snrm);
            } else {
                double* p = kp.partial + ((long long)chunk * kp.band_rows * kp.W +
                                          ((long long)(ly - kp.band_y0) * kp.W + x)) * 9;
                p[0] = srad.x; p[1] = srad.y; p[2] = srad.z;
                p[3] = salb.x; p[4] = salb.y; p[5] = salb.z;
                p[6] = snrm.x; p[7] = snrm.y; p[8] = snrm.z;
            }
        }
    }
    if (COUNT) {
        for (int k = 0; k < RT_NCOUNTERS; ++k) {
            unsigned long long v = cnt.c[k];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if (lane == 0 && v) atomicAdd(kp.counters + k, v);
        }
    }
}

// fill_canva, main.c:245-284: thread = (pixel, chunk of its samples).
template <bool COUNT, bool BVH, bool SKY>
__global__ __launch_bounds__(256, BVH ? RT_WAVES_PER_SIMD_BVH : RT_WAVES_PER_SIMD) void render_kernel(const KParams kp)
{
    render_body<COUNT, BVH, SKY, false>(kp);
}

// render_canva, main_cuda.cu:143-171 semantics (rt.h RT_SEM_CUDA).
template <bool COUNT, bool BVH>
__global__ __launch_bounds__(256, BVH ? RT_WAVES_PER_SIMD_BVH : RT_WAVES_PER_SIMD) void render_kernel_cuda(
    const KParams kp)
{
    render_body<COUNT, BVH, false, true>(kp);
}

// The same two kernels for a wide tree (rt_bvh.h BvhBuild::wide: node or
// triangle indices beyond 16 bits): the walk of the 128-byte nodes, whose
// children are ints, with uint32 stack entries (bvh_stack32: 48 KiB, two
// blocks per CU).  The universal path of wide trees: spp_chunks 1,
// rt_accumulate_async, rt_count_async, RT_SEM_CUDA, trees whose 64-byte form
// does not pack or whose stack bound exceeds the queue kernel's.
template <bool COUNT, bool SKY>
__global__ __launch_bounds__(256, 2) void render_kernel_w(const KParams kp)
{
    render_body<COUNT, true, SKY, false, uint32_t>(kp);
}
template <bool COUNT>
__global__ __launch_bounds__(256, 2) void render_kernel_cuda_w(const KParams kp)
{
    render_body<COUNT, true, false, true, uint32_t>(kp);
}

}  // namespace rt
