// rt_queue.h -- The task-queue integrator QPath and its kernel render_kernel_q.
// Included, behind the headers of its helpers (rt_vec.h ... rt_fixed_grid.h, in
// that order), by the two files that instantiate the kernel: rt_kernels.hip (the
// dense form) and rt_queue_list.hip (the list form).
#pragma once
#include <type_traits>

namespace rt {

// Persistent kernel over (chunk, pixel) tasks (spp_chunks > 1, main.c
// semantics).  A task is one pixel's samples [c*S/P, (c+1)*S/P) in order, summed in the lane's LDS column and written to
// the chunk partials, which combine_kernel sums in chunk order: the result is
// the fixed-grid kernel's bit for bit whichever lane runs the task.  Paths
// run as LanePath rounds (samples_flat); a lane whose task is done starts its
// next one, so lanes with short paths (misses, lights, zero throughput) do
// not idle until the wave's longest slice ends.
// Tasks come from a per-launch counter, kQueueBatch tasks per atomic: a wave
// takes a batch and hands its tasks to its lanes as they need them.  Static
// task lists were 1.3x slower: the dispatcher places waves unevenly over the
// SIMDs (per-lane clocks: waves with the same work ended between 21 and
// 45 ms), so only a dynamic queue keeps every SIMD busy to the end; one
// atomic per lane grab was 1.8x slower (same-address atomics).  The grid is
// the resident capacity; every lane leaves once the counter passes the
// task count.

// One lane's path in render_kernel_q: tracer's state (main.c:118-242) for
// the sample in flight.  Rounds run in three steps so that a lane whose path
// ends starts its next sample's camera ray in the SAME instructions that
// continuing lanes use for their bounce direction (one Philox block and one
// normalize serve both):
//   resolve_hit   everything of tracer's bounce body that does not need the
//                 next direction: hit point, material, albedo/normal chain,
//                 the light seen directly, alpha holes, and -- when the
//                 surface is opaque -- the shading, the zero-throughput exit
//                 and the bounce budget; it leaves the lane a role
//   next_ray      BOUNCE: random_dir_no_norm and normalize(n + dir)
//                 CAMERA: the 4 camera draws and get_ray, normalize
//                 (both: draws from one Philox block, one normalize)
//   finish_bounce reflect/lerp, the refraction branch (whose draw follows
//                 the direction draws), AO set-up
// The draws keep the reference's per-sample order (counter-based stream:
// direction n, n+1, refraction n+2, AO next), so results are bit-identical
// to tracer; work whose result cannot reach the output is skipped: the
// direction after the last bounce, and the AO cast of the last bounce
// (tracer multiplies rayColor by it and then returns incomingLight).
enum : int { ROLE_NONE = 0, ROLE_BOUNCE = 1, ROLE_CAMERA = 2, ROLE_AO = 3, ROLE_PBOUNCE = 4 };
// AO scenes (AOM == AO_ON), an opaque bounce whose draws start a Philox block
// (draw n = 4k: the camera takes draws 0-3 and a shaded bounce with its AO
// ray 4 more, so every such bounce in scenes without translucent surfaces or
// alpha holes): the lane makes ONE direction per round.  ROLE_AO makes the AO
// direction from draws n+2, n+3 right after the shading (ambient_occlusion,
// main.c:96-103), keeping draws n, n+1 of the same block in the LDS cache;
// after the AO cast, ROLE_PBOUNCE makes the bounce direction from them
// (main.c:161-166) and the lerp.  The draws, and so the results, are the
// reference's; each round's shared next-ray step then serves every lane that
// needs a direction, instead of a second sampling pass for the AO ray in
// finish_bounce, and the bounce direction is skipped when the AO factor
// ends the path.

// What resolve_hit leaves for next_ray / finish_bounce in the same round (not
// live across rounds, so not in QPath: the cast and the BVH walk do not carry
// these registers).
struct QHit {
    V3 hn;                           // the hit's normal
    double rs;                       // its reflectionStrength
    bool refr, hole;                 // refraction decided after the direction draws; alpha hole
    TexRef tex;                      // (triangle hits) the texel resolve_hit read: the refraction branch
                                     // re-reads the material from it instead of redoing the barycentrics
};

// One render_kernel_q instantiation: its row T of rt_queue_variants.h's table
// (what the (QB, OPQ) pair means, shared with the host) and, derived from it
// once, what only the device build knows (the RT_* tunables of rt_kernels.hip,
// AO_ON).  QPath and render_kernel_q read these; nothing else compares QB.
template <bool SKY_, int AOM_, int QB_, bool OPQ_>   // OPQ: (BVH scenes) every material opaque
struct QVariant {
    static_assert(queue_variant_index(QB_, OPQ_) >= 0, "not a pair of kQueueVariants (e.g. the wide-tree kernel has no "
                                                       "opaque specialisation)");
    static constexpr QueueVariant T = queue_variant(QB_, OPQ_);
    static constexpr bool SKY = SKY_, OPQ = OPQ_;
    static constexpr int AOM = AOM_, QB = QB_;
    // NT: the scene has no triangles (every hit is a sphere); OP: every material
    // is opaque (host: !(alpha < 0.0001) && !(alpha <= 0.99), so no alpha hole
    // and no refraction branch is ever taken and neither is compiled in)
    static constexpr bool NT = !T.triangles, OP = T.opaque;
    static constexpr bool BVH = T.nodes != QN_NONE;      // spheres, then a bounded BVH walk per round
    static constexpr bool DEEP = T.nodes == QN_H || T.nodes == QN_W;   // the deep-tree walk (64-byte nodes in HBM)
    // Occupancy bound (rt_kernels.hip RT_WAVES_PER_SIMD_*): the sphere-only, the
    // shallow-tree and the wide-tree kernels have their own (the last: 46 KiB of
    // LDS, three blocks per CU)
    static constexpr int WAVES = NT                  ? RT_WAVES_PER_SIMD_QS
                                 : T.nodes == QN_128 ? RT_WAVES_PER_SIMD_Q4
                                 : T.nodes == QN_W   ? RT_WAVES_PER_SIMD_QW
                                                     : RT_WAVES_PER_SIMD_Q;
    // IR: incomingLight / rayColor live in the lane's LDS column (slots
    // ACC_SLOTS..+5 of the sums array) instead of twelve VGPRs: both (2) for the
    // non-BVH kernels, incomingLight alone (1) for the opaque deep-tree kernel
    // (its stack leaves room for 3 doubles)
    static constexpr int IR = !BVH ? 2 : OP ? 1 : 0;
    // KT: a refraction lane keeps its triangle hit's texel (QHit::tex) from
    // resolve_hit to finish_bounce instead of redoing the barycentrics (the
    // brute-force kernel, QB_SCAN: C3 +7.0 %, C5 +6.7 %; the BVH kernels recompute,
    // their registers are tighter: sweep -1.9 % with KT)
    static constexpr bool KT = T.triangles && !BVH;
    // PD: paired draws (render_kernel_q's step 4).  Every material opaque and no
    // AO, so a sample's draws are fixed -- the camera takes draws 0-3 (Philox
    // block 0) and bounce i draws 4 + 2i and 5 + 2i: a bounce with even i opens
    // block 1 + i/2, uses its words 0, 1 and keeps words 2, 3 (kw2, kw3) for
    // bounce i + 1.  Step 4 then needs neither the draw count st.n nor the block
    // cache in LDS; resolve_hit moves o to the hit point of every hit (a lit
    // lane's path is over, its o is dead) and skips the miss's identity adds.  The
    // sphere-only kernels take this form; the opaque deep-tree kernel (QB_DEEP,
    // OPQ) has no registers to spare and keeps the general one.
    static constexpr bool PD = NT && OP && AOM != AO_ON;
    static_assert(!PD || (OP && AOM != AO_ON), "paired draws: two draws per bounce, none else");
    // TTAB: each wave decodes its batches of tasks into LDS -- every
    // instantiation but the deep-tree ones, where the table's registers cost spills
    static constexpr bool TTAB = !DEEP;
    // shallow trees (QB_TOP: depth4 <= 4, e.g. the 50-node sweep tree) keep
    // their top nodes in LDS, as 128-byte nodes; deep trees walk the 64-byte
    // nodes in HBM (HN, bvh_step's node form; host: kp.bvhh / kp.bvhw set)
    static constexpr int HN = BVH ? T.nodes : 0;
    static constexpr int NTOP = T.nodes == QN_128 ? RT_QB_TOP : 0;
    // Node visits per round.  Deep trees: at least RT_QW_MIN visits, then more
    // while at least RT_QW_LANES lanes of the wave are still walking, up to
    // RT_QW_MAX (long walks -- e.g. rays skimming RTX_MAP/nature's terrain --
    // finish in fewer rounds, short ones hand the wave back to the path work as
    // before); QB_TOP: its own value
    static constexpr int JMIN = DEEP ? RT_QW_MIN : BVH ? QB : 0, JMAX = DEEP ? RT_QW_MAX : BVH ? QB : 0;
    static constexpr bool FAR = T.far;                   // ray32's far-origin margins
    // The cast (rt_spheres.h CF_*).  Before a BVH walk: the plain candidate loop.
    // Else the pair loops (closest_hit adds them itself), in the kernels without
    // AO or sky with the AMGM bound; the paired-draw kernels test in half-b units.
    static constexpr unsigned CAST = BVH ? CF_NONE
                                         : cf(!SKY && AOM != AO_ON, CF_AMGM) | cf(NT, CF_PAIRS) | cf(PD, CF_HALFB);
    static constexpr int PHASE_CAST = BVH ? 1 : 0;       // RT_PHASE_CLOCK: the slot that ends at step 2 (the walk's,
                                                         // else the cast's)
};

template <class V>
struct QPath {
    static constexpr bool SKY = V::SKY, NT = V::NT, OP = V::OP, KT = V::KT, PD = V::PD;
    static constexpr int AOM = V::AOM, IR = V::IR;       // IR 1: incomingLight only
    V3 o, d, cd, inc, rc;            // cd: the cast's direction (AO casts; else d)
    double* accp;                    // (IR) the lane's LDS column
    double top_n2, best;
    int i, kind, win, s, state;
    bool chain, ao_cast;
    bool pend;                       // (AO_ON) the bounce direction waits for the AO cast (ROLE_PBOUNCE)
    int pkw;                         // ... the bounce hit: win | kind << 30 (its normal is recomputed at o)
    double prs;                      // ... and its reflectionStrength

    // no path, no task (acc: the lane's LDS column)
    __device__ __forceinline__ void init(double* acc)
    {
        accp = acc;
        o = d = cd = inc = rc = v3(0, 0, 0);
        inc_set(v3(0, 0, 0));
        rc_set(v3(0, 0, 0));
        top_n2 = 1.0;
        best = 0.0;
        i = 0; kind = HIT_NONE; win = -1; s = 0;
        chain = true; ao_cast = false;
        pend = false;
        pkw = 0;
        prs = 0.0;
        state = SM_CAM;              // s = 0 >= s1 = 0: takes a task first
    }

    __device__ __forceinline__ V3 cast_dir() const { return AOM == AO_ON ? cd : d; }
    __device__ __forceinline__ V3 inc_get() const
    {
        if (IR) return v3(accp[(ACC_SLOTS + 0) * 256], accp[(ACC_SLOTS + 1) * 256], accp[(ACC_SLOTS + 2) * 256]);
        return inc;
    }
    __device__ __forceinline__ V3 rc_get() const
    {
        if (IR == 2) return v3(accp[(ACC_SLOTS + 3) * 256], accp[(ACC_SLOTS + 4) * 256], accp[(ACC_SLOTS + 5) * 256]);
        return rc;
    }
    __device__ __forceinline__ void inc_set(V3 v)
    {
        if (IR) {
            accp[(ACC_SLOTS + 0) * 256] = v.x;
            accp[(ACC_SLOTS + 1) * 256] = v.y;
            accp[(ACC_SLOTS + 2) * 256] = v.z;
        } else {
            inc = v;
        }
    }
    __device__ __forceinline__ void rc_set(V3 v)
    {
        if (IR == 2) {
            accp[(ACC_SLOTS + 3) * 256] = v.x;
            accp[(ACC_SLOTS + 4) * 256] = v.y;
            accp[(ACC_SLOTS + 5) * 256] = v.z;
        } else {
            rc = v;
        }
    }

    // The hit's material (sky_material / texel_material are pure functions of
    // the hit, so a refraction lane re-reads it instead of keeping it live;
    // for a triangle it keeps only the texel, H.tex).  keep: where resolve_hit's
    // read stores that texel (KT); null: finish_bounce's re-read, from H.tex.
    __device__ __forceinline__ Mat hit_material(const KParams& kp, V3 hp, const QHit& H, TexRef* keep) const
    {
        if (NT || kind == HIT_SPHERE) {
            Mat mat = load_mat(kp.sph_mat + win);
            if (SKY && win == kp.ns - 1) sky_material(kp, win, kp.sph[win], hp, mat);
            return mat;
        }
        if (!KT) return tri_material(kp, win, hp, H.hn);
        if (keep) *keep = tri_texel(kp, win, hp, H.hn);
        return texel_material(kp, keep ? *keep : H.tex);
    }

    __device__ __forceinline__ static bool zero_rc_of(const KParams& kp, V3 r)
    {
        return kp.zero_exit && r.x == 0.0 && r.y == 0.0 && r.z == 0.0;
    }
    __device__ __forceinline__ bool zero_rc(const KParams& kp) const { return zero_rc_of(kp, rc_get()); }

    // After a cast (state SM_RESOLVE).  Returns the role for next_ray, or
    // ROLE_NONE; a lane whose path is over gets state SM_CAM (sum added).
    // the normal of a hit at point p: sphere (hit_sphere's normalize(p - C),
    // sphere.h:33) or triangle (tri_normal)
    __device__ __forceinline__ static V3 hit_normal(const KParams& kp, V3 p, int k, int w)
    {
        if (NT || k == HIT_SPHERE) {
            const SphGeo sg = kp.sph[w];
            return normalize(p - v3(sg.cx, sg.cy, sg.cz));
        }
        return tri_normal(kp, w);
    }

    __device__ __forceinline__ int resolve_hit(const KParams& kp, double* acc, QHit& H, uint32_t sn)
    {
        // AO kernels: one normal computation per round for hit lanes and pending
        // bounces (without AO there is no second normal)
        constexpr bool MN = AOM == AO_ON;
        bool ended = false, add_inc = true, hit = false, nrm = false;
        V3 np = v3(0, 0, 0);
        int nk = HIT_NONE, nw = 0;
        int role = ROLE_NONE;
        // a hit's material, chain sums, emitter / hole / refraction / shading and
        // the next role (main.c:137-234), H.hn set
        auto hit_rest = [&](const V3 hp) __attribute__((always_inline)) {
            const Mat mat = hit_material(kp, hp, H, &H.tex);
            bool lit = false;
            if (chain) {
                if (mat.es > 0) {                        // direct view of a light, main.c:154-160
                    V3 col;
                    if ((NT || kind == HIT_SPHERE) && !(SKY && win == kp.ns - 1)) {
                        const double* sd = kp_here()->sph_disp + 3 * win;   // (host: the same round trip)
                        col = v3(sd[0], sd[1], sd[2]);
                    } else {
                        col = hsl_roundtrip(mat.emis);
                    }
                    acc_add(acc, ACC_RAD, col);
                    acc_add(acc, ACC_ALB, col);
                    acc_add(acc, ACC_NRM, H.hn);
                    lit = true;
                } else if (OP || !(mat.alpha < 0.0001) || i == kp.B - 1) {
                    acc_add(acc, ACC_ALB, mat.diff);
                    acc_add(acc, ACC_NRM, H.hn);
                    chain = !OP && mat.alpha < 0.0001;
                }
            }
            if (lit) {
                ended = true;
                add_inc = false;
            } else {
                o = hp;
                H.rs = mat.rs;
                H.refr = false;
                H.hole = !OP && mat.alpha < 0.0001;
                if (H.hole) {                              // alpha H.hole: straight on, main.c:200-206;
                    if (i + 1 >= kp.B) ended = true;     // its direction draws are made (and unused)
                    else role = ROLE_BOUNCE;             // so the stream's block cache stays in order
                } else {
                    chain = false;
                    if (!OP && mat.alpha <= 0.99) {      // refraction: decided after the direction draws
                        H.refr = true;
                        role = ROLE_BOUNCE;
                    } else {
                        const V3 nrc = shade(kp, mat);
                        if (zero_rc_of(kp, nrc) || i + 1 >= kp.B) {
                            ended = true;                // nothing more reaches the sum
                        } else if (AOM == AO_ON && (sn & 3u) == 0u) {
                            role = ROLE_AO;              // AO direction first (ROLE_AO above)
                            pend = true;
                            pkw = win | (kind << 30);
                            prs = mat.rs;
                        } else {
                            role = ROLE_BOUNCE;
                        }
                    }
                }
            }
        };
        if (AOM == AO_ON && ao_cast) {
            const double AO = ((cdptr)kp.uni)[opq0() + U_AO];
            const double occ = ao_tail(kind != HIT_NONE, o, cast_dir(), best, AO);
            const V3 r2 = mulv(rc_get(), v3(occ, occ, occ));
            rc_set(r2);
            ao_cast = false;
            ++i;                                         // the bounce after the AO cast
            ended = zero_rc_of(kp, r2) || i >= kp.B;
            if (!ended) {
                if (pend) {                              // its direction is still to be made
                    role = ROLE_PBOUNCE;
                    np = o;                              // the bounce hit's normal (o is its hit point):
                    nw = pkw & 0x3fffffff;               // below, with the hit lanes' normals
                    nk = pkw >> 30;
                    nrm = true;
                    H.rs = prs;
                    H.refr = H.hole = false;
                } else {
                    cd = d;
                    state = SM_CAST;
                }
            }
            pend = false;
        } else if (kind == HIT_NONE) {                   // miss: the path ends, main.c:236-238
            // PD: tracer's two adds of (0, 0, 0) are identities and are not made.
            // A task's sums start at +0.0 and x + y (round to nearest) is -0
            // only when x and y both are, so by induction no sum is ever -0;
            // s + (+0) is s bit for bit for every other s (NaN, infinity too).
            if (!PD && chain) {
                acc_add(acc, ACC_ALB, v3(0, 0, 0));
                acc_add(acc, ACC_NRM, v3(0, 0, 0));
            }
            ended = true;
        } else {
            if (MN) {                                    // the rest after the merged normal below
                hit = true;
                np = o + muls(d, best);                  // ray_at
                nw = win;
                nk = kind;
                nrm = true;
            } else if (PD) {                             // the hit point straight into o (hit_rest's
                o = o + muls(d, best);                   // o = hp for the lanes that go on): no copy
                H.hn = hit_normal(kp, o, kind, win);     // of o at the merge with the missing lanes
                hit_rest(o);
            } else {
                const V3 hp = o + muls(d, best);         // ray_at
                H.hn = hit_normal(kp, hp, kind, win);
                hit_rest(hp);
            }
        }
        // MN: the normal of the hit each lane goes on from -- this cast's,
        // or the bounce hit waiting for the AO cast -- in ONE normalize for the
        // wave instead of one per branch
        if (MN && nrm) H.hn = hit_normal(kp, np, nk, nw);
        if (MN && hit) hit_rest(np);
        if (ended) {
            if (add_inc) acc_add(acc, ACC_RAD, inc_get());
            ++s;
            state = SM_CAM;
            role = ROLE_NONE;
        }
        return role;
    }

    // shading of an opaque surface (main.c:208-234 without the AO cast)
    __device__ __forceinline__ V3 shade_with(const KParams& kp, V3 emis, double es, V3 diff)
    {
        // (LanePath::resolve, rt_fixed_grid.h, has the same arithmetic in its two AO branches)
        V3 r = rc_get();
        if (AOM == AO_ON) es = es * 1.5 * ((cdptr)kp.uni)[opq0() + U_AO];
        const V3 em = muls(emis, es);
        inc_set(inc_get() + mulv(em, r));
        if (any_above_half(r)) r = mulv(diff, muls(r, 1.3));
        const V3 nrc = mulv(diff, r);
        rc_set(nrc);
        return nrc;
    }
    __device__ __forceinline__ V3 shade(const KParams& kp, const Mat& mat) { return shade_with(kp, mat.emis, mat.es, mat.diff); }

    // After next_ray gave a bounce lane its diffuse direction dn.
    __device__ __forceinline__ void finish_bounce(const KParams& kp, V3 dn, Stream& st, double* acc, const QHit& H)
    {
        if (!OP && H.hole) {                               // the ray goes on unchanged from the hit point
            ++i;
            cd = d;
            state = SM_CAST;
            return;
        }
        const V3 reflected_dir = d - muls(H.hn, 2 * dot(d, H.hn));
        const V3 dr = dn + muls(reflected_dir - dn, H.rs);
        bool shaded = true;
        if (!OP && H.refr) {                               // main.c:167-193
            const Mat mat = hit_material(kp, o, H, nullptr);
            const V3 rf = refracted_at(d, H.hn, mat.ior, top_n2);
            // the draw is in the block cache whatever its slot (next_ray's rpre)
            const double rnd = rand_01(st.next31_cached());
            if (rnd > mat.alpha) {
                d = rf;
                shaded = false;
            } else {
                d = dr;
                shade(kp, mat);
            }
        } else {
            d = dr;
        }
        bool ended = false;
        if (!OP && H.refr && shaded) ended = zero_rc(kp);
        if (AOM == AO_ON && shaded && !ended && i + 1 < kp.B) {
            // ambient_occlusion's cast (main.c:96-103): from the hit along n + random
            Cnt cnt;
            cd = normalize(H.hn + random_dir<false>(st, cnt));
            ao_cast = true;
            state = SM_CAST;
            return;
        }
        ++i;
        ended = ended || i >= kp.B;
        if (ended) {                                     // (refraction lanes only) the sample is over
            acc_add(acc, ACC_RAD, inc_get());
            ++s;
            state = SM_CAM;
        } else {
            cd = d;
            state = SM_CAST;
        }
    }
};

// Task t of a queue launch as render_kernel_q's LDS table entry: e[0] its
// chunk-partial index chunk * band_rows * W + p (~0: past the last task),
// e[1] the pixel g * W + x (~0: a padding row of the tiling, no work), e[2]
// the row g, e[3], e[4] its first and end sample (rt.h rt_chunk_bound).
constexpr int kTaskWords = 5;
// Tasks per atomic grab of a wave: one per lane, one batch of the LDS task table.
constexpr int kQueueBatch = 64;
__device__ __forceinline__ void decode_task(KParamsK K, unsigned t, uint32_t e[kTaskWords])
{
    for (int j = 0; j < kTaskWords; ++j) e[j] = 0xffffffffu;
    if (t >= K->npx_here * (unsigned)K->chunks) return;
    unsigned p;
    const unsigned chunk = udiv_q(t, K->npx_here, K->qm_npx, p);
    e[0] = chunk * ((unsigned)K->band_rows * (unsigned)K->W) + p;
    unsigned xr;
    const unsigned row = udiv_q(p, (unsigned)K->W, K->qm_w, xr);
    const int ly = K->band_y0 + (int)row;
    if (ly >= K->local_rows) return;
    unsigned yy;
    const int lt = (int)udiv_q((unsigned)ly, (unsigned)K->tile_rows, K->qm_tile, yy);
    const int g = tile_row(*K, lt, (int)yy);
    if (g >= K->row_end) return;
    e[1] = (uint32_t)g * (uint32_t)K->W + xr;
    e[2] = (uint32_t)g;
    e[3] = (uint32_t)chunk_start(K->S, K->chunks, K->chunk_taper, K->chunk_den, K->qm_chunks, chunk);
    e[4] = (uint32_t)chunk_start(K->S, K->chunks, K->chunk_taper, K->chunk_den, K->qm_chunks, chunk + 1u);
}

// The list form's second by-value argument, behind KParams in the kernarg segment,
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

// A list band's task words: written by the prologue (rt_queue_list.hip
// list_tasks_kernel) before the render kernel starts and by nothing afterwards,
// so they are read as constants (scalar loads).
enum : int { LT_TASKS = 0, LT_ENTRIES = 1, LT_MAGIC = 2 };
static_assert(LT_MAGIC + 1 == kListTaskWords, "the prologue's words");

// decode_task for the tasks of a list band: e[0] the partial index
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

// The (QB, OPQ) pairs are rt_queue_variants.h's, the constants QVariant's (V).
// QB_WIDE: a wide tree (rt_bvh.h BvhBuild::wide) -- the non-opaque deep-tree
// kernel (QB_DEEP, not OPQ: every material branch, the adaptive visit count, the
// far-origin margins, the walk priority) over the BvhNodeW nodes kp.bvhw with
// the 24-bit stack bvh_stack_qw; its 46 KiB of LDS allow three blocks per CU,
// RT_WAVES_PER_SIMD_QW waves per SIMD.
// TAIL: the kernel's arguments behind KParams, and with them its form.  None: the
// dense form, whose tasks are a band's (chunk, pixel) pairs (decode_task).
// ListArgs: the list form over a compacted list of pixels (rt_queue_list.hip),
// whose tasks decode_list_task reads through la_here(); kp.partial is then the
// band's partials.  Step 3's two decoder calls are all that depends on the pack.
// The round loop stays in this one __global__ function: moved into a __device__
// function that two kernels call, it is allocated other registers in 12 to 28 of
// the dense instantiations (tools/isa_same.py pins their machine code).
template <bool SKY, int AOM, int QB, bool OPQ = false, class... TAIL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(QVariant<SKY, AOM, QB, OPQ>::WAVES)))
void render_kernel_q(const KParams kp, const TAIL...)
{
    constexpr bool LIST = sizeof...(TAIL) == 1 && (std::is_same_v<TAIL, ListArgs> && ...);
    static_assert(LIST || sizeof...(TAIL) == 0, "the tail is empty (dense) or ListArgs (list)");
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
    // (PD) A block's counter is {block, 0, pixel, sample} and the pixel is the
    // task's: the lane keeps the head of its task's blocks (rt_shared_math.h
    // philox_head), made when it takes the task, in three LDS words of its own
    // (the block cache's column is unused here), and step 4 starts each block
    // from them.  A lane without a task draws nothing and reads none of them.
    __shared__ uint32_t head_lds[PD ? 3 * 256 : 1];
    uint32_t* head = head_lds + (PD ? threadIdx.x : 0);
#if RT_DIAG_STALE == 2
    diag_cnt()[0] = 0u;
    diag_cnt()[256] = 0u;
#endif
#if RT_DIAG_MERGE
    diag_merge()[DM_FLAGGED_ONE] = 0u;
    diag_merge()[DM_FLAGGED_TWO] = 0u;
    diag_merge()[DM_FORWARD_ONE] = 0u;
    diag_merge()[DM_FORWARD_TWO] = 0u;
#endif
    int x = 0, g = 0, s1 = 0;
    int node = 0, sp = 0, win_orig = 0;      // BVH walk in flight (state SM_TRAV)
    unsigned pixel = 0, qidx = 0;    // the lane's task: its pixel and its chunk-partial index (decode_task e[1], e[0])
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
    const long long t_start = kp.trace ? wall_clock64() : 0;
    unsigned rounds = 0, ntasks = 0;
#if RT_PHASE_CLOCK
    // wave-uniform clock reads at the round's uniform points (SGPR sums)
    unsigned long long ph[5] = {0, 0, 0, 0, 0}, tc = __builtin_amdgcn_s_memtime();
    auto phase = [&](int k) __attribute__((always_inline)) {
        const unsigned long long t = __builtin_amdgcn_s_memtime();
        ph[k] += t - tc;
        tc = t;
    };
#define RT_PHASE(k) phase(k)
#else
#define RT_PHASE(k) ((void)0)
#endif
    while (true) {
        ++rounds;
        RT_PHASE(4);                 // the previous round's next-ray step and finish_bounce
        // ---- 1. closest hit (main.c:52-92) for every lane with a ray ------
        if constexpr (V::BVH) {
            // spheres, then the triangle BVH: up to V::JMAX node visits
            // per round; a deeper walk resumes next round (its lane skips
            // the path work meanwhile), so a wave never waits for its
            // deepest lane's whole walk
            if (L.state == SM_CAST) {
                Cnt cnt;
                L.win = cast_spheres<V::CAST>(kp, L.o, L.cast_dir(), L.best, cnt);
                L.kind = L.win >= 0 ? HIT_SPHERE : HIT_NONE;
                win_orig = 0;
                node = 0;
                sp = 0;
                L.state = SM_TRAV;
            }
            RT_PHASE(0);
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
        RT_PHASE(V::PHASE_CAST);
        // ---- 2. the hit, up to the next direction --------------------------
        int role = ROLE_NONE;
        QHit H;
        if (PD) {
            // No defaults: H.hn and H.rs are read by bounce lanes alone (step 4's
            // else branch and finish_bounce), and resolve_hit sets both on every
            // lane it gives ROLE_BOUNCE.  The empty asm defines the four values
            // here, where the zeros were written, without an instruction: left
            // undefined instead, their registers are allocated elsewhere and the
            // kernel needs 107 VGPRs (profiles/round_trims/README.md).
            asm volatile("" : "=v"(H.hn.x), "=v"(H.hn.y), "=v"(H.hn.z), "=v"(H.rs));
        } else {
            H.hn = v3(0, 0, 0);
            H.rs = 0.0;
        }
        H.refr = H.hole = false;
        if (L.state == SM_RESOLVE) role = L.resolve_hit(kp, acc, H, st.n);
        RT_PHASE(2);
        // ---- 3. lanes whose task is done take the next one -----------------
        const bool need = L.state == SM_CAM && L.s >= s1;
        const unsigned long long nm = __ballot(need);
        if (nm) {                    // wave-uniform: tasks for the lanes that need one
            // launch constants re-read here (SMEM) instead of living in SGPRs
            // spilled to VGPR lanes across the whole round
            const KParamsK K = kp_here();
            const unsigned nn = (unsigned)__popcll(nm), avail = qe - qb;
            const unsigned rank = (unsigned)__popcll(nm & ((1ull << lane) - 1ull));
            // lanes take the rest of the current batch first (old), the others the
            // new batch's first tasks.  TTAB: a batch's 64 tasks are decoded once,
            // by the whole wave, into the wave's LDS table when the batch is
            // grabbed; a lane taking a task reads its entry, old lanes before the
            // new batch overwrites the table.  Otherwise a lane decodes its own
            // task t in registers.
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
                    if constexpr (LIST) decode_list_task(K, nb + (unsigned)lane, d);
                    else decode_task(K, nb + (unsigned)lane, d);
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
                if constexpr (!TTAB) {
                    if constexpr (LIST) decode_list_task(K, t, e);
                    else decode_task(K, t, e);
                }
                ++ntasks;
                if (owns) {              // task done: its sums to the chunk partials (list form: the band's)
                    double* q = K->partial + (size_t)qidx * 9;
#pragma unroll
                    for (int j = 0; j < 9; ++j) q[j] = acc[j * 256];
                    owns = false;
                }
                if (e[0] == 0xffffffffu) {
                    L.state = SM_DONE;
                } else if (e[1] != 0xffffffffu) {  // else no work (a padding row; list: not a pixel): the next task next round
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
        RT_PHASE(3);
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
            // draws: a bounce uses draws n, n+1 of its sample (rtutility.h:
            // 189-203); a camera ray draws 0-3 of sample s (main.c:265-269);
            // ROLE_AO draws n+2, n+3 of block n/4 and keeps n, n+1 in the
            // cache's words 0-1 for ROLE_PBOUNCE
            const uint32_t nd = cam ? 0u : st.n;
            const uint32_t sa = nd & 3u, sb = (nd + 1u) & 3u;
            uint32_t wa = 0, wb = 0;
            Philox blk{0, 0, 0, 0};
            Philox pblk;                 // (PD) its block: read by camera lanes alone, which make it
            if constexpr (PD) {
                // the same words of the same blocks as below, from L.i instead of
                // st.n (n = 4 + 2i).  A camera lane's block leaves kw2, kw3 what its
                // sample never reads: bounce 0 opens block 1.
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
                // rpre: a refraction lane whose direction draws are
                // both cached (n = 2 mod 4) but whose refraction draw n+2 opens
                // the next block makes that block here, in the round's one Philox,
                // instead of in finish_bounce's own (a second Philox per round)
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
                // (PD) the origin straight into L.o: only camera lanes are here
                X = camera_ray_raw<false>(kp, x, g, w, kp.cam_pin != 0, PD ? L.o : no);
            } else {
                // random_dir_no_norm (rtutility.h:189-203), then n + dir (main.c:163)
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
            } else if (aor) {                                  // ambient_occlusion's cast (main.c:96-103)
                L.cd = dn;
                L.ao_cast = true;
                L.state = SM_CAST;
            } else if (pbr) {                                  // main.c:161-166 after the AO cast
                const V3 reflected_dir = L.d - muls(H.hn, 2 * dot(L.d, H.hn));
                L.d = dn + muls(reflected_dir - dn, H.rs);
                L.cd = L.d;
                L.state = SM_CAST;
            } else {
                L.finish_bounce(kp, dn, st, acc, H);
            }
        }
    }
    if (kp.trace) {                  // diagnostics (RT_QUEUE_TRACE): per lane start, end, rounds, tasks
        unsigned long long* q = kp.trace + ((size_t)blockIdx.x * 256 + threadIdx.x) * RT_TRACE_WORDS;
        q[0] = (unsigned long long)t_start;
        q[1] = (unsigned long long)wall_clock64();
        q[2] = rounds;
        q[3] = ntasks;
#if RT_DIAG_STALE == 2
        q[2] = diag_cnt()[0];        // diagnostic: node visits and stale visits of the lane
        q[3] = diag_cnt()[256];
#endif
#if RT_DIAG_MERGE
        q[2] = diag_merge()[DM_FLAGGED_ONE];     // diagnostic: the wave's flagged pairs with one tail, with two
        q[3] = diag_merge()[DM_FLAGGED_TWO];
        q[0] = diag_merge()[DM_FORWARD_ONE];     // ... and its forward pairs (in place of the clocks)
        q[1] = diag_merge()[DM_FORWARD_TWO];
#endif
#if RT_PHASE_CLOCK
        for (int k = 0; k < 5; ++k) q[4 + k] = ph[k];
#endif
    }
}

}  // namespace rt
