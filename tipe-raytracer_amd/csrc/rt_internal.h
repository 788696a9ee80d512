// rt_internal.h — device-side scene layout and launch descriptors shared by
// the C-ABI (rt_api.cpp; the scene's arrays are made by rt_scene_prep.cpp, the
// descriptor and the launch plan by rt_launch_plan.cpp) and the kernels
// (rt_kernels.hip and the headers it includes).
//
// HBM layout of one uploaded scene (DESIGN.md "Data layout"):
//   SphCand [ns_pad] 32 B  center, |C|^2 - radius^2 — the candidate pass,
//                          scanned wave-uniformly through the scalar unit,
//                          two records per s_load_dwordx16; padded to an even
//                          count with never-hit records (k = +inf); in the
//                          host's pairing order (rt_scene_prep.cpp pair_candidates)
//   int     [ns_pad]       the sphere index of each candidate record, and
//   SphGeo  [ns_pad]       its SphGeo (the candidate pass's winner)
//   SphGeo  [ns_pad] 32 B  center, radius^2 — the exact reference test
//                          (winner, fallback scan; r2 = -inf padding)
//   DevMat  [ns]     80 B  sphere material — gathered for the winner only
//   TriGeo  [nt]     96 B  A, B-A, C-A, N  — scanned wave-uniformly
//   TriTex  [nt]    136 B  B, C, uvA/B/C, material, unit normal, area terms — winner only
//   BvhNode4[nodes] 128 B  four child boxes (rt_bvh.h) when nt > 32; the
//   int     [nt]           triangle arrays are then in leaf order and
//                          tri_orig maps back to the caller's order
//   BvhNodeH[nodes]  64 B  the same tree for the queue kernel, or, for a wide
//   BvhNodeW[nodes]  64 B  tree (nt > 65535, rt_bvh.h), its form with 32-bit bases
//   DevMat  [nm*th*tw]     texel table (reference `material` records)
//   DevMat  [nt]           rt_triangle.mat per triangle (RT_SEM_CUDA materials)
//   double  [ns][3]        the colour an emitting sphere shows when seen
//                          directly: hsl_to_rgb(rgb_to_hsl(emission))
// Per launch: a 18-double uniform block (camera, focus, aperture, AO, W-1,
// H-1) read through the scalar unit where used, and, when the samples of a
// pixel are split over P chunks, a [P][pixels][9] partial-sum scratch.
#pragma once
#include <cstdint>

namespace rt {

struct BvhNode4;                                      // rt_bvh.h
struct BvhNodeH;                                      // rt_bvh.h (64-byte form)
struct BvhNodeW;                                      // rt_bvh.h (64-byte form of a wide tree)

struct SphGeo { double cx, cy, cz, r2; };            // r2 = radius*radius (sphere.h:22)
// Candidate-pass record (rt_spheres.h spheres_closest): center and
// k = |C|^2 - r2 (host, long double), so c*a = a*|o|^2 - 2a*o.C + a*k is an
// FMA chain; padding records have k = +inf (never hit).
struct SphCand { double cx, cy, cz, k; };
struct DevMat {                                       // == material, hitinfo.h:6-13
    double dr, dg, db;       // diffuseColor
    double er, eg, eb;       // emissionColor
    double es, rs, alpha, ior;
};
struct TriGeo {                                       // mesh.h:72-74 precomputed
    double ax, ay, az;
    double abx, aby, abz;
    double acx, acy, acz;
    double nx, ny, nz;       // cross(B-A, C-A), unnormalised
};
struct TriTex {                                       // what tri_uvmapping reads
    double bx, by, bz, cx, cy, cz;
    double uau, uav, ubu, ubv, ucu, ucv;
    int mat;                 // quelMatPourTri[i]
    int tex0;                // the texel index when every uv is 0 (it is then (0, 0) of
                             // material mat for any finite hit), else -1
    double unx, uny, unz;    // vec3_normalize(N) (mesh.h:91), host-computed: the hit normal
    double area;             // get_barycentric_coord's areaABC = dot(un, N) (texture.h:18)
};
static_assert(sizeof(SphGeo) == 32, "SphGeo");
static_assert(sizeof(SphCand) == 32, "SphCand");
static_assert(sizeof(DevMat) == 80, "DevMat");
static_assert(sizeof(TriGeo) == 96, "TriGeo");
static_assert(sizeof(TriTex) == 136, "TriTex");
// tri_uvmapping's u, v as affine functions of the hit point (rt_scene_prep.cpp
// tri_uv_affine): u(P) = u0 + gu.(P - A), v(P) = v0 + gv.(P - A), with
// tw*|u_ref - u| <= eu (th*|v_ref - v| <= ev) for every P within diam
// (max-norm) of A, u_ref being the reference's rounded u; diam < 0: no fast
// path for this triangle
struct TriUV {
    double gux, guy, guz, u0;
    double gvx, gvy, gvz, v0;
    double eu, ev, diam;
};
static_assert(sizeof(TriUV) == 88, "TriUV");

// uniform block (doubles)
enum : int {
    U_CAM_O = 0, U_CAM_H = 3, U_CAM_V = 6, U_CAM_C = 9,
    U_FOCUS = 12, U_OX, U_OY, U_AO, U_WM1, U_HM1,
    U_RC_WM1, U_RC_HM1,      // rcp_refined(W-1), rcp_refined(H-1) (device-computed), or 0: plain division
    U_COUNT
};

// Everything one render launch needs, passed by value as the kernel argument.
struct KParams {
    // scene
    const SphGeo* sph;
    const SphCand* sph_cand; // candidate-pass records [ns_pad]
    double cand_lmax;        // >= max_k |C_k| + R_k (+inf: candidate pass off, exact scans)
    const DevMat* sph_mat;
    const TriGeo* tri;
    const TriTex* tri_tex;
    const TriUV* tri_uv;     // (textured scenes) the affine texel map, null: every hit takes the exact path
    const DevMat* texels;
    const double* uni;       // U_COUNT doubles
    const BvhNode4* bvh;     // 4-wide triangle BVH (rt_bvh.h), or null: brute-force scan
    union {                  // the same tree in 64-byte nodes (the queue kernel's), or null: a tree has
        const BvhNodeH* bvhh;    // one such form, BvhNodeH, or (bvh_wide) BvhNodeW, so the two share the
        const BvhNodeW* bvhw;    // kernarg slot (a new field would move every kernel's argument size)
    };
    const int* tri_orig;     // triangle k's index in the caller's list (null: k)
    const DevMat* sky;       // sky texels when sky mode is on, else null
    const DevMat* tri_mat;   // rt_triangle.mat per triangle (leaf order with a BVH): RT_SEM_CUDA
    int cuda;                // rt.h RT_SEM_CUDA (render_kernel_cuda)
    int bvh_wide;            // the tree is wide (rt_bvh.h: node or triangle indices beyond 16 bits): only the
                             // kernels with wider stack entries may walk it, and its 64-byte form is bvhw
                             // (the slot of r05's removed RT_PREC_FP32 flag)
    double cbb[6];           // RT_SEM_CUDA: the triangles' box (lo xyz, hi xyz), hit_BBox
    const double* sph_rinv;  // 1/radius per sphere (sphere_uvmapping's divide)
    const double* sph_disp;  // per sphere: hsl round trip of its emission (main.c:155-158), 3 doubles
    int sky_w, sky_h;
    double bvh_srel, bvh_sabs;   // distance-cull slack (rt_bvh.cpp)
    float bvh_rbox;              // >= |every bound| of the tree's boxes (single-precision slab margin)
    int bvh_stack;               // host only (plan_render): stack entries the tree can need (BvhBuild::stack4),
                                 // 1 << 30 when a narrow tree's node index does not fit 16 bits
    int bvh_steps;               // host only (plan_render): 4 for a tree of 4-wide depth <= 4, else 3
    int bvh_nodes;               // 4-wide nodes (breadth-first order: the top levels first)
    int ns, ns_pad, nt;
    int tw, th;
    long long n_texels;
    // image / integrator
    int W, H, S, B;
    int useAO;
    int zero_exit;           // paths end once rayColor == 0 (host: only where exact, LanePath::zero_rc)
    int tex_const;           // TriTex::tex0 stands for tri_texel (host: every triangle has one,
                             // and every coordinate and ray origin is within 2^100, so the
                             // barycentrics of a hit are finite)
    int cam_pin;             // aperture 0 and no -0 camera coordinate: co + (jx*0, jy*0, 0) == co exactly
    uint32_t key0, key1;
    int chunks;              // samples of a pixel split into this many chunks
    int chunk_taper;         // rt_chunk_bound's taper levels L (0: equal slices)
    unsigned chunk_den;      // rt_chunk_bound's divisor: chunks, or (chunks - L) 2^L + 2^L - 1 tapered
    // tiling
    int row_base, tile_rows, tile_first, tile_step, n_tiles, row_end;
    int local_rows;          // n_tiles * tile_rows
    int band_y0, band_rows;  // local rows [band_y0, band_y0 + band_rows) of this launch (partials are per band)
    // outputs (device, local frame of local_rows x W colors)
    double* canva;
    double* albedo;
    double* normal;
    double* radiance;
    double* partial;         // chunks > 1: [chunks][band_rows*W][9]
    double* sums;            // accumulate mode (rt_accumulate_async): [local_rows*W][9] running sums, or null
    long long s_base;        // global index of this launch's first sample (Philox counter word 3)
    unsigned* task_ctr;      // render_kernel_q's task counter (zeroed per band launch), or null
    unsigned npx_here;       // render_kernel_q: pixels of this band that exist (tasks = npx_here * chunks)
    unsigned qm_npx, qm_w, qm_tile, qm_chunks;   // floor((2^32-1)/d) for d = npx_here, W, tile_rows,
                                                 // chunks (udiv_q); qm_chunks 0: 64-bit chunk starts
    int acc_queue;           // host only (plan_render): rt_set_accumulate_queue's switch -- a launch with running
                             // sums may take the queue kernel.  (In the padding before trace: no field moves.)
    unsigned long long* trace;   // render_kernel_q diagnostics (RT_QUEUE_TRACE), normally null
    unsigned long long* counters;
    int opaque;              // host only (plan_render: QB -2): every sphere material opaque, !(alpha < 0.0001)
                             // && !(alpha <= 0.99) (no hole, no refraction).  Last, so the other fields
                             // keep their kernarg offsets (and the kernels their SMEM loads)
    int opaque_all;          // host only (plan_render: OPQ): ... and so is every triangle material: every
                             // texel, no material index 3 or 4 (tri_material's alpha overrides)
    int ns_cand;             // spheres the candidate pass scans: ns_pad, or 0 when cand_lmax is +inf (every
                             // ray then takes the exact scan: non-finite spheres, or more than 65534
                             // spheres, whose slots do not fit cand_tag's 16 bits)
    int stack_cap;           // COUNT runs only: BVH stack entries of the kernel a render of these params
                             // takes (RenderPlan::stack_cap), which they check every push against
    double bvh_rb;           // the origin bound R_b the tree's padding assumed (rt_bvh.h r_scene)
    double bvh_kdelta;       // padding growth per unit of origin beyond it (rt_bvh.h k_delta)
    float bvh_rb_f;          // a float with rb_f (1 + 2^-23) <= R_b (the walk's cheap "inside" test)
    int bvh_far;             // some ray origin may lie beyond R_b: a sphere or the camera does
    int ns_merge;            // the first ns_merge (even) candidate records are pairs that may share one
                             // root tail (rt_scene_prep.cpp pair_candidates; a hint, any value gives the same result)
    int ns_fwd;              // the next ns_fwd (even) records are forward pairs, which share it by another test
                             // (a hint as well; in the padding before cand_orig: no field moves)
    const int* cand_orig;    // [ns_pad] candidate record (slot) j describes sphere cand_orig[j] of sph
    const SphGeo* sph_slot;  // [ns_pad] sph[cand_orig[j]]: the candidate pass's winner retest
};
static_assert(sizeof(KParams) == 512, "KParams is the kernel argument: no field is added, removed or moved");

struct RenderPlan;                                    // rt_launch_plan.h
struct UniBlock { double v[U_COUNT]; };

// launchers (rt_kernels.hip): one band of a render or a count run, as planned
int launch_set_uniforms(const UniBlock& u, double* d_uni, void* stream);
int launch_render(const KParams& kp, const RenderPlan& plan, void* stream);
// Name of the render kernel of the calling thread's last launch_render.
const char* last_render_kernel();
int launch_count(const KParams& kp, const RenderPlan& plan, void* stream);
int launch_assemble(const double* gathered, long long rank_stride, int world, int tile_rows,
                    int rows_per_rank, int W, int H, double* out, void* stream);
int launch_selftest(int op, const double* d_in, double* d_out, int n, void* stream);
int launch_verify_phi(unsigned long long r0, unsigned long long n, unsigned long long* d_counts);
int launch_verify_normalize(unsigned long long seed, unsigned long long n, unsigned long long* d_counts);
int launch_verify_spheres(const KParams& kp, const double* d_rays, long long n, unsigned long long* d_counts);
int launch_verify_texel(const KParams& kp, const double* d_pts, const int* d_tri, long long n,
                        unsigned long long* d_counts);
int launch_resolve(const KParams& kp, void* stream);
int launch_denoise_pack(long long npx, const double* canva, const double* albedo, const double* normal,
                        float* color3, float* albedo3, float* normal3, void* stream);
// launchers (rt_denoise.hip): the built-in a-trous denoiser (rt.h "built-in denoiser") on a device frame.
// The workspace holds four planes of denoise_plane_floats(W*H) floats; albedo / normal may be null.
size_t denoise_plane_floats(long long npx);
int launch_denoise(int W, int H, double* canva, const double* albedo, const double* normal, int iterations,
                   float sigma_color, float sigma_normal, float sigma_albedo, float* workspace, float* color3_out,
                   void* stream);
// launchers (rt_vdenoise.hip): the variance-guided denoiser (rt.h "variance-guided denoiser") on two device
// accumulators.  The workspace holds four planes of denoise_plane_floats(W*H) floats, then three of
// vdenoise_scalar_floats(W*H); albedo / normal / radiance may be null.  rounds null: every pixel holds spp_half
// samples per accumulator; else pixel p holds spp_half * 2^(k-1), k = rounds[p] clamped to 1..32 (rt.h
// "per-pixel sample counts"), and spp_half is the adaptive schedule's first_half.
size_t vdenoise_scalar_floats(long long npx);
int launch_vdenoise(int W, int H, const double* sums_a, const double* sums_b, const int* rounds, int spp_half,
                    int iterations, float sigma_luminance, float sigma_normal, float sigma_albedo, float* workspace,
                    double* canva, double* albedo, double* normal, double* radiance, void* stream);

// launchers (rt_adaptive.hip): adaptive sampling (rt.h "adaptive sampling").
// What a list launch needs besides KParams, as the render kernel's second
// by-value argument (KParams stays as it is): one band [e0, e1) of the entries.
struct ListArgs {
    const unsigned* list;    // global pixel indices j*W+i, ascending
    const unsigned* count;   // device word: entries of the list (the kernel clamps it to e1)
    double* partial;         // chunks > 1: [chunks][stride][9], indexed by entry - e0
    unsigned e0, e1;         // this launch's entries; e1 <= list_cap
    unsigned stride;         // entries of one chunk's plane of partial (the band size)
};
int launch_render_list(const KParams& kp, const RenderPlan& plan, const ListArgs& la, void* stream);
// launcher (rt_queue_list.hip): the same band on the list form of render_kernel_q<plan.qb, plan.opq, ...>
// (reported as render_kernel_ql; plan.queue; chunks > 1), then combine_list_kernel.  kp.task_ctr: the launch's task counter, with
// kListTaskWords launch-private words kListTaskOffset words behind it (the band's task count, entry count and
// division magic, which a prologue kernel derives from the device's count word).
constexpr int kListTaskOffset = 16, kListTaskWords = 3;
// A launch's stream-ordered scratch (LaunchScratch, rt_api_internal.h), one layout for every launch: the uniform
// block; in double kTaskCtrDouble the queue's task counter, on a 64-byte line of its own; the list form's words
// kListTaskOffset words behind it, on the next line.  The kernels read through these offsets.
constexpr int kTaskCtrDouble = ((U_COUNT + 7) / 8 + 1) * 8;
constexpr size_t kTaskCtrByte = kTaskCtrDouble * sizeof(double);
constexpr size_t kLaunchScratchBytes = kTaskCtrByte + (kListTaskOffset + kListTaskWords) * sizeof(unsigned);
static_assert(kTaskCtrByte % 64 == 0 && kTaskCtrByte >= U_COUNT * sizeof(double),
              "the counter starts a 64-byte line past the uniforms");
static_assert(kListTaskOffset * sizeof(unsigned) == 64, "the list words start on the line behind the counter's");
constexpr int kListLastWord = kListTaskOffset + kListTaskWords - 1;    // counted from the counter, as the kernels index
static_assert(kTaskCtrByte + (kListLastWord + 1) * sizeof(unsigned) <= kLaunchScratchBytes,
              "the allocation covers the last list word");
static_assert(U_COUNT != 20 || (kTaskCtrByte == 256 && kLaunchScratchBytes == 332), "the offsets of 20 uniforms");
int launch_render_list_queue(const KParams& kp, const RenderPlan& plan, const ListArgs& la, void* stream);
// combine_list_kernel (rt_adaptive.hip) for one band, as launch_render_list ends with it.
int launch_combine_list(const KParams& kp, const ListArgs& la, void* stream);
// One selection pass (rt_adaptive_select_async) or one marking of the active
// pixels' round counts, as their kernels' by-value argument.
struct AdaptiveSelect {
    int W, H;
    unsigned npx;            // W * H <= 2^30
    int all;                 // round 0: every pixel is active and the incoming list is not read
    const double* sums_a;
    const double* sums_b;
    double rap;              // 1.0 / n_half
    float tolerance;
    int round;
    unsigned* list;          // in: the active pixels (unless all); out: those that go on
    unsigned* count;         // in / out: entries of list
    int* rounds;
    float* v;                // workspace planes: v and y per pixel (kept between calls),
    float* y;
    unsigned* keep;          //   per active entry its pixel or "settled" (padded to whole blocks of 256),
    unsigned* counts;        //   kept entries per block of 256, then their exclusive scan,
    unsigned* n_in;          //   and the incoming count (the scatter reads it after *count changed)
};
unsigned adaptive_blocks(long long npx);                // blocks of 256 entries: the length of counts
int launch_adaptive_select(const AdaptiveSelect& s, void* stream);
int launch_adaptive_mark(const AdaptiveSelect& s, int value, void* stream);
int launch_adaptive_resolve(long long npx, const double* sums_a, const double* sums_b, const int* rounds,
                            int first_half, double* canva, double* albedo, double* normal, double* radiance,
                            void* stream);

}  // namespace rt
