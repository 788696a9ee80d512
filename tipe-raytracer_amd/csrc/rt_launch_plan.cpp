// rt_launch_plan.cpp — the scene-independent parts of fill_kparams and the
// launch plan (rt_launch_plan.h).  Host only, no HIP.
#include "rt_launch_plan.h"

#include <algorithm>
#include <cstdlib>

namespace rt {

// Image, integrator, camera and the uniform block.
double set_camera(KParams& kp, double* uni, const rt_params* p)
{
    kp.cuda = p->semantics == RT_SEM_CUDA ? 1 : 0;
    kp.W = p->largeur_image;
    kp.H = p->hauteur_image;
    kp.S = p->nbRayonParPixel;
    kp.B = p->nbRebondMax;
    kp.useAO = p->useAO ? 1 : 0;
    kp.key0 = (uint32_t)p->seed;
    kp.key1 = (uint32_t)(p->seed >> 32);
    const double* o = p->cam.origin.e;
    for (int i = 0; i < 3; ++i) {
        uni[U_CAM_O + i] = o[i];
        uni[U_CAM_H + i] = p->cam.horizontal.e[i];
        uni[U_CAM_V + i] = p->cam.vertical.e[i];
        uni[U_CAM_C + i] = p->cam.coin_bas_gauche.e[i];
    }
    const bool ints = p->compat_int_truncation && p->semantics != RT_SEM_CUDA;   // ThreadData int fields, main.c:42-43
    const auto thread_data = [ints](double x) { return ints ? (double)(int)x : x; };
    const double ox = thread_data(p->ouverture_x), oy = thread_data(p->ouverture_y);
    uni[U_FOCUS] = thread_data(p->focus_distance);
    uni[U_OX] = ox;
    uni[U_OY] = oy;
    uni[U_AO] = thread_data(p->AO_intensity);
    uni[U_WM1] = (double)(p->largeur_image - 1);    // main.c:265 (largeur_image-1)
    uni[U_HM1] = (double)(p->hauteur_image - 1);
    uni[U_RC_WM1] = uni[U_RC_HM1] = 0.0;            // refined on the device (set_uniforms_kernel)
    // camera.h:49-54: the ray starts at origin + (jx*ox, jy*oy, 0); with ox = oy = 0
    // the offsets are +-0 and the sum is the origin itself unless a coordinate is -0
    const auto neg0 = [](double x) { return x == 0.0 && std::signbit(x); };
    kp.cam_pin = ox == 0.0 && oy == 0.0 && !neg0(o[0]) && !neg0(o[1]) && !neg0(o[2]);
    // primary rays start at the camera origin + (dx, dy, 0), |dx| <= |ox|/2
    double reach = std::max({0.0, std::fabs(o[0]), std::fabs(o[1]), std::fabs(o[2])}) +
                   0.5 * (std::fabs(ox) + std::fabs(oy));
    if (!std::isfinite(reach) || !std::isfinite(o[0]) || !std::isfinite(o[1]) || !std::isfinite(o[2]))
        reach = HUGE_VAL;                // std::max drops NaN: no gate may pass on a NaN camera
    return reach;
}

// What the kernels may skip because the result stays exact.
void set_gates(KParams& kp, const SceneFacts& f, const rt_params* p, double AO, double reach, bool zero_exit)
{
    const double extent = std::fmax(f.coord_max, reach);
    // Zero-throughput exit (rt_fixed_grid.h LanePath::zero_rc): exact when the
    // shading values are bounded and, with AO, the AO factor stays finite.
    kp.zero_exit = zero_exit && p->semantics != RT_SEM_CUDA && f.mats_bounded &&
                   (!p->useAO || (AO > 0.0 && AO <= 1000.0 && extent <= 0x1p20));
    // TriTex::tex0 (constant texels of uv-less triangles): a hit point P is then
    // within ~2^101 of the origin, the signed areas of get_barycentric_coord stay
    // below 2^205 and areaABC >= |N| (1 - 2^-50) with |N| >= 1e-6 / |d| for any
    // hit (det >= 1e-6), so the barycentrics are finite and u = v = +-0
    kp.tex_const = f.all_tex0 && extent <= 0x1p100;
    // read by plan_render only (the kernels are instantiated per value)
    kp.opaque = f.sph_opaque ? 1 : 0;
    kp.opaque_all = f.sph_opaque && (f.nt == 0 || f.tri_opaque) ? 1 : 0;
}

// The BVH padding assumed every ray origin within r_scene (rt_bvh.cpp); origins
// beyond it -- the camera, hit points on far spheres -- widen the walk's margins
// per ray (rt_triangles.h ray32); a non-finite camera takes the every-triangle scan.
void set_bvh(KParams& kp, const SceneFacts& f, const rt_params* p, double reach, const BvhNode4* bvh,
             const BvhNodeH* bvhh, const BvhNodeW* bvhw)
{
    if (!bvh || p->accel != RT_ACCEL_AUTO || !std::isfinite(reach)) return;
    kp.bvh = bvh;
    kp.bvhh = bvhh;
    kp.bvh_srel = f.s_rel;
    kp.bvh_sabs = f.s_abs;
    kp.bvh_rb = f.r_scene;
    kp.bvh_kdelta = f.k_delta;
    float rf = (float)f.r_scene;              // rb_f (1 + 2^-23) <= R_b
    while (rf > 0.0f && (double)rf * (1.0 + 0x1p-23) > f.r_scene) rf = std::nextafter(rf, 0.0f);
    kp.bvh_rb_f = rf;
    // origins: the camera (+ aperture), hit points on the spheres and on the
    // triangles (inside R_b by construction)
    kp.bvh_far = !(reach <= f.r_scene && f.sph_bound <= f.r_scene);
    kp.bvh_rbox = f.bvh_rbox;
    kp.bvh_nodes = f.bvh_nodes;
    // plan_render's inputs.  The stack entries the tree can need (rt_bvh.cpp's
    // exact bound), or more than any stack when a node index would not fit a
    // narrow tree's uint16 entries; a wide tree (rt_bvh.h) has 32-bit stacks and
    // its own 64-byte nodes, so its bound always counts
    kp.bvh_stack = (f.bvh_nodes < 0x8000 && f.nt <= 0x8000) ? f.bvh_stack4 : 1 << 30;
    if (f.bvh_wide) {
        kp.bvh_wide = 1;
        kp.bvhw = bvhw;
        kp.bvh_stack = f.bvh_stack4;
    }
    // shallow trees finish most walks in one round with 4 visits; deeper ones
    // do best with 3 (measured: sweep depth4 3: 3395 -> 3542 at 4; C4 depth4 7:
    // 1134 at 3, 1122 at 4)
    kp.bvh_steps = f.bvh_depth <= 4 ? 4 : 3;
}

void set_chunking(KParams& kp, const rt_params* p)
{
    kp.chunks = rt_resolve_spp_chunks(p->spp_chunks, p->nbRayonParPixel);
    kp.chunk_taper = rt_chunk_taper_levels(kp.S, kp.chunks);      // rt.h rt_chunk_bound
    kp.chunk_den = kp.chunk_taper ? (unsigned)(kp.chunks - kp.chunk_taper) * (1u << kp.chunk_taper) +
                                        ((1u << kp.chunk_taper) - 1u)
                                  : (unsigned)kp.chunks;
}

void set_tiling(KParams& kp, const rt_tiling* t, int H)
{
    kp.row_base = t->row_base;
    kp.tile_rows = t->tile_rows;
    kp.tile_first = t->tile_first;
    kp.tile_step = t->tile_step;
    kp.n_tiles = t->n_tiles;
    kp.row_end = H;
    kp.local_rows = t->n_tiles * t->tile_rows;
}

// The one place that decides a launch.
//  * Bands.  With spp_chunks > 1 the chunk partials are bounded by a budget of
//    bytes per launch (4 GiB; RT_PARTIAL_BUDGET, read on every launch, lets a
//    test use a small one): taller frames render in row bands of a multiple of
//    16 rows, at least 16, that reuse one buffer (pixels are independent, so
//    banding changes no result).  A count run is one band without partials.
//  * Queue or fixed grid.  render_kernel_q needs its task counter (task_ok: the
//    render band's chunks * pixels below 2^31), RT_SEM_MAIN_C and, with a BVH, a
//    walk that admits the tree; every other launch takes the fixed grid (kStack4
//    entries).  A launch with running sums (rt_accumulate_async) takes the fixed
//    grid too unless kp.acc_queue (rt_set_accumulate_queue) is set; with it, the
//    rules, the pair, the stack and the bands are a render launch's, and
//    combine_kernel adds the slice partials to the sums in slice order.  One
//    slice (chunks 1) never has a task counter: it carries the sums through the
//    samples on the fixed grid.  A list launch (rt_accumulate_list_async) takes
//    the list form of render_kernel_q of the same pair when this plan says queue.
//  * Which queue kernel: one of rt_queue_variants.h's kQueueVariants, which says
//    what each (QB, OPQ) pair walks, its stack and whether it has the far-origin
//    margins.  The rules here admit a scene to a pair.
//  * Which walk, by the tree's exact stack bound (bvh_stack; narrow trees above
//    kStackQN: none).  QB_TOP takes shallow trees (bvh_steps 4) and deep ones
//    that have no 64-byte nodes, when the bound fits and no origin is far.
//    Everything else is QB_DEEP, if the tree has its 64-byte nodes bvhh; the OPQ
//    form when every material is opaque, the bound fits and no origin is far.
//  * A wide tree (indices beyond 16 bits) takes QB_WIDE when its own 64-byte
//    nodes bvhw packed and the bound fits, else the fixed grid's wide
//    instantiation; no narrow kernel walks it, and a narrow tree never takes a
//    wide kernel.
//  * Without a BVH: QB_SPH_OPAQUE, QB_SPH or QB_SCAN.
// stack_cap and name are the pair's table entry (the fixed grid: kStack4); COUNT
// runs check every push against stack_cap (RT_CNT_BVH_STACK_OVER).
RenderPlan plan_render(const KParams& kp, bool count)
{
    RenderPlan pl = {};
    const size_t row_bytes = (size_t)kp.chunks * kp.W * 9 * sizeof(double);
    int band = kp.local_rows;
    if (kp.chunks > 1) {
        const char* e = std::getenv("RT_PARTIAL_BUDGET");
        const long long v = e ? std::atoll(e) : 0;
        const size_t budget = v > 0 ? (size_t)v : ((size_t)4 << 30);
        band = (int)std::min<size_t>(std::max<size_t>(16, budget / row_bytes / 16 * 16), (size_t)kp.local_rows);
    }
    pl.task_ok = kp.chunks > 1 && (unsigned long long)band * kp.W * kp.chunks < (1ull << 31);
    pl.band_rows = count ? kp.local_rows : band;
    pl.partial_bytes = kp.chunks > 1 && !count ? row_bytes * band : 0;
    pl.sky = kp.sky != nullptr;
    pl.ao = kp.useAO != 0;
    pl.cuda = kp.cuda != 0;
    pl.bvh = kp.bvh != nullptr;
    pl.wide = pl.bvh && kp.bvh_wide;
    pl.stack_cap = pl.bvh ? kStack4 : 0;
    const bool can_queue = pl.task_ok && !pl.cuda && (!kp.sums || kp.acc_queue);
    if (pl.wide) {
        if (can_queue && kp.bvhw != nullptr && kp.bvh_stack <= kStackQW) {
            pl.queue = true;
            pl.qb = QB_WIDE;
        }
    } else if (!pl.bvh) {
        pl.queue = can_queue;
        if (pl.queue) pl.qb = kp.nt == 0 ? (kp.opaque ? QB_SPH_OPAQUE : QB_SPH) : QB_SCAN;
    } else if (kp.bvh_stack <= kStackQN) {
        const bool fits4 = kp.bvh_stack <= kStackQ4 && !kp.bvh_far;
        pl.qb = fits4 && (kp.bvh_steps > 3 || kp.bvhh == nullptr) ? QB_TOP : QB_DEEP;
        pl.queue = can_queue && (pl.qb == QB_TOP || kp.bvhh != nullptr);
        if (pl.queue) pl.opq = pl.qb == QB_DEEP && kp.opaque_all && kp.bvh_stack <= kStackQ && !kp.bvh_far;
    }
    if (pl.queue) {
        const QueueVariant& v = queue_variant(pl.qb, pl.opq);       // (the rules above pick listed pairs)
        pl.stack_cap = v.stack;
        pl.name = v.name;
    } else {
        pl.qb = 0;
        pl.name = pl.cuda  ? "render_kernel_cuda"
                  : pl.bvh ? (pl.wide ? "render_kernel<BVH32>" : "render_kernel<BVH>")
                           : "render_kernel";
    }
    return pl;
}

// Entries per band of a chunked list launch: the whole list (list_cap in whole
// blocks of 256 entries) when its partials, chunks x 72 bytes per entry, fit
// kListPartialBudget, else as many whole blocks as fit.  The count is a device
// word, so every band up to list_cap is launched and each launch ends in a tail
// of half-idle CUs: few large bands cost less than many small ones
// (profiles/adaptive/README.md, "Band size").  512 MiB is what a 1200x900 frame
// may take at P = 32: 232 960 entries, five bands; a small frame takes what its
// own pixels need.  RT_LIST_BAND (entries; tests, experiments) is read on every
// launch, so a test can give a small list several bands.
constexpr size_t kListPartialBudget = (size_t)512 << 20;

ListPlan plan_list(int chunks, unsigned list_cap)
{
    ListPlan pl = {list_cap, 0};
    if (chunks <= 1) return pl;
    const size_t per_entry = (size_t)chunks * 9 * sizeof(double);
    size_t band = std::max<size_t>(256, kListPartialBudget / per_entry / 256 * 256);
    if (const char* e = std::getenv("RT_LIST_BAND")) {
        const long long v = std::atoll(e);
        if (v > 0) band = std::min(band, ((size_t)std::min<long long>(v, 1ll << 30) + 255) / 256 * 256);
    }
    band = std::min(band, ((size_t)list_cap + 255) / 256 * 256);
    pl.band = (unsigned)band;
    pl.partial_bytes = band * per_entry;
    return pl;
}

}  // namespace rt
