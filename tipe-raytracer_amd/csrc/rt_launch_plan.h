// rt_launch_plan.h — host-only launch descriptors and the launch plan: how a
// prepared scene (rt_scene_prep.h) and the caller's rt_params become KParams
// (fill_kparams), and which kernel, stack and row bands a launch of them takes
// (plan_render).  No HIP: the C-ABI (rt_api.cpp launch_on_stream) executes the
// plan through rt_kernels.hip, tools/probes/launch_plan_check.cpp tests it on
// the CPU.
#pragma once
#include <cstring>

#include "rt_queue_variants.h"
#include "rt_scene_prep.h"

namespace rt {

// The pointer a kernel gets for one scene array: a HostScene's vector (null
// when empty, as rt_scene_upload leaves an empty array) or a DevArray.
template <class T>
const T* array_ptr(const std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }
template <class A>
auto array_ptr(const A& a) -> decltype(a.p) { return a.p; }

// Scene fields by consumer; the rt_verify_* descriptors (rt_diag.cpp) are these
// alone.  The spheres' geometry and the candidate pass:
template <template <class> class Array>
void set_sphere_fields(KParams& kp, const SceneArrays<Array>& a, const SceneFacts& f)
{
    kp.sph = array_ptr(a.sph);
    kp.sph_cand = array_ptr(a.sph_cand);
    kp.cand_orig = array_ptr(a.cand_orig);
    kp.sph_slot = array_ptr(a.sph_slot);
    kp.cand_lmax = f.cand_lmax;
    kp.ns = f.ns;
    kp.ns_pad = f.ns_pad;
    kp.ns_cand = std::isfinite(f.cand_lmax) ? f.ns_pad : 0;
    kp.ns_merge = f.ns_merge;
    kp.ns_fwd = f.ns_fwd;
}
// ... the triangles' geometry and the texel map:
template <template <class> class Array>
void set_triangle_fields(KParams& kp, const SceneArrays<Array>& a, const SceneFacts& f)
{
    kp.tri = array_ptr(a.tri);
    kp.tri_tex = array_ptr(a.tri_tex);
    kp.tri_uv = array_ptr(a.tri_uv);
    kp.tw = f.tw;
    kp.th = f.th;
    kp.n_texels = f.n_texels;
}

// The parts of fill_kparams that read no scene array (rt_launch_plan.cpp).  set_camera returns the
// camera's reach: >= |every camera ray origin coordinate|, +inf for a non-finite camera.
double set_camera(KParams& kp, double* uni, const rt_params* p);
void set_gates(KParams& kp, const SceneFacts& f, const rt_params* p, double AO, double reach, bool zero_exit);
void set_bvh(KParams& kp, const SceneFacts& f, const rt_params* p, double reach, const BvhNode4* bvh,
             const BvhNodeH* bvhh, const BvhNodeW* bvhw);
void set_chunking(KParams& kp, const rt_params* p);
void set_tiling(KParams& kp, const rt_tiling* t, int H);

// The launch descriptor of scene (a, f) under params p and tiling t, and the
// uniform block uni[U_COUNT].  zero_exit: rt_set_zero_throughput_exit's switch.
// Outputs, band fields, task counter and stack_cap are the launch's to set.
template <template <class> class Array>
void fill_kparams(const SceneArrays<Array>& a, const SceneFacts& f, const rt_params* p, const rt_tiling* t,
                  bool zero_exit, KParams& kp, double* uni)
{
    std::memset(&kp, 0, sizeof kp);
    set_sphere_fields(kp, a, f);
    set_triangle_fields(kp, a, f);
    kp.sph_mat = array_ptr(a.sph_mat);
    kp.sph_rinv = array_ptr(a.sph_rinv);
    kp.sph_disp = array_ptr(a.sph_disp);
    kp.texels = array_ptr(a.texels);
    kp.tri_orig = array_ptr(a.tri_orig);
    kp.tri_mat = array_ptr(a.tri_mat);
    kp.nt = f.nt;
    for (int i = 0; i < 6; ++i) kp.cbb[i] = f.cbb[i];
    if (p->sky_mode == RT_SKY_LAST_SPHERE && array_ptr(a.sky) && f.ns > 0) {
        kp.sky = array_ptr(a.sky);
        kp.sky_w = f.sky_w;
        kp.sky_h = f.sky_h;
    }
    const double reach = set_camera(kp, uni, p);
    set_gates(kp, f, p, uni[U_AO], reach, zero_exit);
    set_bvh(kp, f, p, reach, array_ptr(a.bvh), array_ptr(a.bvhh), array_ptr(a.bvhw));
    set_chunking(kp, p);
    set_tiling(kp, t, p->hauteur_image);
}

// One launch of kp, decided once (plan_render) and executed by launch_render /
// launch_count (rt_kernels.hip).
struct RenderPlan {
    int band_rows;           // local rows per launch; the partials are per band (a count run: one band)
    size_t partial_bytes;    // chunk partials of one band, [chunks][band_rows*W][9] doubles (0: none)
    bool task_ok;            // spp_chunks > 1 and the render's tasks per band fit the queue's 32-bit numbering
    bool queue;              // the render is render_kernel_q<qb, opq, sky, ao> -- (qb, opq) one of
                             // rt_queue_variants.h kQueueVariants --, else the fixed grid's
    int qb;
    bool opq, sky, ao;
    bool cuda, bvh, wide;    // the fixed-grid instantiation (with sky); a count run always takes it
    int stack_cap;           // BVH stack entries of the render's kernel (0 without a BVH): KParams::stack_cap
    const char* name;        // the render's kernel, as rt_last_render_kernel() reports it
};
RenderPlan plan_render(const KParams& kp, bool count);

// The entry bands of a list launch (rt_accumulate_list_async) of up to list_cap
// entries with `chunks` sample slices; launch_render_list (rt_adaptive.hip) or,
// when plan_render gives the launch the queue, launch_render_list_queue
// (rt_queue_list.hip) runs one band.
struct ListPlan {
    unsigned band;           // entries per launch; the partials are per band (chunks 1: one band, no partials)
    size_t partial_bytes;    // chunk partials of one band, [chunks][band][9] doubles (0: none)
};
ListPlan plan_list(int chunks, unsigned list_cap);

}  // namespace rt
