// rt_adaptive_api.cpp — adaptive sampling's entry points of the C-ABI (rt.h
// "adaptive sampling"; kernels: rt_adaptive.hip): samples for a list of pixels
// (rt_accumulate_list_async), the selection pass (rt_adaptive_select_async),
// the loop over both (rt_adaptive_async), its resolve
// (rt_resolve_adaptive_async) and the whole-frame renders into host arrays
// (rt_render_adaptive; rt_render_adaptive_vdenoised, which filters the result
// with rt_vdenoise_adaptive_async of rt_denoise_api.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rt_host_slots.h"

using namespace rt;

namespace {

constexpr rt_adaptive_params kDefaults = {8, 5, 1.0f / 64.0f};

// The private workspace of the selection pass (rt_adaptive_workspace_bytes),
// byte offsets: the v and y planes, the keep plane (each padded to whole
// blocks of 256 entries), the block counts, the recorded incoming count; then
// rt_adaptive_async's list and its count.
struct Layout {
    size_t v, y, keep, counts, n_in, list, count, total;
};
Layout layout_of(long long npx)
{
    const size_t plane = (size_t)adaptive_blocks(npx) * 256 * sizeof(unsigned);
    const size_t cbytes = ((size_t)adaptive_blocks(npx) * sizeof(unsigned) + 15) / 16 * 16;
    Layout l;
    l.v = 0;
    l.y = plane;
    l.keep = 2 * plane;
    l.counts = 3 * plane;
    l.n_in = l.counts + cbytes;
    l.list = l.n_in + 16;
    l.count = l.list + plane;
    l.total = l.count + 16;
    return l;
}

int validate_tolerance(float t)
{
    if (!std::isfinite(t)) return fail(RT_EINVAL, "adaptive: tolerance is not finite");
    if (t < 0x1p-12f || t > 1.0f) return fail(RT_EINVAL, "adaptive: tolerance %g outside [2^-12, 1]", (double)t);
    return RT_OK;
}

int validate_adaptive(const rt_adaptive_params* a)
{
    if (!a) return fail(RT_EINVAL, "adaptive: adaptive params is NULL");
    if (a->first_half < 1) return fail(RT_EINVAL, "adaptive: first_half %d < 1", a->first_half);
    if (a->max_rounds < 1 || a->max_rounds > 16)
        return fail(RT_EINVAL, "adaptive: max_rounds %d outside 1..16", a->max_rounds);
    if (((long long)a->first_half << a->max_rounds) > (1ll << 31))   // 2 n_{R-1} = first_half 2^R
        return fail(RT_EINVAL, "adaptive: %d x 2^%d samples per pixel exceed 2^31", a->first_half, a->max_rounds);
    return validate_tolerance(a->tolerance);
}

// What rt_adaptive_async and the host renders (`entry`) refuse alike.  Yields the params of the schedule's
// first batch (the caller's nbRayonParPixel is not read) and the frame's size.
int adaptive_batch(const char* entry, const rt_params* params, const rt_adaptive_params* aparams, rt_params& batch,
                   int& W, int& H)
{
    if (!params) return fail(RT_EINVAL, "params is NULL");
    int rc;
    if ((rc = validate_adaptive(aparams))) return rc;
    batch = *params;
    batch.nbRayonParPixel = aparams->first_half;
    if ((rc = validate_params(&batch))) return rc;
    if (batch.semantics == RT_SEM_CUDA) return fail(RT_EUNSUPPORTED, "%s renders RT_SEM_MAIN_C only", entry);
    W = batch.largeur_image;
    H = batch.hauteur_image;
    return validate_frame_size("adaptive", W, H);
}

AdaptiveSelect select_args(int W, int H, void* workspace)
{
    const Layout l = layout_of((long long)W * H);
    char* ws = (char*)workspace;
    AdaptiveSelect s;
    std::memset(&s, 0, sizeof s);
    s.W = W;
    s.H = H;
    s.npx = (unsigned)W * (unsigned)H;
    s.v = (float*)(ws + l.v);
    s.y = (float*)(ws + l.y);
    s.keep = (unsigned*)(ws + l.keep);
    s.counts = (unsigned*)(ws + l.counts);
    s.n_in = (unsigned*)(ws + l.n_in);
    return s;
}

// rt_last_list_kernel: the render kernel of the calling thread's last list launch.
thread_local const char* t_last_list = "none";

// The reported name of render_kernel_q's list form for the plan's pair: the pair's
// render_kernel_q name (rt_queue_variants.h) with "render_kernel_ql" in front.
const char* list_queue_name(const RenderPlan& plan)
{
    static const std::vector<std::string> names = [] {
        std::vector<std::string> n;
        for (const QueueVariant& v : kQueueVariants) {
            const char* args = std::strchr(v.name, '<');
            n.push_back(std::string("render_kernel_ql") + (args ? args : ""));
        }
        return n;
    }();
    const int i = queue_variant_index(plan.qb, plan.opq);
    return i < 0 ? "none" : names[(size_t)i].c_str();
}

// Every band of a list launch as plan_list (rt_launch_plan.cpp) sizes them (for
// chunks > 1 the scratch holds one band's partials, reused band after band).
int launch_list_on_stream(KParams& kp, const double* uni, const unsigned* d_list, const unsigned* d_count,
                          unsigned list_cap, hipStream_t st)
{
    int rc;
    if ((rc = keep_pool_memory())) return rc;
    // tree, width and sky -- and, with rt_set_accumulate_queue on, whether a render launch of kp takes the
    // queue and with which pair: the list then takes the queue kernel's list form of that pair (chunks > 1: task_ok)
    const RenderPlan plan = plan_render(kp, false);
    const ListPlan bands = plan_list(kp.chunks, list_cap);
    const unsigned band = bands.band;
    const bool queue = plan.queue && bands.partial_bytes != 0;
    t_last_list = queue ? list_queue_name(plan) : plan.wide ? "render_kernel_list_w"
                                              : plan.bvh    ? "render_kernel_list<BVH>"
                                                            : "render_kernel_list";
    LaunchScratch s;
    if ((rc = s.open(kp, uni, plan.stack_cap, bands.partial_bytes, queue, st))) return rc;
    ListArgs la = {d_list, d_count, s.partial, 0u, 0u, band};
    for (unsigned long long e0 = 0; s.e == hipSuccess && e0 < list_cap; e0 += band) {
        la.e0 = (unsigned)e0;
        la.e1 = (unsigned)std::min<unsigned long long>(e0 + band, list_cap);
        s.e = (hipError_t)(queue ? launch_render_list_queue(kp, plan, la, st) : launch_render_list(kp, plan, la, st));
    }
    return s.result("list render");
}

// rt_render_adaptive (filter false: the planes are rt_resolve_adaptive_async's, vparams is not read) and
// rt_render_adaptive_vdenoised (the planes are rt_vdenoise_adaptive_async's) as one HostFrameJob.  `what`
// names the entry point in messages.
int render_adaptive_host(const char* what, const rt_scene* scene, const rt_params* params,
                         const rt_adaptive_params* aparams, const rt_vdenoise_params* vparams, bool filter,
                         rt_color* canva, rt_color* albedo, rt_color* normal, int* rounds)
{
    rt_params batch;
    int rc, W, H;
    if ((rc = validate_scene(scene)) || (rc = adaptive_batch(what, params, aparams, batch, W, H))) return rc;
    if (filter && (rc = validate_vdenoise(W, H, vparams))) return rc;
    if (!canva) return fail(RT_EINVAL, "adaptive: canva is NULL");
    const size_t npx = (size_t)W * H, plane = npx * sizeof(rt_color), sums = npx * 9 * sizeof(double);
    const size_t rbytes = (npx * sizeof(int) + 15) / 16 * 16, aws_bytes = rt_adaptive_workspace_bytes(W, H);
    // the filter runs behind the loop on the same stream: one workspace serves both, the larger one's size
    const size_t vws_bytes = filter ? rt_vdenoise_workspace_bytes(W, H) : 0;
    const size_t ws_bytes = (std::max(aws_bytes, vws_bytes) + 15) / 16 * 16;
    HostFrameJob job;
    if ((rc = job.open("adaptive", scene, 3 * plane + rbytes, 2 * sums + ws_bytes + rbytes + 3 * plane))) return rc;
    double* acc0 = (double*)job.take(2 * sums);           // the two accumulators, back to back
    double* acc1 = (double*)((char*)acc0 + sums);
    char* ws = job.take(ws_bytes);
    int* d_rounds = (int*)job.take(rbytes);
    rt_color* planes = (rt_color*)job.take(3 * plane);
    const rt_frame fr = {planes, albedo ? planes + npx : nullptr, normal ? planes + 2 * npx : nullptr, nullptr};
    if ((rc = rt_adaptive_async(job.scene(), params, aparams, acc0, acc1, d_rounds, ws, aws_bytes,
                                filter ? nullptr : &fr, job.stream())))
        return rc;
    if (filter && (rc = rt_vdenoise_adaptive_async(W, H, acc0, acc1, d_rounds, aparams->first_half, vparams, ws,
                                                   vws_bytes, &fr, job.stream())))
        return rc;
    return job.finish({{canva, planes, plane}, {albedo, planes + npx, plane}, {normal, planes + 2 * npx, plane},
                       {rounds, d_rounds, npx * sizeof(int)}});
}

}  // namespace

extern "C" {

int rt_accumulate_list_async(const rt_device_scene* scene, const rt_params* params, long long sample_offset,
                             const unsigned* d_list, const unsigned* d_count, unsigned list_cap, double* d_sums,
                             void* hip_stream)
{
    if (!scene) return fail(RT_EINVAL, "scene is NULL");
    int rc;
    if ((rc = validate_params(params))) return rc;
    if (params->semantics == RT_SEM_CUDA)
        return fail(RT_EUNSUPPORTED, "rt_accumulate_list_async renders RT_SEM_MAIN_C only");
    if (!d_list || !d_count || !d_sums) return fail(RT_EINVAL, "d_list, d_count or d_sums is NULL");
    const unsigned long long npx = (unsigned long long)params->largeur_image * (unsigned long long)params->hauteur_image;
    if (list_cap == 0 || list_cap > npx)
        return fail(RT_EINVAL, "list_cap %u outside 1..%llu (the frame's pixels)", list_cap, npx);
    if ((rc = validate_sample_window(sample_offset, params->nbRayonParPixel))) return rc;
    const rt_tiling whole = {0, params->hauteur_image, 0, 1, 1};
    KParams kp;
    double uni[U_COUNT];
    fill_kparams(scene, params, &whole, kp, uni);
    kp.sums = d_sums;
    kp.s_base = sample_offset;
    DeviceGuard guard(scene->device);
    return launch_list_on_stream(kp, uni, d_list, d_count, list_cap, (hipStream_t)hip_stream);
}

const char* rt_last_list_kernel(void) { return t_last_list; }

size_t rt_adaptive_workspace_bytes(int W, int H)
{
    if (!frame_size_ok(W, H)) return 0;
    return layout_of((long long)W * H).total;
}

int rt_adaptive_select_async(int W, int H, const double* d_sums_a, const double* d_sums_b, int n_half,
                             float tolerance, int round, unsigned* d_list, unsigned* d_count, int* d_rounds,
                             void* workspace, size_t workspace_bytes, void* hip_stream)
{
    int rc;
    if ((rc = validate_frame_size("adaptive", W, H))) return rc;
    if (!d_sums_a || !d_sums_b) return fail(RT_EINVAL, "adaptive: an accumulator is NULL");
    if (!d_list || !d_count || !d_rounds) return fail(RT_EINVAL, "adaptive: d_list, d_count or d_rounds is NULL");
    if (n_half < 1) return fail(RT_EINVAL, "adaptive: n_half %d < 1", n_half);
    if (round < 0 || round > 15) return fail(RT_EINVAL, "adaptive: round %d outside 0..15", round);
    if ((rc = validate_tolerance(tolerance)) ||
        (rc = validate_workspace("adaptive", W, H, workspace, workspace_bytes, rt_adaptive_workspace_bytes(W, H))))
        return rc;
    AdaptiveSelect s = select_args(W, H, workspace);
    s.all = round == 0;
    s.sums_a = d_sums_a;
    s.sums_b = d_sums_b;
    s.rap = 1.0 / (double)n_half;
    s.tolerance = tolerance;
    s.round = round;
    s.list = d_list;
    s.count = d_count;
    s.rounds = d_rounds;
    const int e = launch_adaptive_select(s, hip_stream);
    if (e) return fail(RT_EDEVICE, "adaptive select launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

void rt_adaptive_params_init(rt_adaptive_params* p)
{
    if (p) *p = kDefaults;
}

int rt_resolve_adaptive_async(int W, int H, const double* d_sums_a, const double* d_sums_b, const int* d_rounds,
                              int first_half, const rt_frame* frame, void* hip_stream)
{
    int rc;
    if ((rc = validate_frame_size("adaptive", W, H))) return rc;
    if (!d_sums_a || !d_sums_b) return fail(RT_EINVAL, "adaptive: an accumulator is NULL");
    if (!d_rounds) return fail(RT_EINVAL, "adaptive: d_rounds is NULL");
    if (first_half < 1) return fail(RT_EINVAL, "adaptive: first_half %d < 1", first_half);
    if (!frame || !frame->canva) return fail(RT_EINVAL, "adaptive: frame.canva is NULL");
    const int e = launch_adaptive_resolve((long long)W * H, d_sums_a, d_sums_b, d_rounds, first_half,
                                          (double*)frame->canva, (double*)frame->albedo, (double*)frame->normal,
                                          (double*)frame->radiance, hip_stream);
    if (e) return fail(RT_EDEVICE, "adaptive resolve launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

int rt_adaptive_async(const rt_device_scene* scene, const rt_params* params, const rt_adaptive_params* aparams,
                      double* d_sums_a, double* d_sums_b, int* d_rounds, void* workspace, size_t workspace_bytes,
                      const rt_frame* frame, void* hip_stream)
{
    if (!scene) return fail(RT_EINVAL, "scene is NULL");
    rt_params batch;                             // nbRayonParPixel is the schedule's, not the caller's
    int rc, W, H;
    if ((rc = adaptive_batch("rt_adaptive_async", params, aparams, batch, W, H))) return rc;
    if (!d_sums_a || !d_sums_b) return fail(RT_EINVAL, "adaptive: an accumulator is NULL");
    if (!d_rounds) return fail(RT_EINVAL, "adaptive: d_rounds is NULL");
    if ((rc = validate_workspace("adaptive", W, H, workspace, workspace_bytes, rt_adaptive_workspace_bytes(W, H))))
        return rc;
    if (frame && !frame->canva) return fail(RT_EINVAL, "adaptive: frame.canva is NULL");

    const hipStream_t st = (hipStream_t)hip_stream;
    const long long npx = (long long)W * H;
    const Layout l = layout_of(npx);
    unsigned* d_list = (unsigned*)((char*)workspace + l.list);
    unsigned* d_count = (unsigned*)((char*)workspace + l.count);
    const rt_tiling whole = {0, H, 0, 1, 1};
    double* acc[2] = {d_sums_a, d_sums_b};
    DeviceGuard guard(scene->device);
    for (int k = 0; k < 2; ++k) HIP_TRY(hipMemsetAsync(acc[k], 0, (size_t)npx * 9 * sizeof(double), st));
    const int R = aparams->max_rounds;
    for (int r = 0; r < R; ++r) {
        // b_r samples to each accumulator from o_r on; n_r per accumulator afterwards
        const long long n_r = (long long)aparams->first_half << r;
        const long long b = r == 0 ? n_r : n_r / 2, o = r == 0 ? 0 : n_r;
        batch.nbRayonParPixel = (int)b;
        for (int k = 0; k < 2; ++k) {
            rc = r == 0 ? rt_accumulate_async(scene, &batch, o + k * b, &whole, acc[k], st)
                        : rt_accumulate_list_async(scene, &batch, o + k * b, d_list, d_count, (unsigned)npx, acc[k], st);
            if (rc) return rc;
        }
        if (r < R - 1) {
            rc = rt_adaptive_select_async(W, H, d_sums_a, d_sums_b, (int)n_r, aparams->tolerance, r, d_list, d_count,
                                          d_rounds, workspace, workspace_bytes, st);
            if (rc) return rc;
        } else {                                 // the last round selects nothing: its pixels' count only
            AdaptiveSelect s = select_args(W, H, workspace);
            s.all = r == 0;
            s.list = d_list;
            s.count = d_count;
            s.rounds = d_rounds;
            const int e = launch_adaptive_mark(s, R, st);
            if (e) return fail(RT_EDEVICE, "adaptive mark launch: %s", hipGetErrorString((hipError_t)e));
        }
    }
    if (frame) return rt_resolve_adaptive_async(W, H, d_sums_a, d_sums_b, d_rounds, aparams->first_half, frame, st);
    return RT_OK;
}

int rt_render_adaptive(const rt_scene* scene, const rt_params* params, const rt_adaptive_params* aparams,
                       rt_color* canva, rt_color* albedo, rt_color* normal, int* rounds)
{
    return render_adaptive_host("rt_render_adaptive", scene, params, aparams, nullptr, false, canva, albedo, normal,
                                rounds);
}

int rt_render_adaptive_vdenoised(const rt_scene* scene, const rt_params* params, const rt_adaptive_params* aparams,
                                 const rt_vdenoise_params* vparams, rt_color* canva, rt_color* albedo,
                                 rt_color* normal, int* rounds)
{
    return render_adaptive_host("rt_render_adaptive_vdenoised", scene, params, aparams, vparams, true, canva, albedo,
                                normal, rounds);
}

}  // extern "C"
