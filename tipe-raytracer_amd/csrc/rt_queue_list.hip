// rt_queue_list.hip — the list form of the task-queue kernel: render_kernel_q
// (rt_queue.h) over a compacted list of pixels (rt_accumulate_list_async with
// rt_set_accumulate_queue on), reported as "render_kernel_ql<...>": its
// instantiations, its prologue kernel and its launcher.
//
// A band [e0, e1) of a list launch holds n = min(*count, e1) - e0 entries and
// n * P tasks, chunk-major (the tapered short slices come last): task t is
// slice t / n of entry e0 + t % n, and its partial goes to index
// (t / n) * stride + t % n of the band's partials -- the layout
// combine_list_kernel (rt_adaptive.hip) reads, which runs behind this kernel
// unchanged.  The count is a device word that the host never reads, so n, n * P
// and the division magic floor((2^32 - 1) / n) come from a one-wave prologue
// kernel, which also zeroes the task counter; the render kernel reads the three
// words through the scalar unit where a batch of tasks is decoded
// (rt_queue.h decode_list_task).  With n = 0 every lane finds "past the last
// task" on its first grab and the grid drains.
//
// The kernel is render_kernel_q itself with ListArgs as its tail argument.  A
// translation unit of its own: the kernels of rt_kernels.hip and
// rt_adaptive.hip keep theirs.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "rt/rt.h"
#include "rt_internal.h"
#include "rt_bvh.h"
#include "rt_launch_plan.h"
#include "rt_device_math.h"
#include "rt_tunables.h"

#include "rt_vec.h"
#include "rt_spheres.h"
#include "rt_triangles.h"
#include "rt_shading.h"
#include "rt_fixed_grid.h"
#include "rt_queue.h"
#include "rt_queue_launch.h"

namespace rt {

// One wave; its first lane writes.  n <= band and band * chunks < 2^31 (plan_list).
__global__ __launch_bounds__(64) void list_tasks_kernel(const ListArgs la, unsigned chunks, unsigned* __restrict__ ctr)
{
    if (threadIdx.x != 0) return;
    const unsigned end = min(*la.count, la.e1);
    const unsigned n = end > la.e0 ? end - la.e0 : 0u;
    unsigned* w = ctr + kListTaskOffset;
    ctr[0] = 0u;
    w[LT_TASKS] = n * chunks;
    w[LT_ENTRIES] = n;
    w[LT_MAGIC] = n ? 0xffffffffu / n : 0u;
}

// One entry band [la.e0, la.e1) on the queue kernel of the plan's variant: the
// prologue, the resident grid, the combine.
int launch_render_list_queue(const KParams& kp, const RenderPlan& pl, const ListArgs& la, void* stream)
{
    const hipStream_t st = (hipStream_t)stream;
    QueueKernel<ListArgs> kernel = nullptr;
    unsigned nb = 0;
    const bool listed = pl.queue && with_queue_variant(pl, [&](auto v) {
        kernel = queue_kernel<ListArgs>(v);
        nb = queue_grid(v, kernel, "render_kernel_ql");
    });
    if (!listed || !kp.task_ctr || kp.chunks <= 1 || !la.partial) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(list_tasks_kernel, dim3(1), dim3(64), 0, st, la, (unsigned)kp.chunks, kp.task_ctr);
    KParams k2 = kp;
    k2.partial = la.partial;
    k2.trace = nullptr;
    set_queue_magics(k2);
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, st, k2, la);
    return launch_combine_list(kp, la, stream);
}

}  // namespace rt
