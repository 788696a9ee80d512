// rt_queue_variants.h — the (QB, OPQ) instantiations of render_kernel_q
// (rt_queue.h), described once for the host and the device.  No HIP:
// plan_render (rt_launch_plan.cpp) takes a plan's stack and name from here,
// rt_kernels.hip dispatches over the list, and the device code builds its
// stacks (rt_triangles.h bvh_stack_for_q) and the kernel's compile-time
// constants (rt_queue.h QVariant) on the same entries.
#pragma once
#include "rt_bvh.h"

namespace rt {

// The kernel's template parameter QB began as "node visits per round" and is
// now the tag of a kernel family (the values are part of the kernel symbols):
enum : int {
    QB_SPH_OPAQUE = -2,   // sphere-only scene, every material opaque
    QB_SPH = -1,          // sphere-only scene
    QB_SCAN = 0,          // few triangles, brute-force scan
    QB_DEEP = 3,          // deep tree over the 64-byte nodes BvhNodeH
    QB_TOP = 4,           // shallow tree, 128-byte nodes with the top ones in LDS; the one value that
                          // still is the visit count: 4 per round
    QB_WIDE = 5,          // wide tree (rt_bvh.h BvhBuild::wide) over the 64-byte nodes BvhNodeW
};

// The node form a kernel walks (bvh_visit's H), QN_NONE: no BVH.
enum : int { QN_NONE = -1, QN_128 = 0, QN_H = 1, QN_W = 2 };

struct QueueVariant {
    int qb;
    bool opq;             // (BVH scenes) the every-material-opaque form of qb
    const char* name;     // as rt_last_render_kernel() reports it (tests and bench.py read it)
    bool triangles;       // the scene has triangles
    bool opaque;          // every material is opaque: no alpha hole, no refraction branch
    int nodes;            // QN_*
    int stack;            // BVH stack entries per lane (rt_bvh.h kStackQ*), 0 without a BVH
    bool stack24;         // ... of 24 bits, split into a uint16 and a uint8 column (else uint16)
    bool far;             // the walk has the far-origin margins (rt_triangles.h ray32)
};

// Every legal pair.  Who is admitted where is plan_render's rule.  (The order is
// the one rt_kernels.hip instantiates, and so emits, the kernels in.)
inline constexpr QueueVariant kQueueVariants[] = {
    {QB_DEEP, true, "render_kernel_q<QB=3,OP>", true, true, QN_H, kStackQ, false, false},
    {QB_DEEP, false, "render_kernel_q<QB=3>", true, false, QN_H, kStackQN, false, true},
    {QB_TOP, false, "render_kernel_q<QB=4>", true, false, QN_128, kStackQ4, false, false},
    {QB_WIDE, false, "render_kernel_q<QB=5>", true, false, QN_W, kStackQW, true, true},
    {QB_SPH_OPAQUE, false, "render_kernel_q<QB=-2>", false, true, QN_NONE, 0, false, false},
    {QB_SPH, false, "render_kernel_q<QB=-1>", false, false, QN_NONE, 0, false, false},
    {QB_SCAN, false, "render_kernel_q<QB=0>", true, false, QN_NONE, 0, false, false},
};
constexpr int kQueueVariantCount = (int)(sizeof kQueueVariants / sizeof kQueueVariants[0]);

// The pair's place in the list, -1 when it is not a legal pair.
constexpr int queue_variant_index(int qb, bool opq)
{
    for (int i = 0; i < kQueueVariantCount; ++i)
        if (kQueueVariants[i].qb == qb && kQueueVariants[i].opq == opq) return i;
    return -1;
}
// The entry of a legal pair (in a constant expression, any other pair fails to compile).
constexpr const QueueVariant& queue_variant(int qb, bool opq) { return kQueueVariants[queue_variant_index(qb, opq)]; }

// The list against rt_bvh.h: a named entry per pair, no pair twice, and the
// stack of each family -- the host's stack_cap and the device's array length are
// both QueueVariant::stack, and the kernels never check their stack pointer.
constexpr int queue_family_stack(const QueueVariant& v)
{
    return v.nodes == QN_NONE  ? 0
           : v.nodes == QN_128 ? kStackQ4
           : v.nodes == QN_W   ? kStackQW
                               : v.opaque ? kStackQ : kStackQN;
}
template <class P>
constexpr bool every_queue_variant(P holds)
{
    for (int i = 0; i < kQueueVariantCount; ++i)
        if (!holds(kQueueVariants[i], i)) return false;
    return true;
}
static_assert(every_queue_variant([](const QueueVariant& v, int) { return v.name != nullptr && v.name[0] != '\0'; }),
              "kQueueVariants: a pair without a name");
static_assert(every_queue_variant([](const QueueVariant& v, int i) { return queue_variant_index(v.qb, v.opq) == i; }),
              "kQueueVariants: a pair listed twice");
static_assert(every_queue_variant([](const QueueVariant& v, int) {
                  return v.stack == queue_family_stack(v) && v.stack24 == (v.nodes == QN_W) &&
                         (v.triangles || v.nodes == QN_NONE);
              }),
              "kQueueVariants: a stack that is not its family's");

}  // namespace rt
