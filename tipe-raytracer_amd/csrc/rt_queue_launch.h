// rt_queue_launch.h — host side of a task-queue launch, shared by the two files
// that instantiate render_kernel_q: rt_kernels.hip (the dense form) and
// rt_queue_list.hip (the list form).  Included after rt_queue.h.
#pragma once
#include <atomic>
#include <cstdio>
#include <cstdlib>

namespace rt {

// The 28 instantiations of a queue kernel: rt_queue_variants.h's (QB, OPQ) pairs
// x sky x AO.  with_queue_variant maps the plan's tuple to its QVariant
// (rt_queue.h) and hands it to f, so the kernel pointer and its occupancy cache
// cannot disagree; false (f not called) when the pair is not in the list.  (A
// row's kernels are named before the next row is looked at: the code object
// holds the kernels in the table's order.)
template <int QB, bool OPQ, class F>
static void with_queue_variant_qb(const RenderPlan& pl, F&& f)
{
    if (pl.sky && pl.ao) f(QVariant<true, AO_ON, QB, OPQ>{});
    else if (pl.sky) f(QVariant<true, AO_OFF, QB, OPQ>{});
    else if (pl.ao) f(QVariant<false, AO_ON, QB, OPQ>{});
    else f(QVariant<false, AO_OFF, QB, OPQ>{});
}
template <int I = 0, class F>
static bool with_queue_variant(const RenderPlan& pl, F&& f)
{
    if constexpr (I < kQueueVariantCount) {
        constexpr QueueVariant v = kQueueVariants[I];
        if (pl.qb == v.qb && pl.opq == v.opq) {
            with_queue_variant_qb<v.qb, v.opq>(pl, f);
            return true;
        }
        return with_queue_variant<I + 1>(pl, f);
    } else {
        return false;
    }
}

// Variant V's render_kernel_q with the arguments TAIL behind KParams: none (the
// dense form) or ListArgs (the list form).
template <class... TAIL>
using QueueKernel = void (*)(const KParams, const TAIL...);
template <class... TAIL, class V>
constexpr QueueKernel<TAIL...> queue_kernel(V) { return render_kernel_q<V::SKY, V::AOM, V::QB, V::OPQ, TAIL...>; }

// Resident blocks of variant V's queue kernel `kernel` on this device: the grid
// of its launches.  Cached per device, variant and kernel type (one table per
// instantiation of this function); rt_fill_canva may run on several host
// threads at once (main.c's pthreads), so the cache is atomic (every thread
// computes the same value).  `what` names the kernel for RT_QUEUE_VERBOSE.
template <class V, class Kernel>
static unsigned queue_grid(V, Kernel kernel, const char* what)
{
    static std::atomic<int> cached[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::atomic<int>& slot = cached[dev & 63];
    int c = slot.load(std::memory_order_relaxed);
    if (c <= 0) {
        int nb = 0, ncu = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 256, 0);
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
        c = std::max(1, nb) * std::max(1, ncu);
        if (std::getenv("RT_QUEUE_VERBOSE")) std::fprintf(stderr, "%s: %d blocks/CU x %d CUs -> %d\n", what, nb, ncu, c);
        slot.store(c, std::memory_order_relaxed);
    }
    // RT_QUEUE_BLOCKS (tests, experiments) is read on every launch, so a test
    // can shrink the grid to a few blocks and give every lane hundreds of tasks.
    if (const char* e = std::getenv("RT_QUEUE_BLOCKS")) c = std::max(1, std::atoi(e));
    return (unsigned)c;
}

// floor((2^32 - 1) / d) for udiv_q
static inline unsigned qdiv_magic(unsigned d) { return d ? (unsigned)(0xffffffffull / d) : 0u; }

// The launch constants of KParams that both queue kernels' task decoders read.
static inline void set_queue_magics(KParams& k)
{
    k.qm_w = qdiv_magic((unsigned)k.W);
    // chunk starts c*S/P in 32 bits when (P + 1) * S fits
    k.qm_chunks = (unsigned long long)(k.chunk_den + 1) * (unsigned long long)k.S < (1ull << 32)
                      ? qdiv_magic(k.chunk_den) : 0u;
}

}  // namespace rt
