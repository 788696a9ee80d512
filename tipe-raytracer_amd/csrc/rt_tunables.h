// rt_tunables.h — the build-time tunables and diagnostic switches of the render
// kernels' device headers (rt_vec.h .. rt_queue.h).  Included before them by
// every translation unit that instantiates render kernels: rt_kernels.hip and
// rt_adaptive.hip.
#pragma once

// ---- Build-time tunables (numeric; a tuning run varies these) ----------
// Candidate-pass grazing threshold T1 = RT_CAND_T1 * Hs^2 and half-width
// M = RT_CAND_M * Hs (spheres_closest); M must exceed 2^-47.2 / sqrt(RT_CAND_T1)
// by a wide factor (static_assert below).
#ifndef RT_CAND_T1
#define RT_CAND_T1 0x1p-36
#endif
#ifndef RT_CAND_M
#define RT_CAND_M 0x1p-26
#endif
static_assert(RT_CAND_M * RT_CAND_M * RT_CAND_T1 >= 0x1.8p-89 && RT_CAND_M <= 0x1p-20,
              "candidate half-width M must be >= 8 x the sqrt error bound 2^-47.2/sqrt(T1)");
// Forward pairs' liveness certificate (spheres_closest): a sphere is dead for a
// lane with h > 2^-RT_FWD_HEXP Hs and ca > -2^-RT_FWD_CEXP Hs^2.
#define RT_FWD_HEXP 16
#define RT_FWD_CEXP 44
// Occupancy bounds (waves per SIMD): the fixed-grid kernels, the fixed-grid
// BVH variant (traversal state + LDS stack), and the queue kernel with its
// shallow-tree and sphere-only instantiations (rt_queue.h QVariant::WAVES).
#ifndef RT_WAVES_PER_SIMD
#define RT_WAVES_PER_SIMD 4
#endif
#ifndef RT_WAVES_PER_SIMD_BVH
#define RT_WAVES_PER_SIMD_BVH 3
#endif
#ifndef RT_WAVES_PER_SIMD_Q
#define RT_WAVES_PER_SIMD_Q RT_WAVES_PER_SIMD
#endif
#ifndef RT_WAVES_PER_SIMD_Q4
#define RT_WAVES_PER_SIMD_Q4 RT_WAVES_PER_SIMD_Q
#endif
#ifndef RT_WAVES_PER_SIMD_QW        // QB_WIDE (wide trees): 46 KiB of LDS, three blocks per CU
#define RT_WAVES_PER_SIMD_QW 3
#endif
#ifndef RT_WAVES_PER_SIMD_QS
#define RT_WAVES_PER_SIMD_QS RT_WAVES_PER_SIMD_Q
#endif
#define RT_BVH_COOP 1               // fixed-grid BVH kernel: wave-cooperative deep traversal once this
                                    // many lanes wait for it (samples_coop)
#define RT_FLAT_FILL 2              // fixed-grid sphere kernel: camera rays start once this many eighths
                                    // of the live lanes wait (samples_flat)
#ifndef RT_WALK_PRIO                // BVH queue kernel: wave priority during its walk steps (0: off).  The walk
#define RT_WALK_PRIO 2              // is a chain of dependent node/record loads; ahead of the other waves'
#endif                              // VALU it issues sooner
#ifndef RT_QB_TOP                   // QB_TOP: nodes of the tree's top levels copied to LDS (x 128 B; the block
#define RT_QB_TOP 40                // then needs <= 40 KiB of LDS, still 4 blocks per CU)
#endif
// node visits per round of the deep-tree instantiations (QB_DEEP, QB_WIDE): RT_QW_MIN,
// then more while >= RT_QW_LANES lanes still walk, at most RT_QW_MAX
#ifndef RT_QW_MIN
#define RT_QW_MIN 3
#endif
#ifndef RT_QW_MAX
#define RT_QW_MAX 12
#endif
#ifndef RT_QW_LANES
#define RT_QW_LANES 32
#endif
// ---- Diagnostic builds --------------------------------------------------
#ifndef RT_PHASE_CLOCK              // tools/phase_clock.py: render_kernel_q adds the wave's s_memtime
#define RT_PHASE_CLOCK 0            // cycles per round phase to its RT_QUEUE_TRACE record
#endif
// RT_QUEUE_TRACE words per lane: start, end, rounds, tasks (+ RT_PHASE_CLOCK:
// cycles in the sphere cast, the BVH walk, resolve, the task hand-out, and
// the next-ray step with finish_bounce)
#define RT_TRACE_WORDS (RT_PHASE_CLOCK ? 9 : 4)
#ifndef RT_DIAG_STALE               // tools/probes/stale_visits.py: COUNT walks count visits to nodes whose
#define RT_DIAG_STALE 0             // entry distance already exceeds the cull distance (in the stack-over
#endif                              // slot; stack entries below depth 16 only)
#ifndef RT_DIAG_MERGE               // tools/merge_share.py: render_kernel_q's RT_QUEUE_TRACE record carries the
#define RT_DIAG_MERGE 0             // wave's flagged sphere pairs that ran one root tail / two (spheres_closest)
#endif                              // in place of rounds and tasks, and the same of its forward pairs in
                                    // place of the two clocks
