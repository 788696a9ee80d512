// rt_denoise_tile.h — what the two denoisers' pass kernels (rt_denoise.hip,
// rt_vdenoise.hip) share: float3 plane access, rt.h's d2, and the geometry of
// the tiled pass (one wave per 64-pixel row segment, kTileY rows per block,
// the rows of one residue class of the step staged in LDS).
#pragma once
#include <hip/hip_runtime.h>

namespace rt {

namespace {

struct F3 { float x, y, z; };

__device__ __forceinline__ F3 ld3(const float* __restrict__ p, long long px)
{
    const float* q = p + px * 3;
    return F3{q[0], q[1], q[2]};
}

// d2(X) = (d0*d0 + d1*d1) + d2*d2, d = X[q] - X[p]
__device__ __forceinline__ float dist2(const F3 q, const F3 p)
{
    const float d0 = q.x - p.x, d1 = q.y - p.y, d2 = q.z - p.z;
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// (0.25f*(D0*D0) + 0.5f*(D1*D1)) + 0.25f*(D2*D2): rt.h's luminance-weighted square
// (the variance-guided denoiser's v and dl; adaptive sampling's v, rt_adaptive.hip)
__device__ __forceinline__ float lum2(const float d0, const float d1, const float d2)
{
    return (0.25f * (d0 * d0) + 0.5f * (d1 * d1)) + 0.25f * (d2 * d2);
}

constexpr int kTileX = 64;          // pixels of one row a wave filters: every tap row is one coalesced run
constexpr int kTileY = 4;           // rows (waves) per block
constexpr int kTiledRows = kTileY + 4;   // rows a tiled block stages: its own and two tap rows either side

}  // namespace

}  // namespace rt
