// rt_scene_prep.h — host-only preparation of a caller's rt_scene into the
// arrays and scalars of the HBM layout (rt_internal.h).  No HIP: the C-ABI
// (rt_api.cpp rt_scene_upload) uploads the result, and
// tools/probes/scene_prep_check.cpp tests it on the CPU.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "rt/rt.h"
#include "rt_internal.h"
#include "rt_bvh.h"

namespace rt {

// The scalars of one prepared scene (rt_device_scene carries them as they are;
// fill_kparams, rt_launch_plan.h, turns them into KParams fields and launch gates).
struct SceneFacts {
    int ns = 0, ns_pad = 0, nt = 0, tw = 1, th = 1;
    long long n_texels = 0;
    double cand_lmax = HUGE_VAL;     // KParams::cand_lmax
    int ns_merge = 0;                // leading candidate records that are flagged pairs
    int ns_fwd = 0;                  // ... and the records after them that are forward pairs
    double cbb[6] = {0, 0, 0, 0, 0, 0};   // triangles' box (RT_SEM_CUDA hit_BBox)
    int sky_w = 0, sky_h = 0;
    int bvh_nodes = 0, bvh_depth = 0, bvh_stack4 = 0;
    bool bvh_wide = false;           // BvhBuild::wide: indices beyond 16 bits (32-bit stacks, BvhNodeW, no BvhNodeH)
    double s_rel = 0.0, s_abs = 0.0, r_scene = 0.0, k_delta = 0.0;
    double sph_bound = 0.0;          // max over spheres of max_a |c_a| + |r| (+inf for an infinite one); a NaN
                                     // term (a NaN centre coordinate or radius) is dropped, unlike in coord_max
    float bvh_rbox = 0.0f;           // >= every |bound| of the BVH's boxes
    bool mats_bounded = false;       // every diffuse/emission/strength finite, |x| <= 2^100
    bool sph_opaque = false;         // every sphere material takes main.c's opaque branch (no hole, no refraction)
    bool tri_opaque = false;         // ... every texel too, and no triangle uses material index 3 or 4
    double coord_max = HUGE_VAL;     // max |coordinate| of the spheres (|C_a| + R) and triangle vertices
    bool all_tex0 = false;           // every triangle's uv are 0: its texel is TriTex::tex0
};

// The arrays of one prepared scene: std::vectors on the host (HostScene), and
// what rt_scene_upload copies them into (rt_api_internal.h rt_device_scene; an
// empty one stays a null pointer there).
template <template <class> class Array>
struct SceneArrays {
    Array<SphGeo> sph;               // [ns_pad], the caller's order
    Array<SphCand> sph_cand;         // [ns_pad], candidate-record order (rt_scene_prep.cpp pair_candidates)
    Array<int> cand_orig;            // the sphere index of each candidate record
    Array<SphGeo> sph_slot;          // sph in candidate-record order
    Array<DevMat> sph_mat;
    Array<TriGeo> tri;               // the triangle arrays: leaf order with a BVH
    Array<TriTex> tri_tex;
    Array<TriUV> tri_uv;             // affine texel map per triangle (scenes that are not all uv-less)
    Array<DevMat> texels;
    Array<BvhNode4> bvh;             // 4-wide BVH; empty: no BVH (few triangles)
    Array<BvhNodeH> bvhh;            // the same tree in 64-byte nodes, or empty (does not fit binary16)
    Array<BvhNodeW> bvhw;            // a wide tree (facts.bvh_wide) in its 64-byte nodes, or empty (does not pack)
    Array<int> tri_orig;             // leaf order -> caller's triangle index
    Array<DevMat> sky;               // sky texels (scene->sky_mat_list), or empty
    Array<double> sph_rinv;          // 1/radius per sphere
    Array<double> sph_disp;          // hsl round trip of each sphere's emission
    Array<DevMat> tri_mat;           // rt_triangle.mat per triangle (RT_SEM_CUDA)
};
template <class T>
using HostArray = std::vector<T>;
struct HostScene : SceneArrays<HostArray> {
    SceneFacts facts;
};

// Fills `out` from a scene that passed validation.  RT_OK, or RT_EUNSUPPORTED
// with `err` set (2^31 texels or more; mat_list is then not read).
int prepare_scene(const rt_scene* scene, HostScene& out, std::string& err);

}  // namespace rt
