// Host check of prepare_scene (rt_scene_prep.cpp): reads a scene as text on
// stdin, prepares it and prints one JSON line with the SceneFacts fields and,
// per array, its element count, a 64-bit FNV-1a hash of its bytes and (up to
// argv[1] elements, default 64; never for the BVH nodes) its contents.
// Input: the scene sections of scene_text.h (spheres, triangles, texels, sky).
// A refusal prints {"rc": code, "error": text}.
// Used by tests/test_scene_prep.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rt_scene_prep.h"
#include "scene_text.h"
using namespace rt;

static void put_double(double x)
{
    if (std::isnan(x)) std::printf("NaN");
    else if (std::isinf(x)) std::printf(x < 0 ? "-Infinity" : "Infinity");
    else std::printf("%.17g", x);
}

static unsigned long long g_bits = 1469598103934665603ull;       // FNV-1a over the scalars' bytes, field by field
static void fnv(unsigned long long& h, const void* p, size_t n)
{
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
}
static void fact(const char* name, double x)
{
    fnv(g_bits, &x, sizeof x);
    std::printf("\"%s\": ", name);
    put_double(x);
    std::printf(", ");
}
static void fact(const char* name, long long x)
{
    fnv(g_bits, &x, sizeof x);
    std::printf("\"%s\": %lld, ", name, x);
}
static void fact(const char* name, int x) { fact(name, (long long)x); }
static void fact(const char* name, bool x)
{
    fnv(g_bits, &x, sizeof x);
    std::printf("\"%s\": %s, ", name, x ? "true" : "false");
}

static size_t g_limit = 64;

// one record as numbers: nd doubles, or (TriTex) 12 doubles, 2 ints, 4 doubles
static void put_record(const unsigned char* p, size_t size, bool tritex)
{
    std::printf("[");
    for (size_t off = 0, k = 0; off < size; ++k) {
        if (k) std::printf(", ");
        if (tritex && (k == 12 || k == 13)) {
            int v;
            std::memcpy(&v, p + off, sizeof v);
            std::printf("%d", v);
            off += sizeof v;
        } else {
            double v;
            std::memcpy(&v, p + off, sizeof v);
            put_double(v);
            off += sizeof v;
        }
    }
    std::printf("]");
}

template <class T>
static void array(const char* name, const std::vector<T>& v, int kind)      // kind 0: doubles, 1: TriTex, 2: int, 3: no contents
{
    unsigned long long h = 1469598103934665603ull;
    fnv(h, v.data(), v.size() * sizeof(T));
    std::printf("\"%s\": {\"n\": %zu, \"hash\": \"%016llx\"", name, v.size(), h);
    if (kind != 3 && v.size() <= g_limit) {
        std::printf(", \"data\": [");
        for (size_t i = 0; i < v.size(); ++i) {
            if (i) std::printf(", ");
            if (kind == 2) std::printf("%d", *(const int*)&v[i]);
            else put_record((const unsigned char*)&v[i], sizeof(T), kind == 1);
        }
        std::printf("]");
    }
    std::printf("}, ");
}

int main(int argc, char** argv)
{
    if (argc > 1) g_limit = (size_t)std::strtoull(argv[1], nullptr, 10);
    read_tokens();
    SceneText st;
    const std::string unknown = st.read();
    if (!unknown.empty()) {
        std::fprintf(stderr, "scene_prep_check: unknown section %s\n", unknown.c_str());
        return 2;
    }
    const rt_scene& sc = st.sc;

    HostScene hs;
    std::string err;
    const int rc = prepare_scene(&sc, hs, err);
    if (rc != RT_OK) {
        std::printf("{\"rc\": %d, \"error\": \"%s\"}\n", rc, err.c_str());
        return 0;
    }
    const SceneFacts& f = hs.facts;
    std::printf("{\"rc\": 0, ");
    fact("ns", f.ns);
    fact("ns_pad", f.ns_pad);
    fact("nt", f.nt);
    fact("tw", f.tw);
    fact("th", f.th);
    fact("n_texels", f.n_texels);
    fact("cand_lmax", f.cand_lmax);
    fact("ns_merge", f.ns_merge);
    fact("ns_fwd", f.ns_fwd);
    for (int i = 0; i < 6; ++i) fact(("cbb" + std::to_string(i)).c_str(), f.cbb[i]);
    fact("sky_w", f.sky_w);
    fact("sky_h", f.sky_h);
    fact("bvh_nodes", f.bvh_nodes);
    fact("bvh_depth", f.bvh_depth);
    fact("bvh_stack4", f.bvh_stack4);
    fact("s_rel", f.s_rel);
    fact("s_abs", f.s_abs);
    fact("r_scene", f.r_scene);
    fact("k_delta", f.k_delta);
    fact("sph_bound", f.sph_bound);
    fact("bvh_rbox", (double)f.bvh_rbox);
    fact("mats_bounded", f.mats_bounded);
    fact("sph_opaque", f.sph_opaque);
    fact("tri_opaque", f.tri_opaque);
    fact("coord_max", f.coord_max);
    fact("all_tex0", f.all_tex0);
    array("sph", hs.sph, 0);
    array("sph_cand", hs.sph_cand, 0);
    array("cand_orig", hs.cand_orig, 2);
    array("sph_slot", hs.sph_slot, 0);
    array("sph_mat", hs.sph_mat, 0);
    array("tri", hs.tri, 0);
    array("tri_tex", hs.tri_tex, 1);
    array("tri_uv", hs.tri_uv, 0);
    array("texels", hs.texels, 0);
    array("bvh", hs.bvh, 3);
    array("bvhh", hs.bvhh, 3);
    array("tri_orig", hs.tri_orig, 2);
    array("sky", hs.sky, 0);
    array("sph_rinv", hs.sph_rinv, 0);
    array("sph_disp", hs.sph_disp, 0);
    array("tri_mat", hs.tri_mat, 0);
    std::printf("\"facts_bits\": \"%016llx\"}\n", g_bits);
    return 0;
}
