// A scene as text on stdin, shared by the host checkers scene_prep_check.cpp and
// launch_plan_check.cpp.  Whitespace-separated, numbers as strtod reads them
// (inf, nan, hex):
//   spheres N            then N x: cx cy cz radius MAT
//   triangles N tw th nm then N x: A(3) B(3) C(3) uvA(2) uvB(2) uvC(2) quelMat MAT
//   texels K             then K x MAT (K may be short of nm*th*tw only when
//                        that product is refused)
//   sky w h              then w*h x MAT
// MAT: diffuse(3) emission(3) emissionStrength reflectionStrength alpha materialIndex.
// Sections may be absent.
#pragma once
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "rt/rt.h"

static std::vector<std::string> g_tok;
static size_t g_pos = 0;

static void read_tokens()
{
    std::string all;
    char buf[1 << 16];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, stdin)) > 0;) all.append(buf, n);
    for (size_t i = 0; i < all.size();) {
        while (i < all.size() && std::isspace((unsigned char)all[i])) ++i;
        size_t j = i;
        while (j < all.size() && !std::isspace((unsigned char)all[j])) ++j;
        if (j > i) g_tok.emplace_back(all, i, j - i);
        i = j;
    }
}
static const char* next()
{
    if (g_pos >= g_tok.size()) {
        std::fprintf(stderr, "scene text: input ends early\n");
        std::exit(2);
    }
    return g_tok[g_pos++].c_str();
}
static double num() { return std::strtod(next(), nullptr); }
static int inum() { return (int)std::strtol(next(), nullptr, 10); }
static rt_material mat()
{
    rt_material m;
    for (int a = 0; a < 3; ++a) m.diffuseColor.e[a] = num();
    for (int a = 0; a < 3; ++a) m.emissionColor.e[a] = num();
    m.emissionStrength = num();
    m.reflectionStrength = num();
    m.alpha = num();
    m.materialIndex = num();
    return m;
}

// The caller's rt_scene and the arrays it points into.
struct SceneText {
    std::vector<rt_sphere> sph;
    std::vector<rt_triangle> tri;
    std::vector<int> quel;
    std::vector<rt_material> texels, sky;
    rt_scene sc;

    // Reads scene sections up to the end of the input or to a section it does
    // not know, whose name it returns ("" at the end).  Exits when the texel
    // table is short (a table prepare_scene refuses is never read: it may be).
    std::string read()
    {
        std::memset(&sc, 0, sizeof sc);
        std::string what;
        while (g_pos < g_tok.size()) {
            what = next();
            if (what == "spheres") {
                sph.resize((size_t)inum());
                for (rt_sphere& s : sph) {
                    for (int a = 0; a < 3; ++a) s.center.e[a] = num();
                    s.radius = num();
                    s.mat = mat();
                }
            } else if (what == "triangles") {
                tri.resize((size_t)inum());
                sc.tex_width = inum();
                sc.tex_height = inum();
                sc.nbMaterials = inum();
                for (rt_triangle& t : tri) {
                    for (int a = 0; a < 3; ++a) t.A.e[a] = num();
                    for (int a = 0; a < 3; ++a) t.B.e[a] = num();
                    for (int a = 0; a < 3; ++a) t.C.e[a] = num();
                    t.uvA.u = num();
                    t.uvA.v = num();
                    t.uvB.u = num();
                    t.uvB.v = num();
                    t.uvC.u = num();
                    t.uvC.v = num();
                    quel.push_back(inum());
                    t.mat = mat();
                }
            } else if (what == "texels") {
                texels.resize((size_t)inum());
                for (rt_material& m : texels) m = mat();
            } else if (what == "sky") {
                sc.sky_width = inum();
                sc.sky_height = inum();
                sky.resize((size_t)sc.sky_width * (size_t)sc.sky_height);
                for (rt_material& m : sky) m = mat();
            } else {
                break;
            }
            what.clear();
        }
        sc.sphere_list = sph.data();
        sc.nbSpheres = (int)sph.size();
        sc.triangle_list = tri.data();
        sc.nbTriangles = (int)tri.size();
        sc.quelMatPourTri = quel.data();
        sc.mat_list = texels.data();
        sc.sky_mat_list = sky.empty() ? nullptr : sky.data();
        const long long need = (long long)sc.nbMaterials * sc.tex_width * sc.tex_height;
        if (sc.nbTriangles > 0 && need < (1LL << 31) && (long long)texels.size() < need) {
            std::fprintf(stderr, "scene text: %zu texels given, %lld needed\n", texels.size(), need);
            std::exit(2);
        }
        return what;
    }
};
