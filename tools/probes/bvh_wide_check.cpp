// Host check of wide trees (rt_bvh.cpp: build_bvh over more than 65535
// triangles, pack_bvh_w).  For one mesh it reports whether the tree is wide
// and whether its 64-byte nodes (BvhNodeW) packed, and counts
//   child_mismatch  child references and counts decoded from node_base /
//                   tri_base / cnt (the kernel's prefix sums, rt_triangles.h
//                   box4h<true>) that differ from the BvhNode4's,
//   box_fail        decoded binary16 boxes that do not contain the float box
//                   or leave rbox,
//   order_valid     BvhBuild::order is a permutation of 0 .. nt-1 and every
//                   triangle lies in exactly one leaf,
// and replays bvh_step's push rule (every hit internal child but the one
// entered is pushed) with every box hit and for random rays: the peaks must
// stay within stack4.  Input: triangles as 9 doubles per line (A, B, C) on
// stdin; argv[1]: the number of random rays.  Used by tests/test_bvh_wide.py.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rt_bvh.h"
using namespace rt;

static double h2d(unsigned short h)
{
    const int e = (h >> 10) & 0x1f, m = h & 0x3ff;
    const double v = e == 0 ? std::ldexp((double)m, -24) : std::ldexp((double)(m | 0x400), e - 25);
    return (h & 0x8000) ? -v : v;
}

static bool slab(const BvhNode4& n, int c, const double* o, const double* inv)
{
    double t0 = -HUGE_VAL, t1 = HUGE_VAL;
    for (int a = 0; a < 3; ++a) {
        double p = (n.lo[a][c] - o[a]) * inv[a], q = (n.hi[a][c] - o[a]) * inv[a];
        if (p > q) std::swap(p, q);
        t0 = std::fmax(t0, p);
        t1 = std::fmin(t1, q);
    }
    return t0 <= t1 && t1 >= 0.0;
}

// max stack size of the walk; hit(node, child) decides the child boxes
template <class HIT>
static int walk(const std::vector<BvhNode4>& N, HIT hit, bool last = false)
{
    std::vector<int> stk;
    int node = 0, peak = 0;
    for (;;) {
        int next = -1;
        for (int c = 0; c < 4; ++c) {
            if (N[(size_t)node].count[c] != 0 || !hit(node, c)) continue;
            if (next < 0) next = N[(size_t)node].child[c];
            else if (last) {
                stk.push_back(next);
                next = N[(size_t)node].child[c];
            } else stk.push_back(N[(size_t)node].child[c]);
        }
        peak = std::max(peak, (int)stk.size());
        if (next >= 0) {
            node = next;
            continue;
        }
        if (stk.empty()) break;
        node = stk.back();
        stk.pop_back();
    }
    return peak;
}

int main(int argc, char** argv)
{
    const int nrays = argc > 1 ? std::atoi(argv[1]) : 0;
    std::vector<TriGeo> tri;
    double v[9], r = 0.0;
    while (std::scanf("%lf %lf %lf %lf %lf %lf %lf %lf %lf", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8) == 9) {
        TriGeo g;
        g.ax = v[0]; g.ay = v[1]; g.az = v[2];
        g.abx = v[3] - v[0]; g.aby = v[4] - v[1]; g.abz = v[5] - v[2];
        g.acx = v[6] - v[0]; g.acy = v[7] - v[1]; g.acz = v[8] - v[2];
        g.nx = g.aby * g.acz - g.abz * g.acy; g.ny = g.abz * g.acx - g.abx * g.acz; g.nz = g.abx * g.acy - g.aby * g.acx;
        tri.push_back(g);
        for (double x : v) r = std::fmax(r, std::fabs(x));
    }
    const int nt = (int)tri.size();
    BvhBuild b;
    const auto t0 = std::chrono::steady_clock::now();
    const bool built = build_bvh(tri.data(), nt, r, b);
    const double build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!built) {
        std::printf("{\"nt\": %d, \"bvh\": false}\n", nt);
        return 0;
    }
    const std::vector<BvhNode4>& N = b.nodes4;
    // order: a permutation, and the leaves tile [0, nt)
    bool order_valid = (int)b.order.size() == nt;
    {
        std::vector<char> seen((size_t)nt, 0);
        for (int k : b.order) {
            if (k < 0 || k >= nt || seen[(size_t)k]) order_valid = false;
            else seen[(size_t)k] = 1;
        }
        std::vector<char> cov((size_t)nt, 0);
        for (const BvhNode4& n : N)
            for (int c = 0; c < 4; ++c)
                for (int j = 0; j < std::max(0, n.count[c]); ++j) {
                    const long k = (long)n.child[c] + j;
                    if (k < 0 || k >= nt || cov[(size_t)k]) order_valid = false;
                    else cov[(size_t)k] = 1;
                }
        for (char x : cov) order_valid = order_valid && x;
    }
    std::vector<BvhNodeW> w;
    float rbox = 0;
    const bool packed = b.wide && pack_bvh_w(N, w, rbox);
    long child_mismatch = 0, box_fail = 0;
    long max_internal = -1, max_tri = -1;
    if (packed)
        for (size_t i = 0; i < w.size(); ++i) {
            unsigned nn = w[i].node_base, kk = w[i].tri_base;     // box4h<true>'s prefix sums
            for (int c = 0; c < 4; ++c) {
                const unsigned nib = (w[i].cnt >> (4 * c)) & 15u;
                const int cnt = nib == 15u ? -1 : (int)nib;
                const long ch = nib == 0u ? (long)nn : (long)kk;
                nn += nib == 0u ? 1u : 0u;
                kk += nib == 15u || nib == 0u ? 0u : nib;
                if (cnt != N[i].count[c]) ++child_mismatch;
                if (cnt < 0) continue;
                if (ch != (long)N[i].child[c]) ++child_mismatch;
                if (cnt == 0) max_internal = std::max(max_internal, ch);
                else max_tri = std::max(max_tri, ch + cnt - 1);
                for (int a = 0; a < 3; ++a) {
                    const double lo = h2d(w[i].org[a]) + h2d(w[i].plo[a][c]), hi = h2d(w[i].org[a]) + h2d(w[i].phi[a][c]);
                    if (!(lo <= N[i].lo[a][c]) || !(hi >= N[i].hi[a][c])) ++box_fail;
                    if (!(std::fabs(lo) <= rbox && std::fabs(hi) <= rbox)) ++box_fail;
                }
            }
        }
    const int all = std::max(walk(N, [](int, int) { return true; }), walk(N, [](int, int) { return true; }, true));
    int rays = 0;
    std::srand(12345);
    const auto u = [] { return std::rand() / (double)RAND_MAX * 2.0 - 1.0; };
    for (int k = 0; k < nrays; ++k) {
        double o[3] = {u() * r, u() * r, u() * r}, d[3] = {u(), u(), u()}, inv[3];
        for (int a = 0; a < 3; ++a) inv[a] = 1.0 / d[a];
        rays = std::max(rays, walk(N, [&](int n, int c) { return slab(N[(size_t)n], c, o, inv); }));
    }
    std::printf("{\"nt\": %d, \"bvh\": true, \"nodes\": %zu, \"depth4\": %d, \"stack4\": %d, \"wide\": %s, \"packed\": %s, "
                "\"child_mismatch\": %ld, \"box_fail\": %ld, \"order_valid\": %s, \"max_internal_child\": %ld, "
                "\"max_leaf_triangle\": %ld, \"all_hit_peak\": %d, \"ray_peak\": %d, \"build_s\": %.3f}\n",
                nt, N.size(), b.depth4, b.stack4, b.wide ? "true" : "false", packed ? "true" : "false", child_mismatch,
                box_fail, order_valid ? "true" : "false", max_internal, max_tri, all, rays, build_s);
    return 0;
}
