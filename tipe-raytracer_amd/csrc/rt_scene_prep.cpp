// rt_scene_prep.cpp — a caller's rt_scene into the HBM layout's arrays and
// scalars (rt_scene_prep.h), on the host alone: candidate records and their
// pairing order, per-triangle precomputation, the BVH reorder, the texel
// tables and the bounds and flags the launch gates read.
#include "rt_scene_prep.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace rt {
namespace {

// The shading fields a zero rayColor multiplies (LanePath::zero_rc).
bool shading_bounded(const DevMat& m, double lim = 0x1p100)
{
    const double v[7] = {m.dr, m.dg, m.db, m.er, m.eg, m.eb, m.es};
    for (double x : v)
        if (!(std::fabs(x) <= lim)) return false;
    return true;
}

// rgb_to_hsl then hsl_to_rgb (rtutility.h:81-165, main.c:155-158): the colour
// tracer adds when a primary ray sees an emitter.  It depends on the
// emission alone, so each sphere's is computed here once, with the same IEEE
// operations in the same order as the kernel's hsl_roundtrip (which still
// serves triangles and the sky sphere, whose material depends on the hit).
double hue_to_rgb_host(double t1, double t2, double hue)
{
    if (hue < 0.0) hue += 1.0;
    if (hue > 1.0) hue -= 1.0;
    if (6.0 * hue < 1.0) return t1 + (t2 - t1) * 6.0 * hue;
    if (2.0 * hue < 1.0) return t2;
    if (3.0 * hue < 2.0) return t1 + (t2 - t1) * (2.0 / 3.0 - hue) * 6.0;
    return t1;
}
void hsl_roundtrip_host(const rt_vec3& rgb, double out[3])
{
    const double r = rgb.e[0], g = rgb.e[1], b = rgb.e[2];
    const double mx = (r > g) ? ((r > b) ? r : b) : ((g > b) ? g : b);
    const double mn = (r < g) ? ((r < b) ? r : b) : ((g < b) ? g : b);
    double h = 0.0, sat, l = (mx + mn) / 2.0;
    if (mx == mn) {
        h = 0.0;
        sat = 0.0;
    } else {
        const double d = mx - mn;
        sat = (l < 0.5) ? (d / (mx + mn)) : (d / (2.0 - mx - mn));
        if (mx == r) h = (g - b) / d + ((g < b) ? 6.0 : 0.0);
        else if (mx == g) h = (b - r) / d + 2.0;
        else if (mx == b) h = (r - g) / d + 4.0;
        h /= 6.0;
    }
    if (sat == 0.0) {
        out[0] = out[1] = out[2] = l;
        return;
    }
    const double t2 = (l < 0.5) ? (l * (1.0 + sat)) : (l + sat - l * sat);
    const double t1 = 2.0 * l - t2;
    const double third = 1.0 / 3.0;
    out[0] = hue_to_rgb_host(t1, t2, h + third);
    out[1] = hue_to_rgb_host(t1, t2, h);
    out[2] = hue_to_rgb_host(t1, t2, h - third);
}

// tri_uvmapping's texture coordinates (texture.h:16-27, 44-90) as affine
// functions of the hit point.  The reference forms b0 = n.((B-P)x(C-P)) / areaABC
// and b1 = n.((C-P)x(A-P)) / areaABC with n the hit normal (the triangle's unit
// normal un) and areaABC = TriTex::area; in exact arithmetic b0 = (n.N +
// ((B-C)x n).(P-A)) / area and b1 = ((C-A)x n).(P-A) / area for EVERY P (the
// component of P along n cancels in n.((B-P)x(C-P))), so u = uC + b0 (uA-uC) +
// b1 (uB-uC) = u0 + gu.(P-A).  Rounding bound of the reference's u against that,
// for P with |P - A|_max <= diam (so every |P - V|_max <= R = 2 diam), Q =
// |n|_1 R^2 / area, |b_i| <= 2Q: the cross products' components are within 8u R^2,
// each area within 14u |n|_1 R^2, each b within u (38Q + 3), and u_ref within
// sum|uv| u (54Q + 7) (u = 2^-53); the kernel's evaluation (three subtractions,
// three fma, the rounded gradient and u0, the multiplication by tw) adds at most
// 10u (|u0| + |gu|_1 diam) tw.  Stored: eu = tw (4 x the first + the second)
// + 4u tw (the reference's own frac * tw rounding) -- in tw units.
void tri_uv_affine(const TriGeo& g, const TriTex& x, int tw, int th, TriUV& o)
{
    typedef long double L;
    const L u = 0x1p-53L;
    const L Ax = g.ax, Ay = g.ay, Az = g.az, Bx = x.bx, By = x.by, Bz = x.bz, Cx = x.cx, Cy = x.cy, Cz = x.cz;
    const L nx = x.unx, ny = x.uny, nz = x.unz, area = x.area;
    const L nN = nx * (L)g.nx + ny * (L)g.ny + nz * (L)g.nz;
    const L dmax = std::max({std::fabs(Bx - Ax), std::fabs(By - Ay), std::fabs(Bz - Az), std::fabs(Cx - Ax),
                             std::fabs(Cy - Ay), std::fabs(Cz - Az), std::fabs(Cx - Bx), std::fabs(Cy - By),
                             std::fabs(Cz - Bz)});
    o = TriUV{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1.0};
    if (!(area > 0) || !std::isfinite((double)area) || !(dmax > 0) || !std::isfinite((double)dmax)) return;
    // grad b0 = (B - C) x n / area, grad b1 = (C - A) x n / area
    const L p0x = (By - Cy) * nz - (Bz - Cz) * ny, p0y = (Bz - Cz) * nx - (Bx - Cx) * nz, p0z = (Bx - Cx) * ny - (By - Cy) * nx;
    const L p1x = (Cy - Ay) * nz - (Cz - Az) * ny, p1y = (Cz - Az) * nx - (Cx - Ax) * nz, p1z = (Cx - Ax) * ny - (Cy - Ay) * nx;
    const L b0A = nN / area;                 // b0 at A (1 up to areaABC's rounding), b1 at A = 0
    const L uA = x.uau, uB = x.ubu, uC = x.ucu, vA = x.uav, vB = x.ubv, vC = x.ucv;
    const L gux = (p0x * (uA - uC) + p1x * (uB - uC)) / area, guy = (p0y * (uA - uC) + p1y * (uB - uC)) / area,
            guz = (p0z * (uA - uC) + p1z * (uB - uC)) / area;
    const L gvx = (p0x * (vA - vC) + p1x * (vB - vC)) / area, gvy = (p0y * (vA - vC) + p1y * (vB - vC)) / area,
            gvz = (p0z * (vA - vC) + p1z * (vB - vC)) / area;
    const L u0 = uC + b0A * (uA - uC), v0 = vC + b0A * (vA - vC);
    const L R = 2 * dmax;
    const L n1 = std::fabs(nx) + std::fabs(ny) + std::fabs(nz);
    const L Q = n1 * R * R / area;
    const L su = std::fabs(uA) + std::fabs(uB) + std::fabs(uC), sv = std::fabs(vA) + std::fabs(vB) + std::fabs(vC);
    const L gu1 = std::fabs(gux) + std::fabs(guy) + std::fabs(guz), gv1 = std::fabs(gvx) + std::fabs(gvy) + std::fabs(gvz);
    const L mu = std::fabs(u0) + gu1 * dmax, mv = std::fabs(v0) + gv1 * dmax;   // |u(P)|, |v(P)| bounds
    const L eu = tw * (4 * su * u * (54 * Q + 7) + 10 * u * mu + 4 * u);
    const L ev = th * (4 * sv * u * (54 * Q + 7) + 10 * u * mv + 4 * u);
    // the kernel converts floor(tw u) to int: keep |tw u| well inside 2^31
    if (!std::isfinite((double)eu) || !std::isfinite((double)ev) || tw * mu > 0x1p29L || th * mv > 0x1p29L ||
        eu > 0.25L || ev > 0.25L)
        return;
    o = TriUV{(double)gux, (double)guy, (double)guz, (double)u0, (double)gvx, (double)gvy, (double)gvz, (double)v0,
              (double)(eu * (1 + 0x1p-20L)), (double)(ev * (1 + 0x1p-20L)), (double)dmax};
}

DevMat to_dev(const rt_material& m)
{
    return DevMat{m.diffuseColor.e[0],  m.diffuseColor.e[1],  m.diffuseColor.e[2], m.emissionColor.e[0],
                  m.emissionColor.e[1], m.emissionColor.e[2], m.emissionStrength,  m.reflectionStrength,
                  m.alpha,              m.materialIndex};
}

// v in leaf order: v[k] becomes the caller's v[order[k]]
template <class T>
void leaf_order(std::vector<T>& v, const std::vector<int>& order)
{
    std::vector<T> w(v.size());
    for (size_t k = 0; k < v.size(); ++k) w[k] = v[(size_t)order[k]];
    v.swap(w);
}

// max_a |c_a| + |r| of one sphere, +inf when that is infinite: what
// bvh_origin_radius reads per sphere, SceneFacts::sph_bound's term and
// coord_max's.  std::max drops a NaN term.
double sphere_bound(const rt_sphere& q)
{
    double b = 0.0;
    for (int a = 0; a < 3; ++a) b = std::max(b, std::fabs(q.center.e[a]) + std::fabs(q.radius));
    return std::isfinite(b) ? b : HUGE_VAL;
}

// ---- The order of the candidate records (pair_candidates) ----
// The order and how many leading records are pairs that may share one root
// tail (rt_spheres.h spheres_closest): KParams::ns_merge flagged pairs, then
// KParams::ns_fwd forward pairs.  All of it is a performance hint: the pass
// gives the same winner for every order and every count (order[] goes to the
// device as KParams::cand_orig, which turns the winning record's slot back
// into the caller's sphere index); a wrongly flagged pair costs its test,
// never the result.

// RT_CAND_MERGE (tests, A/B runs): "off" flags no pair, "all" makes every pair
// of the caller's order a flagged pair, "fwd-all" every pair a forward pair --
// the results must not notice.
enum class PairMode { kHost, kOff, kAll, kFwdAll };
PairMode pair_mode()
{
    const char* mode = std::getenv("RT_CAND_MERGE");
    if (mode && !std::strcmp(mode, "off")) return PairMode::kOff;
    if (mode && !std::strcmp(mode, "all")) return PairMode::kAll;
    if (mode && !std::strcmp(mode, "fwd-all")) return PairMode::kFwdAll;
    return PairMode::kHost;
}

// Both rules look at kMergeScan spheres: the unpaired ones of smallest or of
// largest radius, in that order (ties by index).
constexpr int kMergeScan = 32;
std::vector<int> scan_list(const rt_scene* scene, const std::vector<char>& used, bool largest)
{
    auto rad = [&](int i) { return std::fabs(scene->sphere_list[i].radius); };
    std::vector<int> list;
    for (int i = 0; i < scene->nbSpheres; ++i)
        if (!used[i]) list.push_back(i);
    const int m = std::min((int)list.size(), kMergeScan);
    std::partial_sort(list.begin(), list.begin() + m, list.end(), [&](int x, int y) {
        return rad(x) != rad(y) ? (largest ? rad(x) > rad(y) : rad(x) < rad(y)) : x < y;
    });
    list.resize((size_t)m);
    return list;
}

// Both rules pair greedily: in the list's order each unpaired sphere takes the
// unpaired partner after it with the smallest score, and the two are appended
// to `order` as a pair when that score is at most `limit`.  A pair that is not
// eligible scores +inf or NaN, which is never the smallest.
template <class Score>
void pair_greedy(const std::vector<int>& list, Score score, double limit, std::vector<char>& used,
                 std::vector<int>& order)
{
    for (size_t ii = 0; ii < list.size(); ++ii) {
        const int i = list[ii];
        if (used[i]) continue;
        int best = -1;
        double sbest = HUGE_VAL;
        for (size_t jj = ii + 1; jj < list.size(); ++jj) {
            const int j = list[jj];
            if (used[j]) continue;
            const double s = score(i, j);
            if (s < sbest) {
                sbest = s;
                best = j;
            }
        }
        if (best >= 0 && sbest <= limit) {
            used[i] = used[best] = 1;
            order.push_back(i);
            order.push_back(best);
        }
    }
}

// Flagged pairs.  The kernel merges a flagged pair's tails in a wave-cast in
// which no lane's line crosses both spheres, and pays about nine cheap VALU
// instructions for the test and the selects against a 15-instruction tail, so
// a pair is worth flagging when that is the common case.
// The rule: of the lines through the centre of one sphere the fraction
// 1 - sqrt(1 - (R/d)^2) <= (R/d)^2 crosses a disjoint sphere of radius R whose
// centre is d away.  Among the kMergeScan spheres of smallest radius (small
// spheres are the ones few lines cross at all), in ascending radius, each
// unpaired sphere takes the unpaired partner with the smallest
// x = (max(R_i, R_j) / d)^2, and the pair is flagged when x <= 1/16 (the
// README box: its five radius-0.5 spheres give two pairs with x < 0.03; a
// radius-500 wall overlaps every other sphere and is never flagged).
// Overlapping, touching and nested spheres have x > 1/16.  An odd count leaves
// the never-hit padding record, which no line crosses: it is flagged with one
// more sphere.
//
// Forward pairs.  The kernel merges such a pair's tails when no lane moves
// towards both spheres, (o - C) . d < 0 for both, and a ray does that only
// when its direction lies in the wedge between the two half-spaces whose
// normals point from its origin to the two centres.  The wedge is thin when
// the origin lies between the spheres: outside both, with the centres nearly
// opposite.  The centroid P of all other spheres' centres stands for where rays
// start (every ray but the camera's starts on a sphere).  Among the kMergeScan
// unflagged spheres of largest radius (large spheres are the ones whose
// D > 0 on most rays, which the first rule cannot merge), in descending
// radius, each takes the unpaired partner with the smallest c = cos of the
// angle C_i P C_j, among partners that are disjoint from it by a margin, d^2 >
// (R_i + R_j)^2 (1 + 2^-12) (touching, overlapping and nested spheres have an
// origin on or in one of them where a ray moves towards both in half of the
// directions), with P outside both, and the pair is flagged when c <= -0.9.
// P is a coarse stand-in, so the threshold is loose: the README box's left/right
// and floor/ceiling walls give c = -0.9675 (its back wall drags P 64 units
// behind the box), while two walls that meet in an edge give c near 0 and a
// wall with a small sphere in front of it c > 0.9.
//
// The other spheres follow in the caller's order, the padding record last if
// no pair took it.  finite: every sphere's centre and radius are finite (else
// no pair of either kind); forward pairs also need three spheres and the
// candidate pass switched on (a finite f.cand_lmax).
void pair_candidates(const rt_scene* scene, bool finite, SceneFacts& f, std::vector<int>& order)
{
    const int ns = f.ns;
    const rt_sphere* sph = scene->sphere_list;
    auto rad = [&](int i) { return std::fabs(sph[i].radius); };
    order.clear();
    f.ns_merge = f.ns_fwd = 0;
    const PairMode mode = pair_mode();
    if (mode != PairMode::kHost) {
        for (int i = 0; i < f.ns_pad; ++i) order.push_back(i);
        f.ns_merge = mode == PairMode::kAll ? f.ns_pad : 0;
        f.ns_fwd = mode == PairMode::kFwdAll ? f.ns_pad : 0;
        return;
    }
    std::vector<char> used((size_t)ns, 0);
    if (finite) {
        const std::vector<int> small = scan_list(scene, used, false);
        pair_greedy(small, [&](int i, int j) {
            double d2 = 0.0;
            for (int a = 0; a < 3; ++a) d2 += (sph[i].center.e[a] - sph[j].center.e[a]) * (sph[i].center.e[a] - sph[j].center.e[a]);
            const double rm = std::max(rad(i), rad(j));
            return rm * rm / d2;                                // (d = 0: +inf or NaN)
        }, 1.0 / 16, used, order);
        if (ns < f.ns_pad) {                                    // odd count: one sphere shares the padding's pair
            for (int i : small)
                if (!used[i]) {
                    used[i] = 1;
                    order.push_back(i);
                    order.push_back(ns);
                    break;
                }
        }
        f.ns_merge = (int)order.size();
    }
    if (finite && ns >= 3 && std::isfinite(f.cand_lmax)) {
        long double sum[3] = {0.0L, 0.0L, 0.0L};
        for (int i = 0; i < ns; ++i)
            for (int a = 0; a < 3; ++a) sum[a] += sph[i].center.e[a];
        pair_greedy(scan_list(scene, used, true), [&](int i, int j) {
            const rt_sphere &p = sph[i], &q = sph[j];
            double d2 = 0.0, uv = 0.0, uu = 0.0, vv = 0.0;
            for (int a = 0; a < 3; ++a) {
                const double P = (double)((sum[a] - p.center.e[a] - q.center.e[a]) / (ns - 2));
                const double u = p.center.e[a] - P, v = q.center.e[a] - P;
                d2 += (p.center.e[a] - q.center.e[a]) * (p.center.e[a] - q.center.e[a]);
                uv += u * v;
                uu += u * u;
                vv += v * v;
            }
            const double rs = rad(i) + rad(j);
            if (!(d2 > rs * rs * (1.0 + 0x1p-12)) || !(uu > rad(i) * rad(i)) || !(vv > rad(j) * rad(j))) return HUGE_VAL;
            return uv / std::sqrt(uu * vv);                     // (overflow: NaN)
        }, -0.9, used, order);
        f.ns_fwd = (int)order.size() - f.ns_merge;
    }
    for (int i = 0; i < ns; ++i)
        if (!used[i]) order.push_back(i);
    if ((int)order.size() < f.ns_pad) order.push_back(ns);      // (no pair took the padding record)
}

}  // namespace

int prepare_scene(const rt_scene* scene, HostScene& hs, std::string& err)
{
    hs = HostScene();
    SceneFacts& f = hs.facts;
    const int ns = scene->nbSpheres, nt = scene->nbTriangles;
    if (nt > 0) {
        f.n_texels = (long long)scene->nbMaterials * scene->tex_width * scene->tex_height;
        if (f.n_texels >= (1LL << 31)) {     // the kernels index texels in 32 bits (160 GiB of texels)
            err = std::to_string(f.n_texels) + " texels >= 2^31";
            return RT_EUNSUPPORTED;
        }
    }
    f.ns = ns;
    f.nt = nt;
    f.tw = nt > 0 ? scene->tex_width : 1;
    f.th = nt > 0 ? scene->tex_height : 1;
    f.sky_w = scene->sky_mat_list ? scene->sky_width : 0;
    f.sky_h = scene->sky_mat_list ? scene->sky_height : 0;
    // fmax drops NaN operands: a non-finite coordinate anywhere makes the bound
    // infinite (coords_finite, below), so the gates that read it (zero_exit,
    // tex_const) hold by construction
    double coord_max = 0.0;

    // Spheres padded to an even count with never-hit records (r2 = -inf makes
    // the discriminant -inf): the kernel reads them two per s_load_dwordx16.
    // The candidate pass keeps the winner's slot in 16 mantissa bits (cand_tag):
    // above 65534 spheres it is switched off (cand_lmax = +inf, KParams::ns_cand = 0)
    // and every ray takes the exact reference scan -- correct for any count, slower.
    f.ns_pad = (ns + 1) & ~1;
    hs.sph.assign((size_t)f.ns_pad, SphGeo{0.0, 0.0, 0.0, -HUGE_VAL});
    std::vector<SphCand> by_sphere((size_t)f.ns_pad, SphCand{0.0, 0.0, 0.0, HUGE_VAL});
    hs.sph_mat.resize((size_t)ns);
    hs.sph_rinv.resize((size_t)ns);
    hs.sph_disp.resize((size_t)ns * 3);
    std::vector<double> sb((size_t)ns);              // sphere_bound of each
    bool spheres_finite = true;
    // Candidate-pass bound L >= |C_k| + R_k for every sphere (rounded up, at
    // least 2^-20); a non-finite sphere makes it +inf, which turns the
    // candidate pass into the exact scan (rt_spheres.h spheres_closest).
    long double lmax = 0x1p-20L;
    for (int i = 0; i < ns; ++i) {
        const rt_sphere& s = scene->sphere_list[i];
        const double r2 = s.radius * s.radius;
        hs.sph[i] = SphGeo{s.center.e[0], s.center.e[1], s.center.e[2], r2};
        const long double cx = s.center.e[0], cy = s.center.e[1], cz = s.center.e[2];
        const long double c2 = cx * cx + cy * cy + cz * cz;
        by_sphere[i] = SphCand{s.center.e[0], s.center.e[1], s.center.e[2], (double)(c2 - (long double)r2)};
        const long double L = (std::sqrt(c2) + std::fabs((long double)s.radius)) * (1.0L + 0x1p-40L);
        lmax = std::isfinite((double)L) && !std::isnan((double)by_sphere[i].k) ? std::max(lmax, L) : (long double)HUGE_VAL;
        hs.sph_mat[i] = to_dev(s.mat);
        hs.sph_rinv[i] = 1 / s.radius;                 // divide(v, t) = v * (1/t), vec3.h:105-107
        hsl_roundtrip_host(s.mat.emissionColor, &hs.sph_disp[3 * (size_t)i]);
        sb[(size_t)i] = sphere_bound(s);
        f.sph_bound = std::max(f.sph_bound, sb[(size_t)i]);
        coord_max = std::fmax(coord_max, sb[(size_t)i]);
        spheres_finite = spheres_finite && std::isfinite(s.radius) && std::isfinite(s.center.e[0]) &&
                         std::isfinite(s.center.e[1]) && std::isfinite(s.center.e[2]);
    }
    bool coords_finite = spheres_finite;
    f.cand_lmax = std::isfinite((double)lmax) && ns <= 65534 ? std::nextafter((double)lmax, HUGE_VAL) : HUGE_VAL;
    // the candidate records in pairing order; SphGeo and the per-sphere tables keep the caller's
    pair_candidates(scene, spheres_finite, f, hs.cand_orig);
    hs.sph_cand.resize((size_t)f.ns_pad);
    hs.sph_slot.resize((size_t)f.ns_pad);
    for (int j = 0; j < f.ns_pad; ++j) {
        hs.sph_cand[j] = by_sphere[hs.cand_orig[j]];
        hs.sph_slot[j] = hs.sph[hs.cand_orig[j]];
    }
    if (scene->sky_mat_list)
        for (long long i = 0; i < (long long)scene->sky_width * scene->sky_height; ++i)
            hs.sky.push_back(to_dev(scene->sky_mat_list[i]));

    std::vector<TriGeo>& tri = hs.tri;
    std::vector<TriTex>& tex = hs.tri_tex;
    tri.resize((size_t)nt);
    tex.resize((size_t)nt);
    hs.tri_mat.resize((size_t)nt);
    double tri_max = 0.0;                            // max |vertex coordinate| (NaN dropped)
    if (nt > 0)                                      // load_geometry_data's box, triangle.hu:142-156
        for (int a = 0; a < 3; ++a) f.cbb[a] = f.cbb[3 + a] = scene->triangle_list[0].A.e[a];
    for (int i = 0; i < nt; ++i) {
        const rt_triangle& t = scene->triangle_list[i];
        for (int a = 0; a < 3; ++a) {
            f.cbb[a] = std::fmin(f.cbb[a], std::fmin(t.A.e[a], std::fmin(t.B.e[a], t.C.e[a])));
            f.cbb[3 + a] = std::fmax(f.cbb[3 + a], std::fmax(t.A.e[a], std::fmax(t.B.e[a], t.C.e[a])));
            tri_max = std::fmax(tri_max, std::fmax(std::fabs(t.A.e[a]), std::fmax(std::fabs(t.B.e[a]), std::fabs(t.C.e[a]))));
            coords_finite = coords_finite && std::isfinite(t.A.e[a]) && std::isfinite(t.B.e[a]) && std::isfinite(t.C.e[a]);
        }
        const double abx = t.B.e[0] - t.A.e[0], aby = t.B.e[1] - t.A.e[1], abz = t.B.e[2] - t.A.e[2];
        const double acx = t.C.e[0] - t.A.e[0], acy = t.C.e[1] - t.A.e[1], acz = t.C.e[2] - t.A.e[2];
        TriGeo& g = tri[i];
        g = TriGeo{t.A.e[0], t.A.e[1], t.A.e[2], abx, aby, abz, acx, acy, acz,
                   aby * acz - abz * acy, abz * acx - abx * acz, abx * acy - aby * acx};   // vec3_cross, vec3.h:121-127
        TriTex& x = tex[i];
        x = TriTex{t.B.e[0], t.B.e[1], t.B.e[2], t.C.e[0], t.C.e[1], t.C.e[2], t.uvA.u, t.uvA.v, t.uvB.u, t.uvB.v,
                   t.uvC.u, t.uvC.v, scene->quelMatPourTri[i], -1, 0.0, 0.0, 0.0, 0.0};
        if (t.uvA.u == 0.0 && t.uvA.v == 0.0 && t.uvB.u == 0.0 && t.uvB.v == 0.0 && t.uvC.u == 0.0 &&
            t.uvC.v == 0.0) {
            // tri_uvmapping (texture.h:44-90) with every uv 0: u = v = +-0 for
            // finite barycentrics, so x = y = 0 and the index is tw*th*mat (clamped
            // into the table as the kernel clamps it)
            long long idx = (long long)scene->tex_height * scene->tex_width * x.mat;
            idx = idx < 0 ? 0 : idx;
            idx = idx >= f.n_texels ? f.n_texels - 1 : idx;
            if (f.n_texels > 0) x.tex0 = (int)idx;
        }
        // hit_triangle's normal, vec3_normalize(normalVect) (mesh.h:91, vec3.h:137-139):
        // a pure function of the triangle, computed once here with the reference's
        // operations (IEEE sqrt and divisions, no contraction) instead of per hit
        const double nl = std::sqrt((g.nx * g.nx + g.ny * g.ny) + g.nz * g.nz);
        x.unx = g.nx / nl;
        x.uny = g.ny / nl;
        x.unz = g.nz / nl;
        // get_barycentric_coord's areaABC (texture.h:18) with the hit normal n = un:
        // dot(n, cross(B - A, C - A)) = dot(un, N), constant per triangle
        x.area = (x.unx * g.nx + x.uny * g.ny) + x.unz * g.nz;
        hs.tri_mat[i] = to_dev(t.mat);
    }
    f.coord_max = coords_finite ? std::fmax(coord_max, tri_max) : HUGE_VAL;
    // Triangle BVH (rt_bvh.cpp) over scenes with more than 32 triangles; the
    // triangle arrays are then stored in leaf order.  r_scene bounds the
    // triangles' coordinates (so every hit point on them) and the spheres
    // whose hit points cost the padding little (bvh_origin_radius); the padding
    // assumes origins within it, and rays from farther out (the camera, hit
    // points on large spheres such as main.c:346's radius-1e5 sky) widen the
    // walk's margins by the rest (rt_triangles.h ray32).  Against r_scene over
    // every sphere: RTX_MAP/nature under the sky 700 -> 808 Msamples/s at 64 spp
    // (r06, tools/probes/nature_radius.py)
    BvhBuild bvh;
    if (nt > 32) {                           // (a BVH over C3's 5 triangles: 5118 -> 4482 Msamples/s)
        double r = std::max(1.0, tri_max);
        if (std::isfinite(r)) r = bvh_origin_radius(tri.data(), nt, r, sb.data(), ns);
        if (std::isfinite(r) && build_bvh(tri.data(), nt, r, bvh)) {
            leaf_order(tri, bvh.order);
            leaf_order(tex, bvh.order);
            leaf_order(hs.tri_mat, bvh.order);
        }
    }
    hs.texels.resize((size_t)f.n_texels);
    for (long long i = 0; i < f.n_texels; ++i) hs.texels[(size_t)i] = to_dev(scene->mat_list[i]);

    f.mats_bounded = true;
    for (const std::vector<DevMat>* v : {&hs.sph_mat, &hs.texels, &hs.sky})
        for (const DevMat& m : *v) f.mats_bounded = f.mats_bounded && shading_bounded(m);
    const auto opaque_mat = [](const DevMat& m) { return !(m.alpha < 0.0001) && !(m.alpha <= 0.99); };
    f.sph_opaque = std::all_of(hs.sph_mat.begin(), hs.sph_mat.end(), opaque_mat);
    // tri_material (rt_shading.h): the texel's alpha, overridden for
    // material indices 1 (1.0), 3 (0.1) and 4 (0.6); the texel index is
    // clamped into the whole table, so every texel counts
    f.tri_opaque = std::all_of(hs.texels.begin(), hs.texels.end(), opaque_mat);
    for (int i = 0; i < nt && f.tri_opaque; ++i)
        if (scene->quelMatPourTri[i] == 3 || scene->quelMatPourTri[i] == 4) f.tri_opaque = false;
    f.all_tex0 = nt > 0 && std::all_of(tex.begin(), tex.end(), [](const TriTex& x) { return x.tex0 >= 0; });
    // the affine texel map (rt_shading.h tri_texel's fast path), in leaf order
    if (nt > 0 && !f.all_tex0) {
        hs.tri_uv.resize(tex.size());
        for (size_t i = 0; i < tex.size(); ++i) tri_uv_affine(tri[i], tex[i], scene->tex_width, scene->tex_height, hs.tri_uv[i]);
    }
    f.bvh_nodes = (int)bvh.nodes4.size();
    f.bvh_depth = bvh.depth4;
    f.bvh_stack4 = bvh.stack4;
    f.bvh_wide = bvh.wide;
    f.s_rel = bvh.s_rel;
    f.s_abs = bvh.s_abs;
    f.r_scene = bvh.r_scene;
    f.k_delta = bvh.k_delta;
    {
        float rb = 0.0f;             // the single-precision slab margin's coordinate bound
        for (const BvhNode4& nd : bvh.nodes4)
            for (int c = 0; c < 4; ++c)
                if (nd.count[c] >= 0)
                    for (int a = 0; a < 3; ++a) rb = std::max({rb, std::fabs(nd.lo[a][c]), std::fabs(nd.hi[a][c])});
        f.bvh_rbox = std::isfinite(rb) ? rb * (1.0f + 0x1p-20f) : HUGE_VALF;
        float rbh = 0.0f;
        if (!bvh.nodes4.empty() && !bvh.wide && pack_bvh_h(bvh.nodes4, hs.bvhh, rbh))
            f.bvh_rbox = std::max(f.bvh_rbox, rbh * (1.0f + 0x1p-20f));   // one bound serves both forms
        else
            hs.bvhh.clear();
        if (bvh.wide && pack_bvh_w(bvh.nodes4, hs.bvhw, rbh))            // (a wide tree: its own 64-byte form)
            f.bvh_rbox = std::max(f.bvh_rbox, rbh * (1.0f + 0x1p-20f));
        else
            hs.bvhw.clear();
    }
    hs.bvh.swap(bvh.nodes4);
    hs.tri_orig.swap(bvh.order);
    return RT_OK;
}

}  // namespace rt
