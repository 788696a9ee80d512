// rt_shading.h -- Texturing, materials, sampling, refraction, the HSL round trip and ambient_occlusion.
// Part of the single translation unit rt_kernels.hip (included there, in this order).
#pragma once

namespace rt {

// tri_uvmapping + get_barycentric_coord, texture.h:16-27,44-90, in two
// steps: the texel a hit picks (barycentrics, uv, fmod, the clamped index)
// and the material read from it (with the material-index overrides).  A
// refraction lane keeps the TexRef from resolve_hit to finish_bounce instead
// of recomputing the barycentrics (host: n_texels < 2^31).
struct TexRef {
    int index;                        // clamped texel index
    int m;                            // the triangle's material index (quelMatPourTri)
};
// hit_triangle's normal vec3_normalize(N) (mesh.h:91): the host's copy
// (TriTex::un*, the same IEEE operations) instead of normalizing N per hit
__device__ __forceinline__ V3 tri_normal(const KParams& kp, int k)
{
    const TriTex* t = kp.tri_tex + k;
    return v3(t->unx, t->uny, t->unz);
}
// The texel through the host's affine uv map (rt_scene_prep.cpp tri_uv_affine): the
// reference's u, v are affine in P up to rounding, so with tw*u within eu of tu,
// x = floor(tw u_ref) - tw floor(u_ref) is certain when no integer lies in
// [tu - eu, tu + eu] (the wrap at integer u and the cells at multiples of 1/tw
// are all integers of tw*u); the same for v.  False: not certain (or P farther
// than diam from A, where the bound does not hold) -- the caller then takes the
// exact path.  rt_verify_texel_map checks it against tri_texel_exact.
__device__ __forceinline__ bool tri_texel_affine(const KParams& kp, int k, const V3 P, TexRef& t)
{
    const TriUV q = kp.tri_uv[k];
    const TriGeo* gp = kp.tri + k;
    const double dx = P.x - gp->ax, dy = P.y - gp->ay, dz = P.z - gp->az;
    const double uf = fma(q.gux, dx, fma(q.guy, dy, fma(q.guz, dz, q.u0)));
    const double vf = fma(q.gvx, dx, fma(q.gvy, dy, fma(q.gvz, dz, q.v0)));
    const double tw = (double)kp.tw, th = (double)kp.th;
    const double tu = uf * tw, tv = vf * th;
    const double lu = floor(tu - q.eu), lv = floor(tv - q.ev);
    if (!(dmax_abs3(dx, dy, dz) <= q.diam && lu == floor(tu + q.eu) && lv == floor(tv + q.ev))) return false;
    const int x = (int)fma(-tw, floor(uf), lu), y = (int)fma(-th, floor(vf), lv);
    const int m = kp.tri_tex[k].mat;
    long long index = ((long long)y * kp.tw + x) + ((long long)kp.th * kp.tw * m);
    index = index < 0 ? 0 : index;                       // reference UB -> clamp
    index = index >= kp.n_texels ? kp.n_texels - 1 : index;
    t = TexRef{(int)index, m};
    return true;
}
// tri_uvmapping + get_barycentric_coord with the reference's operations
__device__ __forceinline__ TexRef tri_texel_exact(const KParams& kp, int k, const V3 P, const V3 n)
{
    const TriGeo g = kp.tri[k];
    const TriTex tx = kp.tri_tex[k];
    const V3 A = v3(g.ax, g.ay, g.az), B = v3(tx.bx, tx.by, tx.bz), C = v3(tx.cx, tx.cy, tx.cz);
    // areaABC = dot(n, cross(B-A, C-A)) = dot(n, N): n is the triangle's own
    // unit normal (tri_normal), so the host's TriTex::area is the same value
    const double areaABC = tx.area;
    const double areaPBC = dot(n, cross(B - P, C - P));
    const double areaPCA = dot(n, cross(C - P, A - P));
    const double b0 = areaPBC / areaABC;
    const double b1 = areaPCA / areaABC;
    const double b2 = 1.0 - b0 - b1;
    double u = (b0 * tx.uau + b1 * tx.ubu + b2 * tx.ucu);
    double v = (b0 * tx.uav + b1 * tx.ubv + b2 * tx.ucv);
    u = u - trunc(u);                 // fmod(u, 1.0): exact
    v = v - trunc(v);
    if (u < 0) u += 1.0;
    if (v < 0) v += 1.0;
    const int x = cvt_i32_x86(u * (double)(kp.tw));
    const int y = cvt_i32_x86(v * (double)(kp.th));
    const int m = tx.mat;
    long long index = ((long long)y * kp.tw + x) + ((long long)kp.th * kp.tw * m);
    index = index < 0 ? 0 : index;                       // reference UB -> clamp
    index = index >= kp.n_texels ? kp.n_texels - 1 : index;
    return TexRef{(int)index, m};
}
__device__ __forceinline__ TexRef tri_texel(const KParams& kp, int k, const V3 P, const V3 n)
{
    if (kp.tex_const)                            // every uv 0: the texel does not depend on P
        return TexRef{kp.tri_tex[k].tex0, kp.tri_tex[k].mat};
    if (kp.tri_uv) {                             // the host's affine uv map when certain
        TexRef t;
        if (tri_texel_affine(kp, k, P, t)) return t;
    }
    return tri_texel_exact(kp, k, P, n);
}
__device__ __forceinline__ Mat texel_material(const KParams& kp, TexRef t)
{
    const int m = t.m;
    Mat res = load_mat(kp.texels + t.index);
    const cdptr b = kcb();
    if (m == 1) {
        res.emis = v3(1, 1, 1);
        res.es = KCV(b, KC_ES1);          // 1.85
        res.alpha = 1.0;
    }
    if (m == 4) {
        res.alpha = KCV(b, KC_A4);        // 0.6
        res.ior = KCV(b, KC_IOR4);        // 1.33
        res.rs = KCV(b, KC_RS4);          // 0.93
    }
    if (m == 3) {
        res.alpha = KCV(b, KC_A3);        // 0.1
        res.ior = KCV(b, KC_IOR3);        // 1.50
        res.rs = KCV(b, KC_RS3);          // 0.3
    }
    return res;
}
__device__ __forceinline__ Mat tri_material(const KParams& kp, int k, const V3 P, const V3 n)
{
    return texel_material(kp, tri_texel(kp, k, P, n));
}

// Sky branch of closest_hit (main.c:64-71, commented out in the reference;
// RT_SKY_LAST_SPHERE): emissionColor = sphere_uvmapping's texel (texture.h:
// 92-112), alpha = 1.  The texel index is clamped into the table (the
// reference indexes unchecked).
__device__ __forceinline__ void sky_material(const KParams& kp, int idx, const SphGeo& s, V3 hp, Mat& mat)
{
    const double ri = kp.sph_rinv[idx];
    const double dx = (hp.x - s.cx) * ri, dy = (hp.y - s.cy) * ri, dz = (hp.z - s.cz) * ri;
    const cdptr b = kcb();
    const double PI = KCV(b, KC_PI);
    const double theta = pm_acos(-dy);
    const double phi = pm_atan2(-dz, dx) + PI;
    const double u = phi / (2 * PI), v = theta / PI;
    const int x = cvt_i32_x86(u * (double)kp.sky_w);
    const int y = cvt_i32_x86(v * (double)kp.sky_h);
    long long index = (long long)y * kp.sky_w + x;
    const long long n = (long long)kp.sky_w * kp.sky_h;
    index = index < 0 ? 0 : (index >= n ? n - 1 : index);
    const DevMat* t = kp.sky + index;
    mat.emis = v3(t->dr, t->dg, t->db);
    mat.alpha = 1.0;
}

// randomDouble(-0.5, 0.5) and randomDouble(0, 1) of one 31-bit draw r
// (rtutility.h:229-231: min + (max - min) * (r / 2^31)): r / 2^31 and the
// product by 1 are exact, so the result is ONE rounding of r 2^-31 - 0.5, i.e.
// fma(r, 2^-31, -0.5), and r 2^-31 itself for [0, 1) (0.0 + u == u for u >= 0)
__device__ __forceinline__ double rand_m05(uint32_t r) { return fma((double)r, 0x1p-31, -0.5); }
__device__ __forceinline__ double rand_01(uint32_t r) { return (double)r * 0x1p-31; }

// random_dir_no_norm's vector before its normalize, rtutility.h:192-200
// (float sinf/cosf of double args), from its two 31-bit draws ru, rv:
// u = ru / 2^31 and v = rv / 2^31 are exact, so 2 PI u = ru (2 PI 2^-31)
// (one rounding of the same product) and 2 v - 1 = fma(rv, 2^-30, -1) (2 v
// exact, one rounding of the difference): the reference's values in three
// VALU fewer
__device__ __forceinline__ V3 sampler_vec(uint32_t ru, uint32_t rv)
{
    const double theta = (double)ru * 0x1.921fb54442d18p-29;      // 2*PI*u
    const double xv = fma((double)rv, 0x1p-30, -1.0);              // phi = acos(2v - 1): only (float)phi is used
    float st_, ct_, sp_, cp_;
    if (!phi_sincosf_fast(xv, sp_, cp_)) {                // uncertain rounding (~1e-4): full path
        const double phi = pm_acos(xv);
        pm_sincosf((float)phi, sp_, cp_);
    }
    pm_sincosf((float)theta, st_, ct_);
    return v3((double)(ct_ * sp_), (double)(st_ * sp_), (double)cp_);
}

// random_dir_no_norm, rtutility.h:189-203
template <bool COUNT>
__device__ __forceinline__ V3 random_dir(Stream& st, Cnt& cnt)
{
    if (COUNT) cnt.c[RT_CNT_SHADE] += 1;
    const uint32_t ru = st.next31();
    const uint32_t rv = st.next31();
    const V3 dir = sampler_vec(ru, rv);
    return normalize_unit(dir);
}

// refracted_vec, rtutility.h:210-227 (indices squared: reference quirk)
__device__ __forceinline__ V3 refracted(V3 v, V3 nrm, double n1, double n2)
{
    n1 *= n1;
    n2 *= n2;
    const double cn = dot(nrm, v);
    const double radical = 1 - ((n1 / n2) * (n1 / n2)) * (1 - (cn * cn));
    if (radical > 0) {
        const V3 comp_tan = muls(v - muls(nrm, dot(v, nrm)), (n1 / n2));
        const V3 comp_normal = muls(v3(-nrm.x, -nrm.y, -nrm.z), sqrt(radical));
        return comp_tan + comp_normal;
    }
    return v - muls(nrm, 2 * dot(v, nrm));
}

// The refracted direction at a translucent hit, main.c:167-193: leaving the
// medium (d along the normal) pops the IOR stack, entering pushes (top.n2,
// ior).  pile.h's stack reduces to its top n2, one register.
__device__ __forceinline__ V3 refracted_at(V3 d, V3 hn, double ior, double& top_n2)
{
    V3 nn = hn;
    double n1, n2;
    if (dot(d, hn) > 0) {                            // leaving: pop restores the stack
        nn = v3(-hn.x, -hn.y, -hn.z);
        n1 = ior;
        n2 = top_n2;
    } else {                                         // entering: push (top.n2, ior)
        n1 = top_n2;
        n2 = ior;
        top_n2 = ior;
    }
    return refracted(d, nn, n1, n2);
}

// rgb_to_hsl / hsl_to_rgb round trip, rtutility.h:81-165 (main.c:155-158)
__device__ __forceinline__ double hue_to_rgb(double t1, double t2, double hue)
{
    if (hue < 0.0) hue += 1.0;
    if (hue > 1.0) hue -= 1.0;
    if (6.0 * hue < 1.0) return t1 + (t2 - t1) * 6.0 * hue;
    if (2.0 * hue < 1.0) return t2;
    if (3.0 * hue < 2.0) return t1 + (t2 - t1) * (KCV(kcb(), KC_TWO_THIRDS) - hue) * 6.0;
    return t1;
}
// CU: main_cuda.cu:92-93 raise L and S by 1.20 (main.c:156-157: x1.0)
template <bool CU = false>
__device__ __forceinline__ V3 hsl_roundtrip(V3 rgb)
{
    const double r = rgb.x, g = rgb.y, b = rgb.z;
    const double mx = (r > g) ? ((r > b) ? r : b) : ((g > b) ? g : b);
    const double mn = (r < g) ? ((r < b) ? r : b) : ((g < b) ? g : b);
    double h = 0.0, s, l = (mx + mn) / 2.0;
    if (mx == mn) {
        h = 0.0;
        s = 0.0;
    } else {
        const double d = mx - mn;
        s = (l < 0.5) ? (d / (mx + mn)) : (d / (2.0 - mx - mn));
        if (mx == r) h = (g - b) / d + ((g < b) ? 6.0 : 0.0);
        else if (mx == g) h = (b - r) / d + 2.0;
        else if (mx == b) h = (r - g) / d + 4.0;
        h /= 6.0;
    }
    l *= CU ? 1.20 : 1.0;
    s *= CU ? 1.20 : 1.0;
    if (s == 0.0) return v3(l, l, l);
    const double t2 = (l < 0.5) ? (l * (1.0 + s)) : (l + s - l * s);
    const double t1 = 2.0 * l - t2;
    const double third = KCV(kcb(), KC_THIRD);                 // 1.0 / 3.0
    return v3(hue_to_rgb(t1, t2, h + third), hue_to_rgb(t1, t2, h), hue_to_rgb(t1, t2, h - third));
}

// ambient_occlusion's tail, main.c:104-115: the factor rayColor is multiplied
// by after an AO cast from p along dir (hit: it hit something, at distance t).
__device__ __forceinline__ double ao_tail(bool hit, const V3 p, const V3 dir, double t, double AO)
{
    double occ = 0.0;
    if (hit) {
        const V3 hp = p + muls(dir, t);
        const V3 df = hp - p;
        const double distance = sqrt(dot(df, df));
        double att = distance / t;
        att = pm_pow(att, AO);
        occ = occ + att;
    }
    return (occ / 1.0) / AO;
}

// ambient_occlusion, main.c:94-116: one cast, only distance/dst matters.
template <bool COUNT, bool BVH, bool CU = false, class SE = unsigned short>
__device__ __forceinline__ double ao_factor(const KParams& kp, const V3 p, const V3 n, double AO, Stream& st,
                                            Cnt& cnt)
{
    const V3 rd = random_dir<COUNT>(st, cnt);
    const V3 dir = normalize(n + rd);
    double t;
    int idx;
    const int kind = closest_hit<cf(COUNT, CF_COUNT) | cf(BVH, CF_BVH) | cf(CU, CF_CUDA), SE>(kp, p, dir, t, idx, cnt);
    return ao_tail(kind != HIT_NONE, p, dir, t, AO);
}

}  // namespace rt
