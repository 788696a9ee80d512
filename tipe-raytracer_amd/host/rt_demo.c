/*
 * rt_demo.c — main.c's flow (main.c:286-498) on the MI355X render path:
 * scene constants -> optional OBJ/MTL mesh + texel table -> init_camera ->
 * ONE rt_render_rows call (instead of the pthread band loop main.c:402-453)
 * -> optional denoiser hook -> P3 PPM (main.c:457-465).
 *
 *   rt_demo [-w W] [-s spp] [-b nbRebondMax] [-ao AO_intensity] [-o out.ppm]
 *           [-obj file.obj -mtl file.mtl [-move x y z]] [-devices N]
 *           [-denoise [iterations]] [-vdenoise [iterations]] [-adaptive TOL]
 *           [-queue] [-packed]
 *
 * -denoise installs the library's built-in a-trous filter (rt_denoise_atrous;
 * not OIDN, and biased: meant for low-spp frames) as the denoiser hook before
 * the render, with `iterations` passes (default 4; more for larger frames).
 * -vdenoise renders through rt_render_vdenoised instead: the variance-guided
 * denoiser over the frame's two sample halves (spp must be even; one device).
 * -adaptive renders through rt_render_adaptive with tolerance TOL (the other
 * parameters at their defaults; -s is ignored; one device) and also prints the
 * mean samples per pixel and the share of pixels per round count.
 * -adaptive with -vdenoise renders through rt_render_adaptive_vdenoised: the
 * adaptive frame filtered with each pixel's own sample count.
 * -queue (with -vdenoise or -adaptive) turns rt_set_accumulate_queue on: their
 * batches take the task-queue kernel; the frame is the same.
 * -packed turns the packed canva transport on (rt_set_fill_packed_canva and
 * RT_GATHER_PACKED_CANVA in the params): the canva leaves the device at 4
 * bytes a pixel; the frame is the same.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>

#include "rt/host.h"
#include "rt/rt.h"

#define C3(a, b, c) {{a, b, c}}
#define MAT(d, e, es, rs) {d, e, es, rs, 1.0, 1.0}

int main(int argc, char** argv)
{
    int W = 400, spp = 100, bounces = 5, ndev = 1, useAO = 0, denoise = 0;
    rt_denoise_params dn;
    rt_denoise_params_init(&dn);
    int vdenoise = 0;
    rt_vdenoise_params vdn;
    rt_vdenoise_params_init(&vdn);
    int adaptive = 0, queue = 0, packed = 0;
    rt_adaptive_params adp;
    rt_adaptive_params_init(&adp);
    double AO = 2.5, mx = 0, my = 0, mz = 0;
    const char *out = "render.ppm", *obj = NULL, *mtl = NULL;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-w") && i + 1 < argc) W = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-s") && i + 1 < argc) spp = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-b") && i + 1 < argc) bounces = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-ao") && i + 1 < argc) { useAO = 1; AO = atof(argv[++i]); }
        else if (!strcmp(argv[i], "-o") && i + 1 < argc) out = argv[++i];
        else if (!strcmp(argv[i], "-obj") && i + 1 < argc) obj = argv[++i];
        else if (!strcmp(argv[i], "-mtl") && i + 1 < argc) mtl = argv[++i];
        else if (!strcmp(argv[i], "-devices") && i + 1 < argc) ndev = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-denoise")) {
            denoise = 1;
            if (i + 1 < argc && argv[i + 1][0] != '-') dn.iterations = atoi(argv[++i]);
        } else if (!strcmp(argv[i], "-vdenoise")) {
            vdenoise = 1;
            if (i + 1 < argc && argv[i + 1][0] != '-') vdn.iterations = atoi(argv[++i]);
        } else if (!strcmp(argv[i], "-adaptive") && i + 1 < argc) {
            adaptive = 1;
            adp.tolerance = (float)atof(argv[++i]);
        } else if (!strcmp(argv[i], "-queue")) {
            queue = 1;
        } else if (!strcmp(argv[i], "-packed")) {
            packed = 1;
        } else if (!strcmp(argv[i], "-move") && i + 3 < argc) {
            mx = atof(argv[++i]);
            my = atof(argv[++i]);
            mz = atof(argv[++i]);
        } else {
            fprintf(stderr, "usage: %s [-w W] [-s spp] [-b bounces] [-ao I] [-o out.ppm] "
                            "[-obj f.obj -mtl f.mtl [-move x y z]] [-devices N] [-denoise [iterations]] "
                            "[-vdenoise [iterations]] [-adaptive TOL] [-queue] [-packed]\n"
                            "  -queue: -vdenoise and -adaptive sample on the task-queue kernel (same frame)\n"
                            "  -packed: the canva leaves the device at 4 bytes a pixel (same frame)\n"
                            "  -adaptive with -vdenoise: the adaptive frame, filtered with each pixel's own sample count\n",
                    argv[0]);
            return 2;
        }
    }
    double ratio = 4.0 / 3.0;
    int H = (int)(W / ratio);
    /* README.md:46-59 sphere list, alpha = 1, materialIndex = 1 */
    rt_sphere spheres[] = {
        {C3(-501, 0, 0), 500, MAT(C3(0, 1, 0), C3(0, 0, 0), 0.0, 0.96)},
        {C3(0, -501, 0), 500, MAT(C3(1, 1, 1), C3(0, 0, 0), 0.0, 0.0)},
        {C3(501, 0, 0), 500, MAT(C3(1, 0, 0), C3(0, 0, 0), 0.0, 0.96)},
        {C3(-0.5, 1.4, -1.2), 0.5, MAT(C3(0, 0, 0), C3(1.0, 0.6, 0.2), 4.0, 0.0)},
        {C3(0.5, 1.4, -2.2), 0.5, MAT(C3(0, 0, 0), C3(0.7, 0.2, 1.0), 4.0, 0.0)},
        {C3(0.6, -1.4, -1.0), 0.5, MAT(C3(0, 0, 0), C3(0.55, 0.863, 1.0), 2.5, 0.0)},
        {C3(-0.5, -1.4, -3.1), 0.5, MAT(C3(0, 0, 0), C3(0.431, 1.0, 0.596), 2.5, 0.0)},
        {C3(0, 0, -504), 500, MAT(C3(1, 1, 1), C3(0, 0, 0), 0.0, 0.0)},
        {C3(0, 501, 0), 500, MAT(C3(1, 1, 1), C3(0, 0, 0), 0.0, 0.0)},
        {C3(0.4, -0.5, -3.3), 0.5, MAT(C3(0.784, 0.965, 1), C3(0, 0, 0), 0.0, 0.99)},
    };
    rt_scene scene;
    memset(&scene, 0, sizeof scene);
    scene.sphere_list = spheres;
    scene.nbSpheres = (int)(sizeof spheres / sizeof spheres[0]);
    rt_mesh mesh;
    memset(&mesh, 0, sizeof mesh);
    rt_material* mats = NULL;
    if (obj) {
        int rc = rt_host_load_obj(obj, mtl, RT_OBJ_COMPAT_QUADS, &mesh);
        if (rc) { fprintf(stderr, "cannot load %s (%d)\n", obj, rc); return 1; }
        rt_host_move_mesh(mx, my, mz, mesh.triangles, mesh.nbTriangles);
        int tw, th;
        rc = rt_host_load_textures(&mesh, 1, &mats, &tw, &th);
        if (rc) { fprintf(stderr, "cannot load textures (%d)\n", rc); return 1; }
        scene.triangle_list = mesh.triangles;
        scene.nbTriangles = mesh.nbTriangles;
        scene.quelMatPourTri = mesh.quelMatPourTri;
        scene.nbMaterials = mesh.nbMaterials;
        scene.mat_list = mats;
        scene.tex_width = tw;
        scene.tex_height = th;
        printf("%s : %d triangles, %d materials (%dx%d texels)\n", obj, mesh.nbTriangles, mesh.nbMaterials, tw, th);
    }
    rt_point3 origin = C3(0.34, 0.3, 0.5), target = C3(0.0, -0.5, -3);
    rt_vec3 up = C3(0, 1, 0);
    rt_params p;
    rt_params_init(&p);
    p.largeur_image = W;
    p.hauteur_image = H;
    p.nbRayonParPixel = spp;
    p.nbRebondMax = bounces;
    p.cam = rt_host_init_camera(origin, target, up, 70, ratio);
    p.focus_distance = 3;
    p.useAO = useAO;
    p.AO_intensity = AO;

    if (ndev > 1) {
        int devs[64];
        for (int i = 0; i < ndev && i < 64; i++) devs[i] = i;
        if (rt_init(ndev, devs)) { fprintf(stderr, "rt_init: %s\n", rt_last_error()); return 1; }
    }
    if (denoise) {      /* main.c:455 with useDenoiser: the built-in filter instead of OIDN */
        if (rt_set_denoise_params(&dn)) { fprintf(stderr, "-denoise: %s\n", rt_last_error()); return 1; }
        rt_set_denoise_hook(rt_denoise_atrous);
    }
    if (queue && (vdenoise || adaptive)) rt_set_accumulate_queue(1);
    if (packed) {
        rt_set_fill_packed_canva(1);
        p.gather |= RT_GATHER_PACKED_CANVA;
    }
    size_t n = (size_t)W * H;
    rt_color* canva = (rt_color*)calloc(n, sizeof(rt_color));
    rt_color* albedo = (rt_color*)calloc(n, sizeof(rt_color));
    rt_color* normal = (rt_color*)calloc(n, sizeof(rt_color));
    int* rounds = adaptive ? (int*)calloc(n, sizeof(int)) : NULL;
    struct timeval t0, t1;
    gettimeofday(&t0, NULL);
    const char* entry = adaptive && vdenoise ? "rt_render_adaptive_vdenoised"
                        : adaptive           ? "rt_render_adaptive"
                        : vdenoise           ? "rt_render_vdenoised"
                                             : "rt_render_rows";
    int rc = adaptive && vdenoise ? rt_render_adaptive_vdenoised(&scene, &p, &adp, &vdn, canva, albedo, normal, rounds)
             : adaptive           ? rt_render_adaptive(&scene, &p, &adp, canva, albedo, normal, rounds)
             : vdenoise           ? rt_render_vdenoised(&scene, &p, &vdn, canva, albedo, normal)
                                  : rt_render_rows(&scene, &p, H - 1, 0, canva, albedo, normal);
    gettimeofday(&t1, NULL);
    if (rc) {
        fprintf(stderr, "%s: %s\n", entry, rt_last_error());
        return 1;
    }
    double dt = (t1.tv_sec - t0.tv_sec) + 1e-6 * (t1.tv_usec - t0.tv_usec);
    if (adaptive) {      /* samples of a pixel with k rounds: 2 * first_half * 2^(k-1) */
        double total = 0, share[17] = {0};
        for (size_t i = 0; i < n; i++) {
            int k = rounds[i] < 1 ? 1 : rounds[i] > 16 ? 16 : rounds[i];
            total += (double)adp.first_half * (double)(1 << k);
            share[k] += 1.0 / (double)n;
        }
        fprintf(stderr, "adaptive%s, tolerance %g: %.2f samples per pixel on average; pixels per round count:",
                vdenoise ? " + variance-guided filter" : "", adp.tolerance, total / (double)n);
        for (int k = 1; k <= adp.max_rounds; k++) fprintf(stderr, " %d: %.1f %%", k, 100.0 * share[k]);
        fprintf(stderr, "\n%dx%d, %d bounces: %.3f s, %.1f Msamples/s (end-to-end)\n", W, H, bounces, dt, total / dt / 1e6);
        free(rounds);
    } else {
        fprintf(stderr, "%dx%d, %d spp, %d bounces: %.3f s, %.1f Msamples/s (end-to-end)\n", W, H, spp, bounces, dt,
                (double)n * spp / dt / 1e6);
    }
    rc = rt_host_write_ppm(out, canva, W, H);
    free(canva);
    free(albedo);
    free(normal);
    free(mats);
    rt_host_free_mesh(&mesh);
    return rc ? 1 : 0;
}
