// Host check of the launch plan (rt_launch_plan.cpp): reads a scene as text on
// stdin (scene_text.h, the reader of scene_prep_check.cpp), prepares it, and for
// each trailing section
//   params KEY VALUE ... end
// calls fill_kparams on the HostScene, then plan_render, and prints one JSON line
// {"rc": 0, "plans": [...]} with one record per section.  Keys (all optional):
// W H spp bounces chunks useAO AO compat semantics accel sky_mode ox oy oz (camera
// origin) aperture_x aperture_y rows (local rows, default H) accumulate count
// accumulate_queue (rt_set_accumulate_queue's switch, default 0).
// In place of the scene sections,
//   facts KEY VALUE ... end
// gives the scalars the plan depends on with no scene: ns nt bvh_nodes bvh_depth
// bvh_stack4 bvh_wide r_scene sph_bound sph_opaque tri_opaque, and bvh bvhh bvhw
// sky (1: the array exists).  With the argument "variants" it reads nothing and
// prints the queue kernel's table (rt_queue_variants.h) as one JSON line
// {"variants": [{"qb", "opq", "name", "stack"}, ...]}.  Used by tests/test_launch_plan.py.
#include <cmath>
#include <cstring>
#include "rt_launch_plan.h"
#include "scene_text.h"
using namespace rt;

// KEY VALUE ... end
static bool pair(std::string& key, double& value)
{
    key = next();
    if (key == "end") return false;
    value = num();
    return true;
}

static void read_facts(HostScene& hs)
{
    SceneFacts& f = hs.facts;
    f.coord_max = 0.0;
    f.mats_bounded = true;
    std::string k;
    for (double v; pair(k, v);) {
        if (k == "ns") f.ns = (int)v, f.ns_pad = ((int)v + 1) & ~1;
        else if (k == "nt") f.nt = (int)v;
        else if (k == "bvh_nodes") f.bvh_nodes = (int)v;
        else if (k == "bvh_depth") f.bvh_depth = (int)v;
        else if (k == "bvh_stack4") f.bvh_stack4 = (int)v;
        else if (k == "bvh_wide") f.bvh_wide = v != 0;
        else if (k == "r_scene") f.r_scene = v;
        else if (k == "sph_bound") f.sph_bound = v;
        else if (k == "sph_opaque") f.sph_opaque = v != 0;
        else if (k == "tri_opaque") f.tri_opaque = v != 0;
        else if (k == "bvh") hs.bvh.resize(v != 0);
        else if (k == "bvhh") hs.bvhh.resize(v != 0);
        else if (k == "bvhw") hs.bvhw.resize(v != 0);
        else if (k == "sky") hs.sky.resize(v != 0);
        else std::fprintf(stderr, "launch_plan_check: unknown fact %s\n", k.c_str()), std::exit(2);
    }
}

// fill_kparams and plan_render on hs under one params section's values.
static void put_plan(const HostScene& hs)
{
    rt_params p;
    std::memset(&p, 0, sizeof p);
    p.largeur_image = 40, p.hauteur_image = 30, p.nbRayonParPixel = 8, p.nbRebondMax = 6;
    p.spp_chunks = 4, p.compat_int_truncation = 1, p.AO_intensity = 2.5, p.focus_distance = 3.0;
    int rows = -1;
    bool accumulate = false, count = false, accumulate_queue = false;
    std::string k;
    for (double v; pair(k, v);) {
        if (k == "W") p.largeur_image = (int)v;
        else if (k == "H") p.hauteur_image = (int)v;
        else if (k == "spp") p.nbRayonParPixel = (int)v;
        else if (k == "bounces") p.nbRebondMax = (int)v;
        else if (k == "chunks") p.spp_chunks = (int)v;
        else if (k == "useAO") p.useAO = (int)v;
        else if (k == "AO") p.AO_intensity = v;
        else if (k == "compat") p.compat_int_truncation = (int)v;
        else if (k == "semantics") p.semantics = (int)v;
        else if (k == "accel") p.accel = (int)v;
        else if (k == "sky_mode") p.sky_mode = (int)v;
        else if (k == "ox") p.cam.origin.e[0] = v;
        else if (k == "oy") p.cam.origin.e[1] = v;
        else if (k == "oz") p.cam.origin.e[2] = v;
        else if (k == "aperture_x") p.ouverture_x = v;
        else if (k == "aperture_y") p.ouverture_y = v;
        else if (k == "rows") rows = (int)v;
        else if (k == "accumulate") accumulate = v != 0;
        else if (k == "count") count = v != 0;
        else if (k == "accumulate_queue") accumulate_queue = v != 0;
        else std::fprintf(stderr, "launch_plan_check: unknown param %s\n", k.c_str()), std::exit(2);
    }
    const rt_tiling t = {0, rows < 0 ? p.hauteur_image : rows, 0, 1, 1};
    KParams kp;
    double uni[U_COUNT];
    fill_kparams(hs, hs.facts, &p, &t, true, kp, uni);
    double sums = 0.0;
    if (accumulate) kp.sums = &sums;                 // (rt_accumulate_async; never read here)
    kp.acc_queue = accumulate_queue ? 1 : 0;
    const RenderPlan pl = plan_render(kp, count);
    std::printf("{\"name\": \"%s\", \"queue\": %d, \"qb\": %d, \"opq\": %d, \"sky\": %d, \"ao\": %d, "
                "\"cuda\": %d, \"bvh\": %d, \"wide\": %d, \"stack_cap\": %d, \"task_ok\": %d, \"band_rows\": %d, "
                "\"partial_bytes\": %zu, \"chunks\": %d, \"bvh_stack\": %d, \"bvh_steps\": %d, \"bvh_far\": %d, "
                "\"zero_exit\": %d, \"tex_const\": %d, \"cam_pin\": %d, \"ns_cand\": %d}",
                pl.name, pl.queue, pl.qb, pl.opq, pl.sky, pl.ao, pl.cuda, pl.bvh, pl.wide, pl.stack_cap, pl.task_ok,
                pl.band_rows, pl.partial_bytes, kp.chunks, kp.bvh_stack, kp.bvh_steps, kp.bvh_far, kp.zero_exit,
                kp.tex_const, kp.cam_pin, kp.ns_cand);
}

// ... under each params section that is left ("params" itself was read).
static void put_plans(const HostScene& hs)
{
    std::printf("\"plans\": [");
    for (bool more = true; more;) {
        put_plan(hs);
        more = g_pos < g_tok.size() && std::string(next()) == "params";
        std::printf(more ? ", " : "]}\n");
    }
}

static void put_variants()
{
    std::printf("{\"variants\": [");
    for (int i = 0; i < kQueueVariantCount; ++i) {
        const QueueVariant& v = kQueueVariants[i];
        std::printf("%s{\"qb\": %d, \"opq\": %d, \"name\": \"%s\", \"stack\": %d}", i ? ", " : "", v.qb, v.opq, v.name,
                    v.stack);
    }
    std::printf("]}\n");
}

int main(int argc, char** argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "variants")) {
        put_variants();
        return 0;
    }
    read_tokens();
    HostScene hs;
    std::string what = next();
    if (what == "facts") {
        read_facts(hs);
        what = next();
    } else {
        --g_pos;
        SceneText st;
        what = st.read();
        std::string err;
        const int rc = prepare_scene(&st.sc, hs, err);
        if (rc != RT_OK) {
            std::printf("{\"rc\": %d, \"error\": \"%s\"}\n", rc, err.c_str());
            return 0;
        }
    }
    if (what != "params") {
        std::fprintf(stderr, "launch_plan_check: a params section is needed, got \"%s\"\n", what.c_str());
        return 2;
    }
    std::printf("{\"rc\": 0, ");
    put_plans(hs);
    return 0;
}
