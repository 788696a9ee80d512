// rt_diag.cpp — the C-ABI's diagnostics: rt_selftest_math and the
// rt_verify_* counters (rt_verify.h kernels), each on the first rt_init device.
#include <memory>

#include "rt_api_internal.h"

using namespace rt;

namespace {

typedef unsigned long long u64;

// Zeroes two device counters, runs launch(d_counts), waits for the device and
// copies the counters back.
template <class F>
hipError_t run_counted(u64 counts[2], const F& launch)
{
    DevArray<u64> d;
    hipError_t e = d.alloc(2);
    if (e == hipSuccess) e = hipMemset(d, 0, 2 * sizeof(u64));
    if (e == hipSuccess) e = (hipError_t)launch((u64*)d);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(counts, d, 2 * sizeof(u64), hipMemcpyDeviceToHost);
    return e;
}

typedef std::unique_ptr<rt_device_scene, void (*)(rt_device_scene*)> ScenePtr;

}  // namespace

extern "C" {

int rt_selftest_math(int op, const double* in, double* out, int n)
{
    if (!in || !out || n < 0 || op < 0 || op > 9) return fail(RT_EINVAL, "bad selftest arguments");
    if (n == 0) return RT_OK;
    int dev = 0, rc;
    if ((rc = first_device(dev))) return rc;
    DeviceGuard guard(dev);
    const size_t nin = (size_t)n * (op == 7 ? 6 : op == 8 ? 3 : (op == 3 || op == 5 || op == 9) ? 2 : 1);
    const size_t nout = (size_t)n * (op == 7 ? 4 : op == 8 ? 3 : 1);
    DevArray<double> d_in, d_out;
    hipError_t e = d_in.upload(in, nin);
    if (e == hipSuccess) e = d_out.alloc(nout);
    if (e == hipSuccess) e = (hipError_t)launch_selftest(op, d_in, d_out, n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, nout * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(RT_EDEVICE, "selftest: %s", hipGetErrorString(e));
    return RT_OK;
}

int rt_verify_sphere_pass(const rt_scene* scene, const double* rays, long long n, unsigned long long counts[2])
{
    if (!counts || !rays || n < 0) return fail(RT_EINVAL, "bad verify arguments");
    counts[0] = counts[1] = 0;
    if (n == 0) return RT_OK;
    int dev = 0, rc;
    if ((rc = first_device(dev))) return rc;
    rt_device_scene* raw = nullptr;
    if ((rc = rt_scene_upload(dev, scene, &raw))) return rc;
    ScenePtr ds(raw, free_scene);
    DeviceGuard guard(dev);
    KParams kp = {};
    set_sphere_fields(kp, *ds, ds->facts);
    DevArray<double> d_rays;
    hipError_t e = d_rays.upload(rays, (size_t)n * 6);
    if (e == hipSuccess) e = run_counted(counts, [&](u64* d) { return launch_verify_spheres(kp, d_rays, n, d); });
    if (e != hipSuccess) return fail(RT_EDEVICE, "verify_sphere_pass: %s", hipGetErrorString(e));
    return RT_OK;
}

int rt_verify_texel_map(const rt_scene* scene, const double* pts, const int* tri, long long n,
                        unsigned long long counts[2])
{
    if (!counts || !pts || !tri || n < 0 || !scene) return fail(RT_EINVAL, "bad verify arguments");
    counts[0] = counts[1] = 0;
    if (scene->nbTriangles < 1 || scene->nbTriangles > 32)
        return fail(RT_EUNSUPPORTED, "verify_texel_map: 1-32 triangles (caller order), got %d", scene->nbTriangles);
    for (long long i = 0; i < n; ++i)
        if (tri[i] < 0 || tri[i] >= scene->nbTriangles) return fail(RT_EINVAL, "tri[%lld] = %d", i, tri[i]);
    if (n == 0) return RT_OK;
    int dev = 0, rc;
    if ((rc = first_device(dev))) return rc;
    rt_device_scene* raw = nullptr;
    if ((rc = rt_scene_upload(dev, scene, &raw))) return rc;
    ScenePtr ds(raw, free_scene);
    if (!ds->tri_uv)
        return fail(RT_EUNSUPPORTED, "verify_texel_map: the scene has no affine texel map (every uv 0)");
    DeviceGuard guard(dev);
    KParams kp = {};
    set_triangle_fields(kp, *ds, ds->facts);
    DevArray<double> d_pts;
    DevArray<int> d_tri;
    hipError_t e = d_pts.upload(pts, (size_t)n * 3);
    if (e == hipSuccess) e = d_tri.upload(tri, (size_t)n);
    if (e == hipSuccess) e = run_counted(counts, [&](u64* d) { return launch_verify_texel(kp, d_pts, d_tri, n, d); });
    if (e != hipSuccess) return fail(RT_EDEVICE, "verify_texel_map: %s", hipGetErrorString(e));
    return RT_OK;
}

int rt_verify_sampler_phi(unsigned long long r0, unsigned long long n, unsigned long long counts[2])
{
    if (!counts || r0 > (1ull << 31) || n > (1ull << 31) - r0) return fail(RT_EINVAL, "bad verify range");
    counts[0] = counts[1] = 0;
    if (n == 0) return RT_OK;
    int dev = 0, rc;
    if ((rc = first_device(dev))) return rc;
    DeviceGuard guard(dev);
    const hipError_t e = run_counted(counts, [&](u64* d) { return launch_verify_phi(r0, n, d); });
    if (e != hipSuccess) return fail(RT_EDEVICE, "verify_sampler_phi: %s", hipGetErrorString(e));
    return RT_OK;
}

int rt_verify_normalize(unsigned long long seed, unsigned long long n, unsigned long long counts[2])
{
    if (!counts) return fail(RT_EINVAL, "verify_normalize: counts is NULL");
    counts[0] = counts[1] = 0;
    if (n == 0) return RT_OK;
    int dev = 0, rc;
    if ((rc = first_device(dev))) return rc;
    DeviceGuard guard(dev);
    const hipError_t e = run_counted(counts, [&](u64* d) { return launch_verify_normalize(seed, n, d); });
    if (e != hipSuccess) return fail(RT_EDEVICE, "verify_normalize: %s", hipGetErrorString(e));
    return RT_OK;
}

}  // extern "C"
