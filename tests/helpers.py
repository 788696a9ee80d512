"""Shared scene builders and oracle/product drivers for the tests."""
import ctypes as C
import hashlib

import numpy as np

import oracle_ffi
import tipe_rt
from tipe_rt import scenes
from tipe_rt.types import Sphere, Triangle, Material, Vec3, UV, RT_RNG_PHILOX


class SceneBundle:
    """Keeps the ctypes arrays alive next to the rt_scene that points at them."""

    def __init__(self, spheres=None, mesh=None, sky=None):
        self.spheres = spheres
        self.mesh = mesh
        self.sky = sky
        if mesh is not None:
            tris, qm, mats, tw, th, nm = mesh
            self.scene = tipe_rt.make_scene(spheres, tris, qm, mats, tw, th, nm, sky=sky)
        else:
            self.scene = tipe_rt.make_scene(spheres, sky=sky)


def spheres_plus(spheres, rows):
    """A new Sphere array: the given spheres, then one per row, last.  A row
    is (center, radius, Material) or a Sphere."""
    rows = list(rows)
    n = len(spheres)
    arr = (Sphere * (n + len(rows)))()
    for k in range(n):
        arr[k] = spheres[k]
    for k, row in enumerate(rows, n):
        if isinstance(row, Sphere):
            arr[k] = row
        else:
            arr[k].center = Vec3(*[float(x) for x in row[0]])
            arr[k].radius = row[1]
            arr[k].mat = row[2]
    return arr


def sphere_array(rows):
    """(center, radius, Material) rows -> a Sphere array."""
    return spheres_plus((), rows)


def mesh_of(mesh, nt):
    """The mesh tuple with its own arrays of nt triangles and material
    indices: the first nt of the mesh's, zeros beyond them (the texels are
    shared)."""
    tris, qm, mats, tw, th, nm = mesh
    t2, q2 = (Triangle * nt)(), (C.c_int * nt)()
    keep = min(nt, len(tris))
    C.memmove(t2, tris, C.sizeof(Triangle) * keep)
    C.memmove(q2, qm, C.sizeof(C.c_int) * keep)
    return t2, q2, mats, tw, th, nm


def mesh_plus_triangle(mesh, A, B, Cc):
    """A copy of the mesh with the triangle A B C (material index 0) appended."""
    n = len(mesh[0])
    out = mesh_of(mesh, n + 1)
    for P, xyz in zip((out[0][n].A, out[0][n].B, out[0][n].C), (A, B, Cc)):
        P.e[0], P.e[1], P.e[2] = xyz
    return out


def mesh_rows(tris):
    """Triangle array -> (n, 9) array of A, B, C."""
    return np.array([[t.A.e[0], t.A.e[1], t.A.e[2], t.B.e[0], t.B.e[1], t.B.e[2], t.C.e[0], t.C.e[1], t.C.e[2]]
                     for t in tris])


def cornell(extra=()):
    return SceneBundle(scenes.cornell_spheres(extra=extra))


def pyramid_scene(move=scenes.PYRAMID_MOVE):
    return SceneBundle(scenes.cornell_spheres(), scenes.moved(scenes.load_mesh_fixture("pyramide"), move))


def sky_scene(w=16, h=8, seed=3):
    """README spheres + an enclosing emissive sky sphere (the last sphere,
    main.c:64-71) with a w x h equirect texel table of random colours."""
    sph = spheres_plus(scenes.cornell_spheres(),
                       [((0.0, 0.0, 0.0), 2000.0, scenes.material((0.5, 0.5, 0.5), (1, 1, 1), 1.2, 0.0, 1.0, 1.0))])
    rng = np.random.default_rng(seed)
    tex = (Material * (w * h))()
    for k in range(w * h):
        tex[k] = scenes.material(tuple(rng.uniform(0, 1, 3)), (0, 0, 0), 0.0, 0.0, 1.0, 0.0)
    return SceneBundle(sph, None, sky=(tex, w, h))


def sky_tree_scene():
    """The sky scene's spheres and texels with the C4 tree mesh (BVH + sky)."""
    sk = sky_scene()
    return SceneBundle(sk.spheres, scenes.moved(scenes.load_tree_fixture(), scenes.TREE_MOVE), sky=sk.sky)


def mineways_scene():
    """mineways_tri.obj (606 triangles, 11 textures incl. alpha leaves) scaled
    into the README box (as test_gpu_parity.test_mineways_alpha_holes)."""
    tris, qm, mats, tw, th, nm = scenes.load_mesh_fixture("mineways")
    for t in tris:
        for P in (t.A, t.B, t.C):
            P.e[0] = P.e[0] * 0.1 - 0.2
            P.e[1] = P.e[1] * 0.1 - 1.0
            P.e[2] = P.e[2] * 0.1 - 2.5
    return SceneBundle(scenes.cornell_spheres(), (tris, qm, mats, tw, th, nm))


def tree_scene(move=scenes.TREE_MOVE):
    """C4: README spheres + 1tree_tri.obj (1320 tris, Kd-flat materials)."""
    return SceneBundle(scenes.cornell_spheres(), scenes.moved(scenes.load_tree_fixture(), move))


def camera_of(spec):
    """scenes.*_CAMERA dict -> the oracle's init_camera (camera.h:21-40)."""
    return oracle_ffi.oracle().oracle_init_camera(Vec3(*spec["origin"]), Vec3(*spec["target"]), Vec3(*spec["up"]),
                                                  spec["vfov"], spec["ratio"])


def nature_scene():
    """RTX_MAP/nature (5812 textured triangles with alpha holes) lit by
    main.c:345-346's sun and sky sphere; camera scenes.NATURE_CAMERA."""
    return SceneBundle(scenes.main_spheres(), scenes.nature_mesh())


def main_regime_scene():
    """main()'s own coordinate regime: its default mesh pyramide_eau/scene.obj
    (+-1813 units, materials 1/3/4 = texture.h:71-87's light / glass / water
    overrides) under main.c:345-346's sun and radius-1e5 sky sphere; camera
    scenes.MAIN_CAMERA (main.c:298-302)."""
    return SceneBundle(scenes.main_spheres(), scenes.pyramide_eau_mesh())


def params(W, H, spp, bounces, use_ao=False, ao=2.5, rng=RT_RNG_PHILOX, seed=1010, compat=1, cam=None,
           aperture=(0.0, 0.0), focus=3.0, chunks=1, accel=0, sky_mode=0, semantics=0):
    if cam is None:
        cam = camera_of(scenes.README_CAMERA)
    return tipe_rt.make_params(W, H, spp, bounces, cam, focus=focus, aperture=aperture, use_ao=use_ao, ao=ao,
                               seed=seed, rng=rng, compat=compat, chunks=chunks, accel=accel, sky_mode=sky_mode,
                               semantics=semantics)


def oracle_render(bundle, p, row_hi=None, row_lo=0, nthreads=1, counters=False, zero_exit=False):
    """zero_exit: the oracle's restatement of the zero-throughput exit
    (rt_oracle.h oracle_set_zero_exit) for this call; off again afterwards."""
    W, H = p.largeur_image, p.hauteur_image
    if row_hi is None:
        row_hi = H - 1
    canva, alb, nrm, rad = (np.zeros((H, W, 3)) for _ in range(4))
    cnt = oracle_ffi.counters() if counters else None
    lib = oracle_ffi.oracle()
    lib.oracle_set_zero_exit(1 if zero_exit else 0)
    try:
        rc = lib.oracle_render_rows(C.byref(bundle.scene), C.byref(p), row_hi, row_lo, nthreads, 1,
                                    canva.ctypes.data, alb.ctypes.data, nrm.ctypes.data, rad.ctypes.data, cnt)
    finally:
        lib.oracle_set_zero_exit(0)
    assert rc == 0, rc
    out = dict(canva=canva, albedo=alb, normal=nrm, radiance=rad)
    if counters:
        out["counters"] = np.array(list(cnt), dtype=np.uint64)
    return out


def ppm_text(canva):
    """The P3 file main.c:457-465 writes (rows top to bottom: j = H-1 .. 0)."""
    H, W, _ = canva.shape
    lines = ["P3\n%d %d\n255\n" % (W, H)]
    for j in range(H - 1, -1, -1):
        row = canva[j].astype(np.int64)
        lines.extend("%d %d %d\n" % (r, g, b) for r, g, b in row)
    return "".join(lines)


def ppm_md5(canva):
    return hashlib.md5(ppm_text(canva).encode()).hexdigest()


def rmse_per_channel(a, b):
    d = (np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).reshape(-1, 3)
    return np.sqrt((d * d).mean(axis=0))


def adversarial_sphere_scene():
    """Sphere pairs the candidate pass cannot separate (spheres_closest):
    an exact duplicate (equal t: the reference keeps the first), a sphere
    1e-12 larger than its neighbour, spheres touching each other and the
    floor, a tiny sphere and a huge far one.  Each must fall back to the
    exact scan or be resolved exactly."""
    m = scenes.material
    extra = [
        ((0.3, 0.2, -2.5), 0.3, m((1, 0, 0))),
        ((0.3, 0.2, -2.5), 0.3, m((0, 1, 0), refl=0.5)),                 # duplicate: first wins
        ((-0.4, 0.1, -2.0), 0.25, m((0, 0, 1))),
        ((-0.4, 0.1, -2.0), 0.25 + 1e-12, m((1, 1, 0))),                  # 1e-12 apart
        ((0.0, -0.5, -1.8), 0.5, m((0.9, 0.9, 0.9), refl=0.9)),          # touches the floor (y = -1)
        ((0.5, -0.5, -1.8), 0.5, m((0.2, 0.8, 0.5))),        # touches the previous one
        ((0.05, 0.3, -1.2), 1e-4, m((1, 1, 1), (1, 1, 1), 3.0)),         # tiny emitter
        ((0.0, 0.0, -2e4), 1e4, m((0.5, 0.5, 0.5))),                     # huge, far
    ]
    return cornell(extra)


def stress_rays(spheres, n, seed):
    """Rays that stress the candidate pass's bound: origins on sphere surfaces
    (as a bounce leaves them), directions near tangent at 1e-3..1e-12, rays
    aimed at silhouettes (disc ~ 0), unnormalised directions, far origins."""
    rng = np.random.default_rng(seed)
    C_ = np.array([[s.center.e[0], s.center.e[1], s.center.e[2]] for s in spheres])
    R_ = np.array([s.radius for s in spheres])

    def unit(v):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)
    m = n // 5
    k = rng.integers(0, len(R_), m)
    # 1. surface origins, random and near-tangent directions
    nrm = unit(rng.normal(size=(m, 3)))
    o1 = C_[k] + R_[k, None] * nrm
    tan = unit(np.cross(nrm, rng.normal(size=(m, 3))))
    eps = rng.choice([0.0, 1e-3, 1e-6, 1e-9, 1e-12], m)[:, None] * rng.choice([-1.0, 1.0], (m, 1))
    d1 = np.where(rng.random((m, 1)) < 0.5, unit(rng.normal(size=(m, 3))), tan + eps * nrm)
    # 2. silhouette rays from random box points
    o2 = rng.uniform([-1, -1, -4], [1, 1, 0.5], (m, 3))
    k2 = rng.integers(0, len(R_), m)
    w = C_[k2] - o2
    perp = unit(np.cross(w, rng.normal(size=(m, 3))))
    d2 = (C_[k2] + R_[k2, None] * perp * (1 + rng.choice([0, 1e-9, -1e-9, 1e-14], m)[:, None])) - o2
    # 3. random rays, 4. unnormalised, 5. far origins
    o3 = rng.uniform([-1, -1, -4], [1, 1, 0.5], (m, 3))
    d3 = unit(rng.normal(size=(m, 3)))
    d4 = unit(rng.normal(size=(m, 3))) * 10.0 ** rng.uniform(-3, 3, (m, 1))
    o5 = unit(rng.normal(size=(m, 3))) * rng.uniform(10, 2000, (m, 1))
    d5 = unit(rng.uniform(-1, 1, (m, 3)) - o5)
    o = np.concatenate([o1, o2, o3, o3, o5])
    d = np.concatenate([d1, d2, d3, d4, d5])
    return np.concatenate([o, d], axis=1)


def _zero_some(rng, c, zeros):
    """With zeros, each colour channel is exactly 0 with probability 0.35,
    so rayColor reaches (0, 0, 0) and the zero-throughput exit runs."""
    if not zeros:
        return c
    return tuple(0.0 if rng.random() < 0.35 else float(x) for x in c)


def random_scene(seed, zeros=False, chunks=None, nt_range=None, spp=None, opaque=False, mesh_p=0.7,
                 bounce_hi=25, far=False):
    """bounce_hi: nbRebondMax is drawn from [0, bounce_hi), covering main.c's
    own default of 20 (main.c:310); the scenes pinned by reference fixtures
    (tests/composition_cases._random) keep the r05 draw, bounce_hi 9.
    far: the scene moved into main()'s coordinate regime (below).
    opaque: only opaque materials (no glass or hole spheres, texels at
    alpha 1, no material index 3 or 4), the scenes the queue kernel's
    opaque instantiations take (QB -2, the deep-tree OPQ kernel);
    mesh_p: probability of a mesh when nt_range is None."""
    rng = np.random.default_rng(seed)
    ns = int(rng.integers(1, 14))
    sph = (Sphere * ns)()
    for k in range(ns):
        kind = rng.choice(["diffuse", "mirror", "light", "big"] if opaque
                          else ["diffuse", "mirror", "glass", "hole", "light", "big"])
        c = rng.uniform([-2, -2, -6], [2, 2, -1])
        r = rng.uniform(0.2, 1.2)
        diff = _zero_some(rng, tuple(rng.uniform(0, 1, 3)), zeros)
        em, es, refl, alpha, ior = (0, 0, 0), 0.0, 0.0, 1.0, 1.0
        if kind == "mirror":
            refl = float(rng.uniform(0.5, 1.0))
        elif kind == "glass":
            alpha, ior = float(rng.uniform(0.05, 0.99)), float(rng.uniform(1.0, 2.0))
        elif kind == "hole":
            alpha = 0.0
        elif kind == "light":
            em, es = tuple(rng.uniform(0.2, 1, 3)), float(rng.uniform(0.5, 5))
        elif kind == "big":                               # encloses the camera
            c, r = rng.uniform(-0.5, 0.5, 3), float(rng.uniform(20, 600))
        sph[k].center = Vec3(*c)
        sph[k].radius = r
        sph[k].mat = scenes.material(diff, em, es, refl, alpha, ior)
    mesh = None
    if nt_range is not None or rng.random() < mesh_p:
        nt = int(rng.integers(40, 120)) if seed % 2 else int(rng.integers(1, 20))
        if nt_range is not None:
            nt = int(rng.integers(*nt_range))
        tris = (Triangle * nt)()
        nm, tw, th = 5, int(rng.integers(1, 5)), int(rng.integers(1, 5))
        qm = (C.c_int * nt)(*[int(x) for x in (rng.choice([0, 1, 2], nt) if opaque else rng.integers(0, nm, nt))])
        for k in range(nt):
            A = rng.uniform([-2, -2, -5], [2, 2, -1.5])
            e = rng.normal(size=(2, 3)) * 0.5
            tris[k].A, tris[k].B, tris[k].C = Vec3(*A), Vec3(*(A + e[0])), Vec3(*(A + e[1]))
            tris[k].uvA, tris[k].uvB, tris[k].uvC = (UV(*rng.uniform(-2, 2, 2)) for _ in range(3))
        mats = (Material * (nm * tw * th))()
        for k in range(nm * tw * th):
            mats[k] = scenes.material(_zero_some(rng, tuple(rng.uniform(0, 1, 3)), zeros), (0, 0, 0), 0.0, 0.0,
                                      1.0 if opaque else float(rng.choice([0.0, 0.5, 1.0, 0.7])), 0.0)
        mesh = (tris, qm, mats, tw, th, nm)
    cam_o, cam_t = rng.uniform(-0.5, 0.5, 3), rng.uniform([-1, -1, -4], [1, 1, -2])
    vfov = float(rng.uniform(40, 100))
    W, H = int(rng.integers(8, 33)), int(rng.integers(6, 25))
    spp_b = (int(rng.integers(1, 6)), int(rng.integers(0, bounce_hi)))
    use_ao, ao, rseed = bool(rng.random() < 0.4), float(rng.uniform(0.5, 3.5)), int(rng.integers(0, 2 ** 40))
    aperture, focus = tuple(rng.choice([0.0, 0.0, 1.0, 2.0], 2)), float(rng.uniform(1, 5))
    compat, chunks_d = int(rng.integers(0, 2)), int(rng.choice([1, 1, 2, 3]))
    if far:
        # main()'s coordinate regime (camera at |o| ~ 1000, main.c:300-301;
        # sky sphere of radius 1e5, main.c:346): the whole scene scaled by s
        # and moved by T, then enclosed by an emissive radius-1e5 sky
        s, T = float(rng.uniform(50, 2000)), rng.uniform(-1000, 1000, 3)
        for k in range(ns):
            sph[k].center = Vec3(*(T + s * np.array(sph[k].center.tolist())))
            sph[k].radius = s * sph[k].radius
        if mesh is not None:
            for t in mesh[0]:
                t.A, t.B, t.C = (Vec3(*(T + s * np.array(P.tolist()))) for P in (t.A, t.B, t.C))
        cam_o, cam_t = T + s * cam_o, T + s * cam_t
        focus *= s
        sph = spheres_plus(sph, [((0.0, 0.0, 0.0), 1e5, scenes.material((0, 0, 0), scenes.SKY, 1.0, 0.0, 1.0, 1.0))])
    bundle = SceneBundle(sph, mesh)
    cam = tipe_rt.init_camera(tuple(cam_o), tuple(cam_t), (0, 1, 0), vfov, 4.0 / 3.0)
    p = params(W, H, *spp_b, use_ao=use_ao, ao=ao, seed=rseed, cam=cam, aperture=aperture, focus=focus,
               compat=compat, chunks=chunks_d)
    if chunks is not None:
        p.spp_chunks = chunks
        p.nbRayonParPixel = max(p.nbRayonParPixel, chunks)
    if spp is not None:
        p.nbRayonParPixel = spp
    return bundle, p
