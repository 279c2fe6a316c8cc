"""Scene queries on the GPU (crt_abi.h "scene queries"): BaseScene::IsOccluded through crt_is_occluded / crt_is_occluded_device, and FindNearest on device
buffers through crt_find_nearest_device, enqueued on torch streams.

Expected values come from the oracle (oracle/orc.py) and from the real reference's committed outputs (tests/golden/ref_bvh_rays.npz, ref_alt_rays.npz); the
device-vs-host comparisons are agreement checks between the product's two entries and say so."""
import os
import re

import numpy as np
import pytest

from conftest import ASSETS, GOLDEN, scene_path
from test_gpu_golden_and_edges import write_scene

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("t", "u", "v", "objIdx", "triIdx", "traversed", "tested")
LIGHT = (0.0, 3.0, 1.0)            # write_scene's light position; the floor is the plane y = -1


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def dev():
    return torch.device("cuda", 0)


def ray_records(O, D, inside=None):
    import importlib
    crt = importlib.import_module("cpu_ray_tracer_amd")
    r = np.zeros(len(O), crt.RAY_DTYPE)
    r["O"], r["D"] = O, D
    if inside is not None:
        r["inside"] = inside
    return torch.from_numpy(r.view(np.float32).reshape(-1, 7).copy()).to(dev())


def shadow_records(O, D, t):
    import importlib
    crt = importlib.import_module("cpu_ray_tracer_amd")
    r = np.zeros(len(O), crt.SHADOW_RAY_DTYPE)
    r["O"], r["D"], r["t"] = O, D, t
    return torch.from_numpy(r.view(np.float32).reshape(-1, 7).copy()).to(dev())


def hits_np(crt, h):
    return h.cpu().numpy().view(crt.HIT_DTYPE).reshape(-1)


def assert_hits_equal(a, b, what):
    for f in FIELDS:
        assert np.array_equal(np.asarray(a[f]).view(np.uint32), np.asarray(b[f]).view(np.uint32)), (what, f)


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def camera_rays(n, seed, cam=(0.0, 0.0, -2.0), half=(1.6, 1.0), z=0.0):
    """rays from around the camera position through a window of the z = 0 plane (as GetPrimaryRay's screen plane, jittered)"""
    rng = np.random.default_rng(seed)
    O = np.tile(np.array(cam, np.float32), (n, 1)) + rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32)
    P = np.stack([rng.uniform(-half[0], half[0], n), rng.uniform(-half[1], half[1], n), np.full(n, z)], 1).astype(np.float32)
    return O, unit(P - O)


def up_rays(n, seed, light, xr, zr, y0, y1, spread=0.8):
    """rays from points above the floor and below the light, aimed up at points of the light's plane within `spread` of the quad's centre (the quad's half
    size is 0.5: with 0.8 about a third cross it, with 0.45 all do)"""
    rng = np.random.default_rng(seed)
    O = np.stack([rng.uniform(*xr, n), rng.uniform(y0, y1, n), rng.uniform(*zr, n)], 1).astype(np.float32)
    T = np.stack([light[0] + rng.uniform(-spread, spread, n), np.full(n, light[1]), light[2] + rng.uniform(-spread, spread, n)], 1).astype(np.float32)
    D = unit(T - O)
    assert (D[:, 1] > 0).all() and (D != 0).all()
    return O, D


def quad_occluded(O, D, t, light, size=0.5):
    """Quad::IsOccluded (template/primitives.h:347-362) in float32, operation for operation, for the quad FileScene / TLASFileScene build: T = Translate(light),
    invT = FastInvertedTransformNoScale(T) = identity rotation with translation -light.  Returns (occluded, quad distance)."""
    f = np.float32
    c = np.eye(4, dtype=f)
    c[0, 3], c[1, 3], c[2, 3] = -f(light[0]), -f(light[1]), -f(light[2])
    O = O.astype(f); D = D.astype(f); t = np.asarray(t, f)
    with np.errstate(all="ignore"):
        Oy = ((c[1, 0] * O[:, 0] + c[1, 1] * O[:, 1]) + c[1, 2] * O[:, 2]) + c[1, 3]
        Dy = (c[1, 0] * D[:, 0] + c[1, 1] * D[:, 1]) + c[1, 2] * D[:, 2]
        tq = Oy / -Dy
        Ox = ((c[0, 0] * O[:, 0] + c[0, 1] * O[:, 1]) + c[0, 2] * O[:, 2]) + c[0, 3]
        Oz = ((c[2, 0] * O[:, 0] + c[2, 1] * O[:, 1]) + c[2, 2] * O[:, 2]) + c[2, 3]
        Dx = (c[0, 0] * D[:, 0] + c[0, 1] * D[:, 1]) + c[0, 2] * D[:, 2]
        Dz = (c[2, 0] * D[:, 0] + c[2, 1] * D[:, 1]) + c[2, 2] * D[:, 2]
        Ix = Ox + tq * Dx
        Iz = Oz + tq * Dz
        s = f(size)
        occ = (tq < t) & (tq > 0) & (Ix > -s) & (Ix < s) & (Iz > -s) & (Iz < s)
    return occ, tq


def pick_t(tq):
    """per ray one of: 1e34, the quad distance, and its two float neighbours (a finite positive quad distance only; otherwise 1e34)"""
    ok = np.isfinite(tq) & (tq > 0)
    k = np.arange(len(tq)) % 4
    t = np.full(len(tq), 1e34, np.float32)
    t[ok & (k == 1)] = tq[ok & (k == 1)]
    t[ok & (k == 2)] = np.nextafter(tq[ok & (k == 2)], np.float32(np.inf))
    t[ok & (k == 3)] = np.nextafter(tq[ok & (k == 3)], np.float32(-np.inf))
    return t


def light_of(xml):
    m = re.search(r"<light_position><x>([^<]+)</x><y>([^<]+)</y><z>([^<]+)</z>", open(xml).read())
    return tuple(float(v) for v in m.groups())


def rigid(angle, pos):
    c, s = np.cos(angle), np.sin(angle)
    T = np.array([[c, 0, s, pos[0]], [0, 1, 0, pos[1]], [-s, 0, c, pos[2]], [0, 0, 0, 1]], np.float32)
    return T


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 1. find_nearest_device == the host entries, bit for bit (agreement check), and == the oracle on a subset
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def ray_pool(n=1 << 20):
    z = np.load(os.path.join(GOLDEN, "ref_bvh_rays.npz"))
    Og, Dg = z["bunny_O"], z["bunny_D"]                                  # the real reference's ray set, axis-aligned rays included
    Oc, Dc = camera_rays(n - len(Og) - 6, 11)
    Oa = np.tile(np.array([[0.0, 0.5, -2.0]], np.float32), (6, 1))
    Da = np.array([[0, 0, 1], [0, -1, 0], [1, 0, 0], [0, 0, -1], [0, 1, 0], [-1, 0, 0]], np.float32)
    O = np.concatenate([Og, Oa, Oc]).astype(np.float32); D = np.concatenate([Dg, Da, Dc]).astype(np.float32)
    inside = (np.arange(n) % 5 == 3).astype(np.int32)
    return O, D, inside


@pytest.fixture(scope="module")
def bunny_file(crt, tmp_path_factory):
    xml = write_scene(tmp_path_factory.mktemp("bunny"), "bunny")
    hs = crt.HostScene(xml, 0, ASSETS)
    hs.build_alt(crt.ACCEL_KDTREE); hs.build_alt(crt.ACCEL_GRID)
    ctx = crt.Context(64, 64)
    hs.upload(ctx); hs.upload_alt(ctx, crt.ACCEL_KDTREE); hs.upload_alt(ctx, crt.ACCEL_GRID)
    yield xml, hs, ctx
    ctx.close()


@pytest.mark.parametrize("scene", ["file", "tlas", "kd", "grid", "prim"])
def test_find_nearest_device_equals_host_entry(crt, orc, bunny_file, scene):
    O, D, inside = ray_pool()
    accel = {"kd": crt.ACCEL_KDTREE, "grid": crt.ACCEL_GRID}.get(scene, 0)
    own = None
    if scene in ("file", "kd", "grid"):
        xml, hs, ctx = bunny_file
    elif scene == "tlas":
        xml = scene_path("tlas_scene.xml"); hs = crt.HostScene(xml, 1, ASSETS); ctx = own = crt.Context(64, 64); hs.upload(ctx)
    else:
        xml = None; hs = crt.HostPrimitiveScene(ASSETS); hs.set_time(0.7); ctx = own = crt.Context(64, 64); hs.upload(ctx)
        O = O.copy(); O[:, 2] += 1.5                                      # from inside the room
    rays = ray_records(O, D, inside)
    for n in (1, 63, 65, 3000, 1 << 20):
        if accel:
            host = ctx.find_nearest_alt(accel, O[:n], D[:n])                 # (the host entry has no `inside` column: FindNearest does not read it)
        else:
            host = ctx.find_nearest(O[:n], D[:n], inside[:n])
        ctx.reset_counters(); c_host = None
        if not accel:
            ctx.find_nearest(O[:n], D[:n], inside[:n]); c_host = ctx.counters(); ctx.reset_counters()
        h = ctx.find_nearest_device(rays[:n], accel=accel)
        torch.cuda.current_stream().synchronize()
        assert_hits_equal(hits_np(crt, h), host, (scene, n))
        if c_host is not None:
            assert ctx.counters() == c_host, (scene, n)                   # the same counting as crt_find_nearest
    big = hits_np(crt, h)                                                 # the 2^20-ray launch: every wavefront refills from the cursor, under real contention
    # the O / D form builds the same records
    h2 = ctx.find_nearest_device(O=torch.from_numpy(O[:3000]).to(dev()), D=torch.from_numpy(D[:3000]).to(dev()),
                                 inside=torch.from_numpy(inside[:3000]).to(dev()), accel=accel)
    assert_hits_equal(hits_np(crt, h2), hits_np(crt, ctx.find_nearest_device(rays[:3000], accel=accel)), (scene, "O/D form"))
    f = crt.hit_fields(h2)
    assert f["objIdx"].dtype == torch.int32 and f["t"].dtype == torch.float32
    # against the oracle on a subset (oracle: the scene's BVH / TLAS / PrimitiveScene, no alternative accelerator)
    if scene in ("file", "tlas", "prim"):
        if scene == "prim":
            o = orc.primitive_scene(ASSETS, 0.7)
        else:
            o, _ = orc.load_scene(xml, 1 if scene == "tlas" else 0, ASSETS)
        w = o.find_nearest(O[:4000], D[:4000], inside[:4000])
        got = hits_np(crt, ctx.find_nearest_device(rays[:4000]))
        for fld in ("t", "u", "v", "objIdx", "triIdx"):
            assert np.array_equal(got[fld].view(np.uint32), w[fld].view(np.uint32)), (scene, fld)
    # ... and the 2^20-ray launch, where every lane takes ray after ray, on a strided subset of 8 192 (tests/test_gpu_query_lane_reuse.py: the same with the
    # launch bounded to a few workgroups and the rays in adversarial orders)
    n = 1 << 20
    sub = np.arange(8192) * (n // 8192)
    if scene in ("file", "tlas", "prim"):
        w = o.find_nearest(O[sub], D[sub], inside[sub])
        for fld in (("t", "u", "v", "objIdx", "triIdx") if scene == "prim" else FIELDS):          # (PrimitiveScene counts no traversal steps)
            assert np.array_equal(big[fld][sub].view(np.uint32), w[fld].view(np.uint32)), (scene, "2^20", fld)
    else:
        # the oracle's restatement of the accelerator alone: the whole record where the device reports a miss, the same hit where it reports the mesh
        # (test_gpu_alt_accel.test_alt_accel_edge_cases_and_errors), and the oracle's BVH answer on rays without a zero direction component
        a = orc.alt_accel(scene, hs.bvh(0)["tris"]); w = a.intersect(O[sub], D[sub]); a.close()
        got = big[sub]
        miss, mesh, general = got["objIdx"] == -1, got["objIdx"] >= 2, np.all(D[sub] != 0, axis=1)
        assert miss.sum() > 100 and mesh.sum() > 100
        for fld in FIELDS:
            assert np.array_equal(got[fld][miss].view(np.uint32), w[fld][miss].view(np.uint32)), (scene, "2^20 miss", fld)
        for fld in ("t", "u", "v", "triIdx"):
            assert np.array_equal(got[fld][mesh].view(np.uint32), w[fld][mesh].view(np.uint32)), (scene, "2^20 mesh", fld)
        ob, _ = orc.load_scene(xml, 0, ASSETS)
        wb = ob.find_nearest(O[sub], D[sub], inside[sub])
        for fld in ("t", "u", "v", "objIdx", "triIdx"):
            assert np.array_equal(got[fld][general].view(np.uint32), wb[fld][general].view(np.uint32)), (scene, "2^20 BVH answer", fld)
    if own is not None:
        own.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 2. pinned occlusion: FILE / KD-tree / grid against the real reference's golden hits + the Quad::IsOccluded restatement
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def pinned_rays(crt, orc, xml, hs, mesh, kind):
    z = np.load(os.path.join(GOLDEN, "ref_bvh_rays.npz")); r = np.load(os.path.join(GOLDEN, "ref_alt_rays.npz"))
    Og, Dg = z[mesh + "_O"].astype(np.float32), z[mesh + "_D"].astype(np.float32)
    gmesh = (z[mesh + "_objIdx"] if kind == "bvh" else r["%s_%s_objIdx" % (mesh, kind)]) > -1       # BVH / KDTree / Grid::Intersect alone, whole ray
    top = hs.bvh(0)["nodes"][0]["aabbMax"][1]
    assert top < LIGHT[1] - 0.01, "the mesh must lie below the light plane"
    lo, hi = hs.bvh(0)["nodes"][0]["aabbMin"], hs.bvh(0)["nodes"][0]["aabbMax"]
    Ou1, Du1 = up_rays(400, 5, LIGHT, (-1.5, 1.5), (0.5, 3.5), -0.9, LIGHT[1] - 0.3)        # around the mesh, above and beside it
    Ou2, Du2 = up_rays(200, 6, LIGHT, (lo[0], hi[0]), (lo[2], hi[2]), -0.95, max((lo[1] + hi[1]) / 2, -0.5), spread=0.45)   # from under / inside the mesh into the quad
    Ou, Du = np.concatenate([Ou1, Ou2]), np.concatenate([Du1, Du2])
    o, _ = orc.load_scene(xml, 0, ASSETS)
    w = o.find_nearest(Ou, Du)["objIdx"]
    assert set(np.unique(w)) <= {-1, 0} | set(range(2, 64)), "an upward ray above the floor cannot hit it"
    umesh = w >= 2                                                        # 0 / -1: no mesh on the ray (nothing lies above the light)
    O = np.concatenate([Og, Ou]); D = np.concatenate([Dg, Du])
    _, tq = quad_occluded(O, D, np.full(len(O), 1e34, np.float32), LIGHT)
    t = pick_t(tq)
    q, _ = quad_occluded(O, D, t, LIGHT)
    m = np.concatenate([gmesh, umesh])
    return O, D, t, q, m


@pytest.mark.parametrize("kind", ["bvh", "kd", "grid"])
@pytest.mark.parametrize("mesh", ["bunny", "teapot", "cube"])
def test_is_occluded_pinned(crt, orc, tmp_path, mesh, kind):
    xml = write_scene(tmp_path, mesh)
    hs = crt.HostScene(xml, 0, ASSETS)
    ctx = crt.Context(64, 64); hs.upload(ctx)
    accel = {"bvh": 0, "kd": crt.ACCEL_KDTREE, "grid": crt.ACCEL_GRID}[kind]
    if accel:
        hs.build_alt(accel); hs.upload_alt(ctx, accel)
    O, D, t, q, m = pinned_rays(crt, orc, xml, hs, mesh, kind)
    for name, sel in (("quad only", q & ~m), ("mesh only", ~q & m), ("both", q & m), ("neither", ~q & ~m)):
        assert sel.sum() >= 20, (name, int(sel.sum()))
    want = q | m
    got_host = ctx.is_occluded(O, D, t, accel=accel)
    assert np.array_equal(got_host, want), np.flatnonzero(got_host != want)[:10]
    got_dev = ctx.is_occluded_device(shadow_records(O, D, t), accel=accel).cpu().numpy()
    assert got_dev.dtype == np.int32 and set(np.unique(got_dev)) <= {0, 1}
    assert np.array_equal(got_dev != 0, want)
    got_od = ctx.is_occluded_device(O=torch.from_numpy(O).to(dev()), D=torch.from_numpy(D).to(dev()), t=torch.from_numpy(t).to(dev()), accel=accel)
    assert np.array_equal(got_od.cpu().numpy() != 0, want)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 3. TLAS occlusion against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def tlas_up_rays(hs, light, n=4000, seed=3):
    nodes, _ = hs.tlas()
    lo, hi = nodes[0]["aabbMin"], nodes[0]["aabbMax"]
    assert hi[1] < light[1] - 0.01, "every instance must lie below the light plane"
    sets = [up_rays(n, seed, light, (lo[0], hi[0]), (lo[2], hi[2]), -0.95, light[1] - 0.2)]
    for i in range(hs.bvh_count()):                                       # from under / inside each instance into the quad
        _, _, blo, bhi = hs.blas_transform(i)
        sets.append(up_rays(200, seed + 1 + i, light, (blo[0], bhi[0]), (blo[2], bhi[2]), -0.95, max((blo[1] + bhi[1]) / 2, -0.5), spread=0.45))
    return np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])


def test_is_occluded_tlas_vs_oracle(crt, orc):
    xml = scene_path("tlas_scene.xml"); light = light_of(xml)
    hs = crt.HostScene(xml, 1, ASSETS)
    ctx = crt.Context(64, 64); hs.upload(ctx)
    O, D = tlas_up_rays(hs, light)
    o, _ = orc.load_scene(xml, 1, ASSETS)
    w = o.find_nearest(O, D)["objIdx"]
    assert not (w == 1).any()                                             # upward rays above the floor never reach it
    _, tq = quad_occluded(O, D, np.full(len(O), 1e34, np.float32), light)
    t = pick_t(tq)
    q, _ = quad_occluded(O, D, t, light)
    m = w >= 2                                                            # a light hit (0) hides nothing: no instance lies above the light
    for name, sel in (("quad only", q & ~m), ("mesh only", ~q & m), ("both", q & m), ("neither", ~q & ~m)):
        assert sel.sum() >= 20, (name, int(sel.sum()))
    want = q | m
    assert np.array_equal(ctx.is_occluded(O, D, t), want)
    assert np.array_equal(ctx.is_occluded_device(shadow_records(O, D, t)).cpu().numpy() != 0, want)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 4. stream ordering
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_stream_ordering_against_scene_updates(crt, orc):
    xml = scene_path("tlas_scene.xml"); light = light_of(xml)
    hs = crt.HostScene(xml, 1, ASSETS)
    ctx = crt.Context(64, 64); hs.upload(ctx)
    o, _ = orc.load_scene(xml, 1, ASSETS)
    n = 1 << 20
    O, D = camera_rays(n, 21, cam=(0.0, 0.5, -1.0), half=(2.5, 1.2), z=2.0)
    t = np.full(n, 1e34, np.float32)
    rays, srays = ray_records(O, D), shadow_records(O, D, t)
    sub = np.arange(0, n, 64)                                             # the oracle's share: every 64th ray
    before = o.find_nearest(O[sub], D[sub])
    occ_before = ctx.is_occluded(O, D, t)                                 # host entry (agreement with the device entry below)
    T0 = hs.blas_transform(1)[0].reshape(4, 4)
    T = rigid(0.9, T0[:3, 3] + np.array([-0.6, 0.0, -1.2], np.float32))
    side = torch.cuda.Stream(device=dev())
    h1 = ctx.find_nearest_device(rays, stream=side)
    q1 = ctx.is_occluded_device(srays, stream=side)
    hs.set_transform(1, T); hs.update(ctx, crt.UPDATE_TRANSFORMS)        # no host sync in between
    h2 = ctx.find_nearest_device(rays, stream=side)
    q2 = ctx.is_occluded_device(srays, stream=side)
    side.synchronize()
    o.set_transform(1, T)
    after = o.find_nearest(O[sub], D[sub])
    g1, g2 = hits_np(crt, h1), hits_np(crt, h2)
    for fld in ("t", "u", "v", "objIdx", "triIdx"):
        assert np.array_equal(g1[fld][sub].view(np.uint32), before[fld].view(np.uint32)), ("before", fld)
        assert np.array_equal(g2[fld][sub].view(np.uint32), after[fld].view(np.uint32)), ("after", fld)
    assert (before["objIdx"] != after["objIdx"]).sum() > 50                # the move changes what these rays see
    assert np.array_equal(q1.cpu().numpy() != 0, occ_before)
    assert np.array_equal(q2.cpu().numpy() != 0, ctx.is_occluded(O, D, t))
    assert (occ_before != ctx.is_occluded(O, D, t)).any()
    # two queries in flight on two streams at once (each draws from its own cursor)
    sA, sB = torch.cuda.Stream(device=dev()), torch.cuda.Stream(device=dev())
    O2, D2 = camera_rays(n, 22, cam=(0.3, 0.8, -1.5), half=(2.0, 1.5), z=2.5)
    rays2 = ray_records(O2, D2)
    hA = ctx.find_nearest_device(rays, stream=sA)
    hB = ctx.find_nearest_device(rays2, stream=sB)
    qA = ctx.is_occluded_device(srays, stream=sA)
    sA.synchronize(); sB.synchronize()
    assert_hits_equal(hits_np(crt, hA), g2, "stream A")
    assert_hits_equal(hits_np(crt, hB), ctx.find_nearest(O2, D2), "stream B")
    assert np.array_equal(qA.cpu().numpy(), q2.cpu().numpy())
    # a torch op on the same stream consumes the hits without a host synchronisation
    with torch.cuda.stream(sA):
        h = ctx.find_nearest_device(rays2)                                  # current stream = sA
        meshes = (crt.hit_fields(h)["objIdx"] >= 2).sum()
    sA.synchronize()
    assert int(meshes.item()) == int((ctx.find_nearest(O2, D2)["objIdx"] >= 2).sum())
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(crt, bunny_file):
    import ctypes as C
    L = crt.lib()
    xml, hs, ctx = bunny_file
    host = np.zeros((16, 7), np.float32)
    d_rays = ray_records(np.zeros((16, 3), np.float32), np.tile(np.array([[0, 0, 1]], np.float32), (16, 1)))
    d_out = torch.empty((16, 7), dtype=torch.float32, device=dev())
    p = lambda a: C.c_void_p(a.ctypes.data)                                 # noqa: E731
    d = lambda x: C.c_void_p(x.data_ptr())                                   # noqa: E731
    # host pointers where device buffers belong
    assert L.crt_find_nearest_device(ctx.h, 0, p(host), d(d_out), C.c_size_t(16), None) == -1
    assert L.crt_find_nearest_device(ctx.h, 0, d(d_rays), p(host), C.c_size_t(16), None) == -1
    assert L.crt_is_occluded_device(ctx.h, 0, p(host), d(d_out), C.c_size_t(16), None) == -1
    assert b"device memory" in L.crt_last_error(ctx.h)
    # n == 0: a no-op, even with NULL buffers;  n > 2^31-1: unsupported
    for entry in (L.crt_find_nearest_device, L.crt_is_occluded_device):
        assert entry(ctx.h, 0, None, None, C.c_size_t(0), None) == 0
        assert entry(ctx.h, 0, d(d_rays), d(d_out), C.c_size_t(1 << 31), None) == -4
    assert L.crt_is_occluded(ctx.h, 0, None, None, C.c_size_t(0)) == 0
    # PrimitiveScene occlusion
    pc = crt.Context(64, 64); ps = crt.HostPrimitiveScene(ASSETS); ps.upload(pc)
    with pytest.raises(crt.CrtError) as e:
        pc.is_occluded(np.zeros((1, 3)), np.array([[0, 1, 0]]), 1e34)
    assert e.value.code == -4
    with pytest.raises(crt.CrtError) as e:
        pc.is_occluded_device(O=torch.zeros((1, 3), device=dev()), D=torch.tensor([[0.0, 1.0, 0.0]], device=dev()), t=1e34)
    assert e.value.code == -4
    pc.close()
    # an accelerator that was not uploaded, and no scene at all
    c2 = crt.Context(64, 64)
    for call in (lambda: c2.is_occluded(np.zeros((1, 3)), np.array([[0, 1, 0]]), 1e34),
                 lambda: c2.find_nearest_device(d_rays),
                 lambda: c2.is_occluded_device(O=torch.zeros((1, 3), device=dev()), D=torch.tensor([[0.0, 1.0, 0.0]], device=dev()), t=1e34)):
        with pytest.raises(crt.CrtError) as e:
            call()
        assert e.value.code == -5
    hs.upload(c2)
    for accel in (crt.ACCEL_KDTREE, crt.ACCEL_GRID):
        with pytest.raises(crt.CrtError) as e:
            c2.find_nearest_device(d_rays, accel=accel)
        assert e.value.code == -5
        with pytest.raises(crt.CrtError) as e:
            c2.is_occluded(np.zeros((1, 3)), np.array([[0, 1, 0]]), 1e34, accel=accel)
        assert e.value.code == -5
    c2.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 6. the host entries' device staging: one context serving entry after entry == a fresh context per call (agreement check)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_host_entries_in_sequence_equal_fresh_contexts(crt):
    """The host-buffer entries stage their records in device memory that the context keeps and grows.  Seven calls on ONE context, whose record sizes and counts
    differ (28-byte rays and hits, 48-byte hit infos, 4-byte flags and seeds, 12-byte colours; 63 / 64 / 65 rays = one wavefront less one, exact, plus one, and
    130 = two plus two), each answer bit-equal to the same call on a context that has done nothing else; the last repeats the first."""
    hs = crt.HostScene(scene_path("cube_scene.xml"), 0, ASSETS)
    hs.build_alt(crt.ACCEL_KDTREE)

    def context():
        ctx = crt.Context(64, 64)
        hs.upload(ctx); hs.upload_alt(ctx, crt.ACCEL_KDTREE)
        return ctx

    O, D = camera_rays(130, 5)
    inside = (np.arange(130) % 5 == 3).astype(np.int32)
    seeds = (np.arange(130, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)) | np.uint32(1)
    tq = quad_occluded(O, D, np.full(130, 1e34, np.float32), LIGHT)[1]
    calls = [
        ("find_nearest 64", lambda c, first: c.find_nearest(O[:64], D[:64], inside[:64])),
        ("get_hit_info 64", lambda c, first: c.get_hit_info(O[:64], D[:64], first)),
        ("is_occluded 65", lambda c, first: c.is_occluded(O[:65], D[:65], pick_t(tq)[:65])),
        ("sample 130", lambda c, first: np.concatenate([a.view(np.uint32).reshape(130, -1) for a in c.sample(O, D, seeds, inside)], axis=1)),
        ("get_sky_color 63", lambda c, first: c.get_sky_color(D[:63])),
        ("find_nearest_alt 65", lambda c, first: c.find_nearest_alt(crt.ACCEL_KDTREE, O[:65], D[:65])),
        ("find_nearest 64 again", lambda c, first: c.find_nearest(O[:64], D[:64], inside[:64])),
    ]
    shared = context()
    got = []
    for what, call in calls:
        got.append(call(shared, got[0] if got else None))
        fresh = context()
        want = call(fresh, got[0])
        fresh.close()
        assert got[-1].dtype == want.dtype and got[-1].shape == want.shape and got[-1].tobytes() == want.tobytes(), what
    shared.close()
    assert got[-1].tobytes() == got[0].tobytes()
    obj = got[0]["objIdx"]
    assert (obj >= 2).any() and (obj == 1).any() and (obj == -1).any()          # the rays see the cube, the floor and the sky: the records differ


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 7. one HIP runtime in the process (stream handles are only meaningful then)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_one_hip_runtime_is_loaded(crt):
    torch.cuda.init()
    crt.lib()
    libs = set()
    for line in open("/proc/self/maps"):
        parts = line.split()
        if len(parts) >= 6 and "libamdhip64" in parts[-1]:
            libs.add(os.path.realpath(parts[-1]))
    assert len(libs) == 1, sorted(libs)
