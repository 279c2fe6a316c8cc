"""crt_refit_device: BVH::Refit / BLASBVH::Refit (infra/bvh.cpp:26-61) on the GPU from vertex positions held in a torch tensor — leaf triangles and node boxes of
one uploaded BVH rewritten in place by HIP kernels, bit for bit what the host Refit + crt_update_scene(CRT_UPDATE_BOUNDS) leave, the reference's skipped node 1
included.  Every comparison is exact: against the oracle doing move_and_refit, and against contexts that took the host path."""
import numpy as np
import pytest

from conftest import ASSETS, scene_path
from test_oracle_pinning import deform

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

W, H = 96, 64
FIELDS = ("t", "u", "v", "objIdx", "triIdx", "traversed", "tested")
# (scene, kind, BLAS): cube = 12 triangles, 13 nodes, leaves of 2 — the smallest tree with every node kind; the two-level scene's first and last BLAS
CASES = [("cube_scene.xml", 0, 0), ("bunny_scene.xml", 0, 0), ("tlas_scene.xml", 1, 0), ("tlas_scene.xml", 1, -1)]
IDS = ["cube", "bunny", "tlas-first", "tlas-last"]


def dev():
    return torch.device("cuda", 0)


def to_dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev())
    torch.cuda.synchronize()
    return t


def positions(b):
    t = b["tris"]
    return np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1).astype(np.float32)


def load(crt, orc, xml, kind, which, upload=True):
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    o, _ = orc.load_scene(scene_path(xml), kind, ASSETS)
    o.renderer_init(W, H)
    ctx = crt.Context(W, H)
    if upload:
        hs.upload(ctx)
    return hs, o, ctx, which % hs.bvh_count()


def world_box(hs, kind, i):
    if kind == 1:
        _, _, lo, hi = hs.blas_transform(i)
        return lo, hi
    n = hs.bvh(i)["nodes"][0]
    return n["aabbMin"].copy(), n["aabbMax"].copy()


def aimed_rays(lo, hi, n, seed):
    """rays from a shell around the box towards points inside it (slightly enlarged, so that some graze and miss)"""
    rng = np.random.default_rng(seed)
    c, r = (lo + hi) * 0.5, np.linalg.norm(hi - lo) * 0.5
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    O = (c + d * rng.uniform(1.5, 3.0, (n, 1)) * r).astype(np.float32)
    T = c + (rng.uniform(-0.6, 0.6, (n, 3)) * (hi - lo))
    D = T - O; D /= np.linalg.norm(D, axis=1, keepdims=True)
    return O, D.astype(np.float32)


def assert_hits_equal(a, b, what):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (what, f)


@pytest.fixture(params=["default", "pool_always"])
def kernel(request, monkeypatch):
    if request.param != "default":
        monkeypatch.setenv("CRT_RENDER_KERNEL", request.param)
    return request.param


# 1. hits
@pytest.mark.parametrize("xml,kind,which", CASES, ids=IDS)
def test_hits_match_oracle_and_host_refit(crt, orc, xml, kind, which):
    hs, o, ctx, i = load(crt, orc, xml, kind, which)
    b0 = hs.bvh(i)
    moved = deform(positions(b0))
    O, D = aimed_rays(*world_box(hs, kind, i), 2000, 5)
    before = ctx.find_nearest(O, D)
    hs.refit_device(ctx, i, to_dev(moved)); o.move_and_refit(i, moved)
    got = ctx.find_nearest(O, D)
    assert_hits_equal(got, o.find_nearest(O, D), "oracle")
    assert (got["objIdx"] >= 2).sum() > 200
    h2 = crt.HostScene(scene_path(xml), kind, ASSETS); c2 = crt.Context(W, H); h2.upload(c2)
    h2.move_and_refit(i, moved); h2.update(c2, crt.UPDATE_BOUNDS)
    assert_hits_equal(got, c2.find_nearest(O, D), "host refit + UPDATE_BOUNDS")
    assert (got["traversed"] != before["traversed"]).any()                  # the update is seen
    n1 = h2.bvh(i)["nodes"]                                                  # the quirk the kernel must keep: Refit skips node 1 (bvh.cpp:28)
    assert n1[1].tobytes() == b0["nodes"][1].tobytes() and n1[2].tobytes() != b0["nodes"][2].tobytes()


# 2. images, both render kernels, with renders of the old scene still in flight
@pytest.mark.parametrize("xml,kind,which", CASES, ids=IDS)
def test_images_match_oracle_and_fresh_upload(crt, orc, kernel, xml, kind, which):
    hs, o, ctx, i = load(crt, orc, xml, kind, which)
    moved = deform(positions(hs.bvh(i)))
    moved_t = to_dev(moved)
    ctx.render(1, 2, 1)                                                     # no sync
    hs.refit_device(ctx, i, moved_t); o.move_and_refit(i, moved)
    ctx.clear()
    ctx.render(1, 3, 1); o.render(3, 4)
    acc = ctx.accumulator()
    assert np.array_equal(acc, o.accumulator())
    h2 = crt.HostScene(scene_path(xml), kind, ASSETS); h2.move_and_refit(i, moved)
    c2 = crt.Context(W, H); h2.upload(c2); c2.render(1, 3, 1)
    assert np.array_equal(acc, c2.accumulator())


# 3. the TLAS follow-up of the host front, and the returned root box
@pytest.mark.parametrize("which", [0, -1])
def test_tlas_follow_up_and_root_box(crt, orc, which):
    hs, o, ctx, i = load(crt, orc, "tlas_scene.xml", 1, which)
    moved = deform(positions(hs.bvh(i)))
    hs.refit_device(ctx, i, to_dev(moved)); o.move_and_refit(i, moved)
    assert np.array_equal(hs.tlas()[0], o.tlas()[0]) and hs.tlas()[1] == o.tlas()[1]
    for a, b in zip(hs.blas_transform(i), o.blas_transform(i)):
        assert np.array_equal(a, b)
    root = o.bvh(i)["nodes"][0]
    assert np.array_equal(hs.bvh(i)["nodes"][0]["aabbMin"], root["aabbMin"]) and np.array_equal(hs.bvh(i)["nodes"][0]["aabbMax"], root["aabbMax"])
    box = ctx.refit_device(i, to_dev(moved))                                 # the ABI entry alone, same positions: the same box comes back
    assert np.array_equal(box[0], root["aabbMin"]) and np.array_equal(box[1], root["aabbMax"])
    assert ctx.refit_device(i, to_dev(moved), root_box=False) is None


# 4. twice, and back
@pytest.mark.parametrize("xml,kind,which", [CASES[1], CASES[3]], ids=[IDS[1], IDS[3]])
def test_refit_twice_and_back(crt, orc, xml, kind, which):
    hs, o, ctx, i = load(crt, orc, xml, kind, which)
    b0 = hs.bvh(i); p0 = positions(b0)
    O, D = aimed_rays(*world_box(hs, kind, i), 2000, 9)
    original = ctx.find_nearest(O, D)
    first = deform(p0); second = (p0 * np.float32(1.03) + np.float32(0.01)).astype(np.float32)
    for step, pos in (("first", first), ("second", second), ("back", p0)):
        hs.refit_device(ctx, i, to_dev(pos)); o.move_and_refit(i, pos)
        got = ctx.find_nearest(O, D)
        assert_hits_equal(got, o.find_nearest(O, D), step)
        assert o.bvh(i)["nodes"][1].tobytes() == b0["nodes"][1].tobytes()   # node 1 never changes
    assert_hits_equal(got, original, "the original positions again")
    fresh = crt.Context(W, H); crt.HostScene(scene_path(xml), kind, ASSETS).upload(fresh)
    assert_hits_equal(got, fresh.find_nearest(O, D), "fresh upload of the original scene")


# 5. streams: the refit on one torch stream, a device query on another, no host synchronisation in between
def test_refit_and_query_on_different_streams(crt, orc):
    hs, o, ctx, i = load(crt, orc, "bunny_scene.xml", 0, 0)
    moved = deform(positions(hs.bvh(i)))
    O, D = aimed_rays(*world_box(hs, 0, i), 2000, 13)
    rays = np.zeros(len(O), crt.RAY_DTYPE); rays["O"], rays["D"] = O, D
    rays_t = torch.from_numpy(rays.view(np.float32).reshape(-1, 7).copy()).to(dev())
    moved_t = to_dev(moved)
    s1, s2 = torch.cuda.Stream(device=dev()), torch.cuda.Stream(device=dev())
    old = ctx.find_nearest_device(rays_t, stream=s2)                       # in flight when the refit is enqueued: still the old scene
    ctx.refit_device(i, moved_t, stream=s1)
    new = ctx.find_nearest_device(rays_t, stream=s2)
    torch.cuda.synchronize()
    o_old = o.find_nearest(O, D); o.move_and_refit(i, moved)
    assert_hits_equal(old.cpu().numpy().view(crt.HIT_DTYPE).reshape(-1), o_old, "before")
    assert_hits_equal(new.cpu().numpy().view(crt.HIT_DTYPE).reshape(-1), o.find_nearest(O, D), "after")


# 6. crt_tick: the frames rendered ahead are of the old scene
def test_tick_after_refit_drops_frames_rendered_ahead(crt, orc):
    hs, o, ctx, i = load(crt, orc, "bunny_scene.xml", 0, 0)
    moved = deform(positions(hs.bvh(i)))
    moved_t = to_dev(moved)
    ctx.tick(1); ctx.tick(2)                                                # the second still Tick renders frames 3.. ahead
    hs.refit_device(ctx, i, moved_t)
    px, acc, energy = ctx.tick(3)
    o.render(2, 4); o.move_and_refit(i, moved); o.render(1, 4)              # frames 1, 2 of the old scene, frame 3 of the refitted one
    assert np.array_equal(acc, o.accumulator()) and np.array_equal(px, o.screen()) and energy == o.energy()


# 7. a root that is a leaf: no node pair at all, node 0's box is UpdateNodeBounds
def test_leaf_root(crt):
    tris = np.zeros(2, crt.TRI_DTYPE)
    tris["vertex0"] = [[-0.5, -0.5, 2.0], [0.1, -0.4, 2.5]]; tris["vertex1"] = [[0.5, -0.5, 2.0], [0.9, -0.4, 2.5]]; tris["vertex2"] = [[0.0, 0.5, 2.2], [0.5, 0.6, 2.4]]
    for k in ("normal0", "normal1", "normal2"):
        tris[k] = [0, 0, -1]
    tris["objIdx"] = 2

    def arrays(t):
        p = positions(dict(tris=t))
        nodes = np.zeros(1, crt.NODE_DTYPE)
        nodes["aabbMin"][0] = p.reshape(-1, 3).min(0); nodes["aabbMax"][0] = p.reshape(-1, 3).max(0); nodes["leftFirst"] = 0; nodes["triCount"] = 2
        return dict(nodes=nodes, tris=t, triIndices=np.array([1, 0], np.uint32))

    tex = np.full((4, 4), 0x808080, np.uint32); ident = np.eye(4, dtype=np.float32)
    lt = ident.copy(); lt[:3, 3] = (0, 3, 1); li = ident.copy(); li[:3, 3] = (0, -3, -1)
    common = dict(textures=[tex, tex], floor_texture=0, sky_texture=1, materials=[(0.0, 0.0, (0.0, 0.0, 0.0), -1)], light_T=lt, light_invT=li, obj_mat_idx=[0])
    a, b = crt.Context(64, 64), crt.Context(64, 64)
    a.upload_desc(crt.SCENE_FILE, [arrays(tris)], **common); b.upload_desc(crt.SCENE_FILE, [arrays(tris)], **common)
    moved = deform(positions(dict(tris=tris)) * np.float32(1.5))
    t2 = tris.copy(); t2["vertex0"], t2["vertex1"], t2["vertex2"] = moved[:, 0], moved[:, 1], moved[:, 2]
    host = arrays(t2)
    O, D = aimed_rays(host["nodes"]["aabbMin"][0], host["nodes"]["aabbMax"][0], 1500, 3)
    before = a.find_nearest(O, D)
    box = a.refit_device(0, to_dev(moved.reshape(-1, 9)))                    # the [triCount, 9] form
    assert np.array_equal(box[0], host["nodes"]["aabbMin"][0]) and np.array_equal(box[1], host["nodes"]["aabbMax"][0])
    b.upload_desc(crt.SCENE_FILE, [host], update_what=crt.UPDATE_BOUNDS, **common)
    got = a.find_nearest(O, D)
    assert_hits_equal(got, b.find_nearest(O, D), "UPDATE_BOUNDS from host-refitted arrays")
    assert (got["objIdx"] == 2).sum() > 100 and any((got[f] != before[f]).any() for f in ("t", "objIdx"))


# 8. refusals leave the scene as it was; the stale mark of the host front
def test_refusals_and_stale_mark(crt, orc):
    hs, o, ctx, i = load(crt, orc, "bunny_scene.xml", 0, 0, upload=False)
    p0 = positions(hs.bvh(0)); good = to_dev(p0 * np.float32(1.1))
    o.render(1, 4); want = o.accumulator()

    def unchanged():
        ctx.clear(); ctx.render(1, 1, 1)
        assert np.array_equal(ctx.accumulator(), want)

    with pytest.raises(crt.CrtError) as e:                                  # before any upload
        ctx.refit_device(0, good)
    assert e.value.code == -5
    hs.upload(ctx); unchanged()
    C = crt.C
    for call in (lambda: ctx.refit_device(0, good[:-1].contiguous()),                                        # wrong triCount
                 lambda: ctx.refit_device(1, good),                                                          # bvh out of range
                 lambda: ctx._ck(ctx.L.crt_refit_device(ctx.h, C.c_uint32(0), p0.ctypes.data_as(C.c_void_p), C.c_uint32(len(p0)), None, None))):   # a host pointer
        with pytest.raises(crt.CrtError) as e:
            call()
        assert e.value.code == -1
        unchanged()
    with pytest.raises(ValueError):                                         # a CPU tensor does not get as far as the ABI
        ctx.refit_device(0, torch.from_numpy(p0))
    with pytest.raises(ValueError):
        hs.refit_device(ctx, 0, torch.from_numpy(p0))
    unchanged()
    # a PrimitiveScene has no BVH
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(0.0)
    pc = crt.Context(W, H); ps.upload(pc)
    with pytest.raises(crt.CrtError) as e:
        pc.refit_device(0, good)
    assert e.value.code == -4
    op = orc.primitive_scene(ASSETS, 0.0); op.renderer_init(W, H); op.render(1, 4)
    pc.render(1, 1, 1)
    assert np.array_equal(pc.accumulator(), op.accumulator())
    # the stale mark: after a device refit the host arrays of the BVH are old, so the calls that would send them are refused until move_and_refit
    moved = deform(p0)
    hs.refit_device(ctx, 0, to_dev(moved))
    other = crt.Context(W, H)
    for call in (lambda: hs.upload(other), lambda: hs.update(ctx, crt.UPDATE_BOUNDS)):
        with pytest.raises(crt.CrtError) as e:
            call()
        assert e.value.code == -5 and "stale" in str(e.value)
    hs.move_and_refit(0, moved); o.move_and_refit(0, moved)
    hs.update(ctx, crt.UPDATE_BOUNDS); hs.upload(other)
    o.clear(); o.render(1, 4)
    for c in (ctx, other):
        c.clear(); c.render(1, 1, 1)
        assert np.array_equal(c.accumulator(), o.accumulator())


# 9. a two-level scene's KD-tree / grid set is dropped, as by CRT_UPDATE_BOUNDS (the reference has no Refit for those structures)
@pytest.mark.parametrize("code", [1, 2], ids=["kdtree", "grid"])
def test_refit_drops_the_blas_set(crt, orc, code):
    xml = scene_path("tlas_scene.xml")
    hs = crt.HostScene(xml, 1, ASSETS); hs.build_alt(code)
    ctx = crt.Context(W, H); hs.upload(ctx); hs.upload_alt(ctx, code)
    o, _ = orc.load_scene(xml, 1, ASSETS); o.renderer_init(W, H)
    ctx.set_render_accel(code)
    pos = positions(hs.bvh(0)) * np.float32(1.01)
    hs.refit_device(ctx, 0, to_dev(pos)); o.move_and_refit(0, pos)
    with pytest.raises(crt.CrtError) as e:
        ctx.find_nearest_alt(code, np.zeros((1, 3), np.float32), np.array([[0, 0, 1]], np.float32))
    assert e.value.code == -5
    with pytest.raises(crt.CrtError):
        ctx.set_render_accel(code)
    ctx.render(1, 3, 1); o.render(3, 8)                                     # back on the BVH
    assert np.array_equal(ctx.accumulator(), o.accumulator())
