"""crt_update_transforms_device: BLASBVH::SetTransform of every instance + TLASBVH::Build on the GPU from transforms held in a torch tensor.  Every comparison is
exact: against the oracle after set_transform for every instance, and against contexts that took the host route (set_transform x N + UPDATE_TRANSFORMS).
The input sets and what each is for: tests/tlas_device_inputs.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import ASSETS, scene_path
from test_oracle_pinning import deform
import tlas_device_inputs as inp

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

W, H = 96, 64
FIELDS = ("t", "u", "v", "objIdx", "triIdx", "traversed", "tested")
BUILDABLE = [s for s in inp.SETS if s != "nan"]
INVALID, UNSUPPORTED, STATE = -1, -4, -5


def dev():
    return torch.device("cuda", 0)


def to_dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev())
    torch.cuda.synchronize()
    return t


def load(crt, orc, tmp_path, name, oracle=True, **ctx_args):
    xml = inp.scene_xml(tmp_path, name)
    hs = crt.HostScene(xml, 1, ASSETS)
    ctx = crt.Context(W, H, **ctx_args)
    hs.upload(ctx)
    o = None
    if oracle:
        o, _ = orc.load_scene(xml, 1, ASSETS)
        o.renderer_init(W, H)
    return xml, hs, o, ctx, inp.transforms(name)


def host_route(crt, xml, T, **ctx_args):
    """a second context that gets the same transforms through the host: set_transform for every instance, then UPDATE_TRANSFORMS"""
    hs = crt.HostScene(xml, 1, ASSETS)
    ctx = crt.Context(W, H, **ctx_args)
    hs.upload(ctx)
    for i in range(len(T)):
        hs.set_transform(i, T[i])
    hs.update(ctx, crt.UPDATE_TRANSFORMS)
    return hs, ctx


def move_oracle(o, T):
    for i in range(len(T)):
        o.set_transform(i, T[i])


def assert_hits_equal(a, b, what):
    for f in FIELDS:
        assert a[f].tobytes() == b[f].tobytes(), (what, f)


def records(crt, O, D):
    rays = np.zeros(len(O), crt.RAY_DTYPE)
    rays["O"], rays["D"] = O, D
    return torch.from_numpy(rays.view(np.float32).reshape(-1, 7).copy()).to(dev())


@pytest.fixture(params=["default", "pool_always"])
def kernel(request, monkeypatch):
    if request.param != "default":
        monkeypatch.setenv("CRT_RENDER_KERNEL", request.param)
    return request.param


# 1. the node array and the scene on the device, per input set
@pytest.mark.parametrize("name", BUILDABLE)
def test_tlas_and_hits_match_oracle_and_host_route(crt, orc, tmp_path, name):
    xml, hs, o, ctx, T = load(crt, orc, tmp_path, name)
    O, D = inp.aimed_rays(T)
    nodes = ctx.update_transforms_device(to_dev(T))
    move_oracle(o, T)
    want, used = o.tlas()
    assert used == 2 * len(T) and nodes.tobytes() == want.tobytes()
    got = ctx.find_nearest(O, D)
    assert_hits_equal(got, o.find_nearest(O, D), "oracle")                  # `traversed` pins the topology on the device, not only in tlasOut
    assert (got["objIdx"] >= 2).sum() >= 200
    _, c2 = host_route(crt, xml, T)
    assert_hits_equal(got, c2.find_nearest(O, D), "host route")


# 2. images and counters, both render kernels
@pytest.mark.parametrize("name", ["tlas3", "ring40", "rand256"])
def test_render_matches_oracle(crt, orc, tmp_path, kernel, name):
    xml, hs, o, ctx, T = load(crt, orc, tmp_path, name, collect_stats=True)
    ctx.update_transforms_device(to_dev(T).reshape(-1, 16))                  # the [N, 16] form
    move_oracle(o, T)
    ctx.render(1, 2, 1); o.render(2, 4)
    assert np.array_equal(ctx.accumulator(), o.accumulator())
    assert ctx.counters() == o.counters()


# 3. the chain the entry exists for: a refit on the device, then the TLAS on the device, nothing from the host in between
def test_refit_device_then_update_transforms_device(crt, orc, tmp_path):
    xml, hs, o, ctx, T = load(crt, orc, tmp_path, "ring40")
    i = 7
    t = hs.bvh(i)["tris"]
    moved = deform(np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1).astype(np.float32) * np.float32(1.7))
    O, D = inp.aimed_rays(T)
    ctx.refit_device(i, to_dev(moved), root_box=False)                      # the ABI entry alone: the host front's would rebuild the TLAS on the host
    nodes = ctx.update_transforms_device(to_dev(T))
    o.move_and_refit(i, moved); move_oracle(o, T)
    assert nodes.tobytes() == o.tlas()[0].tobytes()
    got = ctx.find_nearest(O, D)
    assert_hits_equal(got, o.find_nearest(O, D), "oracle")
    assert (got["objIdx"] == i + 2).sum() > 0


# 4. stream order: query, update, query on one side stream without a host synchronisation in between
def test_stream_order(crt, orc, tmp_path):
    xml, hs, o, ctx, T = load(crt, orc, tmp_path, "ring40")
    O, D = inp.aimed_rays(T)
    rays_t = records(crt, O, D); T_t = to_dev(T)
    s = torch.cuda.Stream(device=dev())
    old = ctx.find_nearest_device(rays_t, stream=s)
    ctx.update_transforms_device(T_t, stream=s)
    new = ctx.find_nearest_device(rays_t, stream=s)
    torch.cuda.synchronize()
    o_old = o.find_nearest(O, D); move_oracle(o, T)
    assert_hits_equal(old.cpu().numpy().view(crt.HIT_DTYPE).reshape(-1), o_old, "before")
    assert_hits_equal(new.cpu().numpy().view(crt.HIT_DTYPE).reshape(-1), o.find_nearest(O, D), "after")
    assert (o_old["traversed"] != new.cpu().numpy().view(crt.HIT_DTYPE).reshape(-1)["traversed"]).any()


# 5. the host mirror: a later CRT_UPDATE_BOUNDS-only update rewrites the TLAS and instance sections from it
def test_mirror_follows_the_device_update(crt, orc, tmp_path):
    xml, hs, o, ctx, T = load(crt, orc, tmp_path, "ring40", oracle=False)
    O, D = inp.aimed_rays(T)
    original = ctx.find_nearest(O, D)
    nodes = ctx.update_transforms_device(to_dev(T))
    got = ctx.find_nearest(O, D)
    assert any((got[f] != original[f]).any() for f in ("t", "objIdx"))
    bvhs = []
    for i in range(hs.bvh_count()):
        b = hs.bvh(i); T0, invT0, _, _ = hs.blas_transform(i)               # the host scene's transforms are still the old ones: UPDATE_BOUNDS does not read them
        b.update(objIdx=i + 2, matIdx=0, T=T0, invT=invT0); bvhs.append(b)
    tex = np.full((4, 4), 0x808080, np.uint32); ident = np.eye(4, dtype=np.float32)
    ctx.upload_desc(crt.SCENE_TLAS, bvhs, tlas_nodes=nodes, update_what=crt.UPDATE_BOUNDS, textures=[tex, tex], floor_texture=0, sky_texture=1,
                    materials=[(0.0, 0.0, (0.0, 0.0, 0.0), -1)], light_T=ident, light_invT=ident)
    assert_hits_equal(got, ctx.find_nearest(O, D), "after UPDATE_BOUNDS with the unchanged BVH arrays")


# 6. crt_tick: the frames rendered ahead are of the old scene
def test_tick_after_update_drops_frames_rendered_ahead(crt, orc, tmp_path):
    xml, hs, o, ctx, T = load(crt, orc, tmp_path, "tlas3")
    for spp in (1, 2, 3):
        ctx.tick(spp)                                                       # consecutive spp: frames 4.. are rendered ahead
    ctx.update_transforms_device(to_dev(T))
    move_oracle(o, T)
    ctx.clear(); o.clear(); o.set_spp(4)
    for spp in (4, 5):
        px, acc, energy = ctx.tick(spp)
        o.render(1, 4)
        assert np.array_equal(acc, o.accumulator()) and np.array_equal(px, o.screen()) and energy == o.energy()


# 7. a KD-tree BLAS set lives in object space: it is kept
def test_blas_kdtree_set_survives(crt, tmp_path):
    name = "ring40"
    xml = inp.scene_xml(tmp_path, name); T = inp.transforms(name)
    O, D = inp.aimed_rays(T)
    ctxs = []
    for route in ("device", "host"):
        hs = crt.HostScene(xml, 1, ASSETS); hs.build_alt(crt.ACCEL_KDTREE)
        ctx = crt.Context(W, H); hs.upload(ctx); hs.upload_alt(ctx, crt.ACCEL_KDTREE)
        if route == "device":
            ctx.update_transforms_device(to_dev(T))
        else:
            for i in range(len(T)):
                hs.set_transform(i, T[i])
            hs.update(ctx, crt.UPDATE_TRANSFORMS)
        ctxs.append(ctx)
    got = ctxs[0].find_nearest_alt(crt.ACCEL_KDTREE, O, D)
    assert_hits_equal(got, ctxs[1].find_nearest_alt(crt.ACCEL_KDTREE, O, D), "host route")
    assert (got["objIdx"] >= 2).sum() >= 200


# 8. the host front follows
def test_host_front_follows(crt, orc, tmp_path):
    xml, hs, o, ctx, T = load(crt, orc, tmp_path, "ring40")
    O, D = inp.aimed_rays(T)
    hs.set_transforms_device(ctx, to_dev(T))
    move_oracle(o, T)
    assert hs.tlas()[0].tobytes() == o.tlas()[0].tobytes() and hs.tlas()[1] == o.tlas()[1]
    for i in range(len(T)):
        for a, b in zip(hs.blas_transform(i), o.blas_transform(i)):
            assert a.tobytes() == b.tobytes(), i
    got = ctx.find_nearest(O, D)
    assert_hits_equal(got, o.find_nearest(O, D), "oracle")
    hs.update(ctx, crt.UPDATE_TRANSFORMS)                                    # the host scene's own arrays describe the same scene
    assert_hits_equal(got, ctx.find_nearest(O, D), "after the host's UPDATE_TRANSFORMS")
    with pytest.raises(ValueError):
        hs.set_transforms_device(ctx, torch.from_numpy(T))                  # a CPU tensor does not get as far as the ABI
    with pytest.raises(ValueError):
        hs.set_transforms_device(ctx, to_dev(T[:-1]))


def chain_blas(crt, n_tris, obj_idx):
    """a BLAS that is one long chain (height n_tris - 1) of small triangles along x"""
    tris = np.zeros(n_tris, crt.TRI_DTYPE)
    for k in range(n_tris):
        x = np.float32(-0.5 + 0.004 * k)
        tris["vertex0"][k] = (x, 0.0, 0.0); tris["vertex1"][k] = (x + np.float32(0.003), 0.0, 0.0); tris["vertex2"][k] = (x, 0.003, 0.0)
    for f in ("normal0", "normal1", "normal2"):
        tris[f] = (0.0, 0.0, -1.0)
    tris["objIdx"] = obj_idx
    lo = np.minimum(np.minimum(tris["vertex0"], tris["vertex1"]), tris["vertex2"]); hi = np.maximum(np.maximum(tris["vertex0"], tris["vertex1"]), tris["vertex2"])
    nodes = np.zeros(2 * n_tris - 1, crt.NODE_DTYPE)
    interior = 0
    for k in range(n_tris - 1):
        left = 2 * k + 1
        nodes[interior] = (lo[k:].min(0), hi[k:].max(0), left, 0)
        nodes[left] = (lo[k], hi[k], k, 1)
        if k == n_tris - 2:
            nodes[left + 1] = (lo[k + 1], hi[k + 1], k + 1, 1)
        interior = left + 1
    return dict(nodes=nodes, tris=tris, triIndices=np.arange(n_tris, dtype=np.uint32), objIdx=obj_idx, matIdx=0)


# 9. refusals: the code of each, and nothing modified
def test_refusals(crt, orc, tmp_path):
    L = crt.lib()
    xml, hs, o, ctx, T = load(crt, orc, tmp_path, "nan", oracle=False)
    good = T.copy(); good[5] = inp.rigid((0.0, 0.0, 5.0))
    O, D = inp.aimed_rays(good)
    before = ctx.find_nearest(O, D)
    d_good, d_nan = to_dev(good), to_dev(T)
    n = C.c_uint32(len(T))
    d = lambda x, off=0: C.c_void_p(x.data_ptr() + off)                      # noqa: E731

    def refused(rc, code, c=ctx):
        assert rc == code, (rc, code)
        assert len(L.crt_last_error(c.h)) > 0

    refused(L.crt_update_transforms_device(ctx.h, d(d_good), C.c_uint32(len(T) - 1), None, None), INVALID)        # blasCount
    refused(L.crt_update_transforms_device(ctx.h, None, n, None, None), INVALID)                                  # NULL
    refused(L.crt_update_transforms_device(ctx.h, d(d_good, 2), n, None, None), INVALID)                          # misaligned
    refused(L.crt_update_transforms_device(ctx.h, C.c_void_p(good.ctypes.data), n, None, None), INVALID)          # a host pointer
    if torch.cuda.device_count() > 1:                                       # memory / a stream of another device
        other = torch.device("cuda", 1)
        refused(L.crt_update_transforms_device(ctx.h, d(d_good.to(other)), n, None, None), INVALID)
        refused(L.crt_update_transforms_device(ctx.h, d(d_good), n, C.c_void_p(torch.cuda.Stream(device=other).cuda_stream), None), INVALID)
    with pytest.raises(crt.CrtError) as e:                                  # a NaN translation: FindBestMatch without a candidate while nodes are open
        ctx.update_transforms_device(d_nan)
    assert e.value.code == INVALID and "FindBestMatch" in str(e.value)
    with pytest.raises(ValueError):
        ctx.update_transforms_device(torch.from_numpy(good))
    assert_hits_equal(before, ctx.find_nearest(O, D), "after the refused calls")
    ctx.update_transforms_device(d_good)                                    # and the context still takes a good one
    assert any((ctx.find_nearest(O, D)[f] != before[f]).any() for f in ("t", "objIdx"))

    # no scene; a FileScene; a PrimitiveScene
    c2 = crt.Context(W, H)
    refused(L.crt_update_transforms_device(c2.h, d(d_good), n, None, None), STATE, c2)
    crt.HostScene(scene_path("cube_scene.xml"), 0, ASSETS).upload(c2)
    refused(L.crt_update_transforms_device(c2.h, d(d_good), C.c_uint32(1), None, None), INVALID, c2)
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(0.0)
    pc = crt.Context(W, H); ps.upload(pc)
    refused(L.crt_update_transforms_device(pc.h, d(d_good), n, None, None), UNSUPPORTED, pc)

    # a TLAS too high for the LDS budget of 241 stack entries: 16 chain BLAS of height 230 under the TLAS of a 4 x 4 grid fit (230 + 5 + 1), under the caterpillar
    # that transforms at x = 4^i make (230 + 15 + 1) they do not
    N, tris = 16, 231
    bvhs = [chain_blas(crt, tris, i + 2) for i in range(N)]
    boxes = np.stack([np.stack([b["nodes"][0]["aabbMin"], b["nodes"][0]["aabbMax"]]) for b in bvhs])
    flat = np.stack([inp.rigid((i % 4 - 1.5, i // 4 - 1.5, 5.0)) for i in range(N)])
    first = inp.restate(boxes, flat)
    assert first["height"] == 5
    for b, t, it in zip(bvhs, flat, first["invT"]):
        b.update(T=t, invT=it.reshape(4, 4))
    tex = np.full((4, 4), 0x808080, np.uint32); ident = np.eye(4, dtype=np.float32)
    c3 = crt.Context(W, H)
    c3.upload_desc(crt.SCENE_TLAS, bvhs, tlas_nodes=first["nodes"], textures=[tex, tex], floor_texture=0, sky_texture=1, materials=[(0.0, 0.0, (0.0, 0.0, 0.0), -1)],
                   light_T=ident, light_invT=ident)
    O3, D3 = inp.aimed_rays(flat, 500)
    before3 = c3.find_nearest(O3, D3)
    line = np.stack([inp.rigid((4.0 ** i, 0.0, 5.0)) for i in range(N)])
    assert inp.restate(boxes, line)["height"] == 15
    refused(L.crt_update_transforms_device(c3.h, d(to_dev(line)), C.c_uint32(N), None, None), UNSUPPORTED, c3)
    assert_hits_equal(before3, c3.find_nearest(O3, D3), "after the refused height")
