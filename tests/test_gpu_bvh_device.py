"""crt_build_bvh_device: BVH::Build / BLASBVH::Build (infra/bvh.cpp:63-178, binned SAH) on the GPU from vertex positions held in a torch tensor, and crt_get_bvh, which
reads a live BVH back in the reference's form.  Every comparison is exact.  The tree is held to the host build over the same positions (crt.host_bvh_build, which
tests/test_bvh_device_cpu.py holds to HostScene's own build and to the reference's); the scene the call leaves is held to a second context that uploaded the
host-rebuilt scene — the path the rest of the suite holds to the oracle: queries with their traversal counters, the Whitted inspection metrics, Sample and
renders — and, bit for bit, the WHOLE geometry buffer with the Scene words that describe it (crt_debug_geometry), which covers the pool form of every reference.
The oracle itself cannot stand in: it has no rebuild, and the tree its Refit leaves answers differently (node 1 keeps its stale box, bvh.cpp:28), so it only
supplies the camera's rays; where the reference's own bvh.cpp is built (oracle/_ref), its Build + Intersect over the moved triangles is the independent judge of
the nearest hits.  The helpers are those of tests/test_gpu_grid_device.py."""
import numpy as np
import pytest

from conftest import ASSETS, scene_path
import bvh_build_inputs as B

torch = pytest.importorskip("torch")

import test_gpu_grid_device as TG                                          # noqa: E402  (helpers only; a module object is not collected)

pytestmark = pytest.mark.gpu

BUNNY = "bunny_scene.xml"
to_dev, ray_records, hits_np, assert_hits_equal, positions, pixel_rays = TG.to_dev, TG.ray_records, TG.hits_np, TG.assert_hits_equal, TG.positions, TG.pixel_rays


def as_bvh(b):
    """HostScene.bvh's dict in Context.get_bvh's layout"""
    return dict(nodes=b["nodes"], indices=b["triIndices"], nodesUsed=b["nodesUsed"], maxDepth=b["maxDepth"])


def described(crt, p, t):
    """a host build `t` over positions p as upload_desc takes a BVH"""
    return dict(nodes=t["nodes"], tris=TG.tri_records(crt, p), triIndices=t["indices"], nodesUsed=t["nodesUsed"])


def centroid_rays(p, count=512):
    cen = p.mean(axis=1)[:count]; n = np.cross(p[:count, 1] - p[:count, 0], p[:count, 2] - p[:count, 0]); ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(ln > 0, n / np.where(ln > 0, ln, 1), [0, 0, 1]).astype(np.float32)
    return (cen + n * np.float32(0.05)).astype(np.float32), (-n).astype(np.float32)


def geometry(ctx):
    """(the Scene words that describe the geometry buffer, the buffer's bytes) as the device holds them"""
    import ctypes as C
    words = np.zeros(24, np.uint32); size = C.c_ulonglong()
    ctx._ck(ctx.L.crt_debug_geometry(ctx.h, words.ctypes.data_as(C.c_void_p), C.byref(size), None))
    buf = np.zeros(size.value, np.uint8)
    ctx._ck(ctx.L.crt_debug_geometry(ctx.h, None, C.byref(size), buf.ctypes.data_as(C.c_void_p)))
    return words, buf


def assert_same_scene(a, b, what):
    """offsets, root reference in both forms, root pair, stack depths; then every byte of the geometry buffer: pairs with ref and ref16, leaf triangles, TLAS nodes
    and pairs, instances with rootRef and rootRef16, shade records, the padding between them"""
    (wa, ga), (wb, gb) = geometry(a), geometry(b)
    assert wa.tolist() == wb.tolist(), (what, wa.tolist(), wb.tolist())
    assert ga.shape == gb.shape, (what, ga.shape, gb.shape)
    if not np.array_equal(ga, gb):
        bad = np.flatnonzero(ga != gb)
        raise AssertionError((what, "geometry bytes differ", len(bad), bad[:16].tolist(), wa.tolist()))


def assert_same_pictures(a, b, what):
    """the two contexts answer alike: the Whitted inspection with its metrics, then a 2-frame render"""
    (pa, ma), (pb, mb) = a.whitted_tick_inspect(1), b.whitted_tick_inspect(1)
    assert np.array_equal(pa, pb) and ma == mb, (what, ma, mb)
    a.clear(); b.clear()
    a.render(1, 2, 1); b.render(1, 2, 1)
    assert np.array_equal(a.accumulator().view(np.uint32), b.accumulator().view(np.uint32)), what


@pytest.fixture(scope="module")
def bunny(crt):
    """the bunny scene's positions, two deformations of them and the host builds over the first (computed once, never modified)"""
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS)
    p0 = positions(hs.bvh(0))
    moved = B.wobble(p0); moved2 = B.wobble(moved)
    for a in (p0, moved, moved2):
        a.setflags(write=False)
    return dict(p0=p0, moved=moved, moved2=moved2, built=crt.host_bvh_build(moved))


# 1. FileScene, every mesh: the tree equals the host build byte for byte, and the scene answers as a fresh upload of that build
@pytest.mark.parametrize("name", B.NAMES)
def test_file_scene_bvh_equals_the_host_build(crt, bunny, name):
    p = bunny["moved"] if name == "bunny_moved" else B.mesh(crt, name)
    want = bunny["built"] if name == "bunny_moved" else crt.host_bvh_build(p)
    ctx = crt.Context(32, 32)
    TG.upload_described(crt, ctx, TG.leaf_root_bvh(crt, p))
    t = to_dev(p)
    box = ctx.build_bvh_device(0, t)
    first = ctx.get_bvh()
    B.assert_bvh_equal(first, want, name)
    assert first["height"] == want["height"] == B.depths(want["nodes"]).max()
    assert box.tobytes() == np.stack([want["nodes"]["aabbMin"][0], want["nodes"]["aabbMax"][0]]).tobytes()
    if name in ("bunny_moved", "zeros-neg"):                                # two runs over the same input: identical bytes
        ctx.build_bvh_device(0, t)
        B.assert_bvh_equal(ctx.get_bvh(), first, "second run")
    c2 = crt.Context(32, 32)
    TG.upload_described(crt, c2, described(crt, p, want))
    O, D = centroid_rays(p)
    got, ref = ctx.find_nearest(O, D), c2.find_nearest(O, D)
    assert_hits_equal(got, ref, name)
    if name in ("bunny_moved", "pair", "three", "spanner"):
        assert (ref["objIdx"] >= 2).any(), name
    assert_same_scene(ctx, c2, name)
    assert_same_pictures(ctx, c2, name)


# 2. an uploaded BVH reads back as uploaded
def test_get_bvh_after_a_plain_upload(crt):
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS)
    ctx = crt.Context(32, 32)
    with pytest.raises(crt.CrtError) as e:
        ctx.get_bvh()
    assert e.value.code == -5
    hs.upload(ctx)
    b = hs.bvh(0)
    got = ctx.get_bvh()
    B.assert_bvh_equal(got, as_bvh(b), "uploaded")
    assert got["height"] == B.depths(b["nodes"]).max()
    with pytest.raises(crt.CrtError) as e:
        ctx.get_bvh(1)
    assert e.value.code == -1
    ht = crt.HostScene(scene_path("tlas_scene.xml"), 1, ASSETS)
    ct = crt.Context(32, 32); ht.upload(ct)
    for i in range(ht.bvh_count()):
        B.assert_bvh_equal(ct.get_bvh(i), as_bvh(ht.bvh(i)), "uploaded BLAS %d" % i)


# 3. the per-frame loop on the bunny: refit, rebuild, everything through the rebuilt tree; then a refit and a KD build on top of it
@pytest.mark.parametrize("kernel", ["default", "pool_always"])
def test_bunny_refit_rebuild_and_everything_through_the_new_tree(crt, orc, bunny, monkeypatch, kernel):
    if kernel != "default":
        monkeypatch.setenv("CRT_RENDER_KERNEL", kernel)
    W = H = 32
    xml = scene_path(BUNNY)
    moved, moved2 = bunny["moved"], bunny["moved2"]
    hs = crt.HostScene(xml, 0, ASSETS)
    ctx = crt.Context(W, H); hs.upload(ctx)
    t = to_dev(moved)
    ctx.refit_device(0, t)
    ctx.build_bvh_device(0, t)
    B.assert_bvh_equal(ctx.get_bvh(), bunny["built"], "device build")
    assert bunny["built"]["nodesUsed"] != hs.bvh(0)["nodesUsed"]             # the pair section changed size: every section behind it moved
    h2 = crt.HostScene(xml, 0, ASSETS); h2.move_and_rebuild(0, moved)
    B.assert_bvh_equal(as_bvh(h2.bvh(0)), bunny["built"], "host rebuild")
    c2 = crt.Context(W, H); h2.upload(c2)
    o, _ = orc.load_scene(xml, 0, ASSETS); o.renderer_init(W, H)
    O, D = pixel_rays(o, W, H, 64)
    rays = ray_records(crt, O, D)
    got, ref = hits_np(crt, ctx.find_nearest_device(rays)), hits_np(crt, c2.find_nearest_device(rays))
    torch.cuda.synchronize()
    assert_hits_equal(got, ref, "find_nearest_device")
    assert (ref["objIdx"] >= 2).sum() > 300
    assert_same_scene(ctx, c2, "after the rebuild")
    try:                                                                    # the reference's own Build + Intersect over the moved triangles, where it is built
        live = orc.Ref()
    except FileNotFoundError:
        live = None
    if live is not None:
        h, rb = live.bvh_build(B.tri_records(orc, moved))
        try:
            rh = live.bvh_intersect(h, O, D)
        finally:
            live.bvh_free(h)
        B.assert_bvh_equal(ctx.get_bvh(), dict(nodes=rb["nodes"], indices=rb["triIndices"], nodesUsed=rb["nodesUsed"], maxDepth=rb["maxDepth"]), "device build vs the reference")
        mesh = got["objIdx"] >= 2                                           # (the scene's floor and light are not the BVH's)
        assert (rh["t"][mesh] < 1e30).all()
        for f in ("t", "u", "v", "triIdx"):
            assert np.array_equal(np.asarray(got[f][mesh]).view(np.uint32), np.asarray(rh[f][mesh]).view(np.uint32)), f
    sub = slice(0, 4096, 4)
    tt = np.where(ref["objIdx"][sub] >= 0, ref["t"][sub] * np.float32(2), np.float32(100)).astype(np.float32)
    shadow = ray_records(crt, O[sub], D[sub], tt, crt.SHADOW_RAY_DTYPE)
    occ = ctx.is_occluded_device(shadow).cpu().numpy()
    assert np.array_equal(occ, c2.is_occluded_device(shadow).cpu().numpy()) and 0 < occ.sum() < len(occ)
    seeds = (np.arange(1024, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)) | np.uint32(1)
    sd = torch.from_numpy(seeds.view(np.int32).copy()).to(TG.dev())
    r1, s1 = ctx.sample_device(ray_records(crt, O[sub], D[sub]), seeds=sd)
    r2, s2 = c2.sample_device(ray_records(crt, O[sub], D[sub]), seeds=sd)
    assert torch.equal(r1.view(torch.int32), r2.view(torch.int32)) and torch.equal(s1, s2)
    assert_same_pictures(ctx, c2, "after the rebuild")
    for c in (ctx, c2):                                                     # the pool kernel reads the pool-form references: it must have rendered under pool_always
        assert (c.timing()["pool_launches"] > 0) == (kernel == "pool_always")
    # Refit on top of the rebuilt tree (the plan of the old topology is gone): the host's refit of the rebuilt tree
    t2 = to_dev(moved2)
    ctx.refit_device(0, t2)
    h2.move_and_refit(0, moved2)
    B.assert_bvh_equal(ctx.get_bvh(), as_bvh(h2.bvh(0)), "refit of the rebuilt tree")
    h2.upload(c2)
    assert_hits_equal(hits_np(crt, ctx.find_nearest_device(rays)), hits_np(crt, c2.find_nearest_device(rays)), "refitted")
    assert_same_scene(ctx, c2, "refitted")
    # ... and the KD-tree build reads the triangle ids of the rebuilt tree's leaf records
    ctx.build_kdtree_device(0, t2)
    import kd_build_inputs as K
    K.assert_kd_equal(ctx.get_kdtree(), crt.host_kd_build(moved2), "KD-tree after the rebuild")


# 4. a two-level scene: one BLAS rebuilt, the TLAS follows on the device; the other BLASes' records are carried over
def test_two_level_scene_follows_a_rebuilt_blas(crt, orc, monkeypatch):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")                  # the renders go through render_pool_kernel: the relocated BLASes' ref16, the instances' rootRef16
    W = H = 32
    xml = scene_path("tlas_scene.xml")
    hs = crt.HostScene(xml, 1, ASSETS)
    n = hs.bvh_count(); assert n == 3
    ctx = crt.Context(W, H); hs.upload(ctx)
    before = [as_bvh(hs.bvh(i)) for i in range(n)]
    p1 = positions(hs.bvh(1)); moved = B.wobble(p1); t1 = to_dev(moved)
    T = to_dev(np.stack([hs.blas_transform(i)[0] for i in range(n)]))
    want1 = crt.host_bvh_build(moved)
    assert want1["nodesUsed"] != before[1]["nodesUsed"]                      # the BLASes behind it move
    ctx.build_bvh_device(1, t1)
    ctx.update_transforms_device(T)
    B.assert_bvh_equal(ctx.get_bvh(1), want1, "the rebuilt BLAS")
    for i in (0, 2):
        B.assert_bvh_equal(ctx.get_bvh(i), before[i], "carried over %d" % i)
    h2 = crt.HostScene(xml, 1, ASSETS); h2.move_and_rebuild(1, moved)
    c2 = crt.Context(W, H); h2.upload(c2)
    o, _ = orc.load_scene(xml, 1, ASSETS); o.renderer_init(W, H)
    O, D = pixel_rays(o, W, H, 64)
    rays = ray_records(crt, O, D)
    ref = hits_np(crt, c2.find_nearest_device(rays))
    assert len(set(ref["objIdx"][ref["objIdx"] >= 2])) >= 2
    assert_hits_equal(hits_np(crt, ctx.find_nearest_device(rays)), ref, "two-level queries")
    assert_same_scene(ctx, c2, "two-level")
    assert_same_pictures(ctx, c2, "two-level")
    assert ctx.timing()["pool_launches"] > 0 and c2.timing()["pool_launches"] > 0
    # the host front's entry: device rebuild, host rebuild, the TLAS by the host route
    h3 = crt.HostScene(xml, 1, ASSETS)
    c3 = crt.Context(W, H); h3.upload(c3)
    h3.build_bvh_device(c3, 1, t1)
    B.assert_bvh_equal(as_bvh(h3.bvh(1)), want1, "host scene in step")
    for i in range(n):
        B.assert_bvh_equal(c3.get_bvh(i), c2.get_bvh(i), "host route, BLAS %d" % i)
    assert_hits_equal(hits_np(crt, c3.find_nearest_device(rays)), ref, "host route queries")
    assert_same_scene(c3, c2, "host route")
    assert_same_pictures(c3, c2, "host route")
    h3.upload(c3)                                                           # the host arrays are current: an upload of them changes nothing
    assert_hits_equal(hits_np(crt, c3.find_nearest_device(rays)), ref, "uploaded again")


# 5. ordering on one non-default stream, no host synchronisation in between: query, build, query
def test_build_is_ordered_between_two_queries_on_one_stream(crt, bunny):
    xml = scene_path(BUNNY)
    hs = crt.HostScene(xml, 0, ASSETS)
    ctx = crt.Context(32, 32); hs.upload(ctx)
    c_old = crt.Context(32, 32); hs.upload(c_old)
    h2 = crt.HostScene(xml, 0, ASSETS); h2.move_and_rebuild(0, bunny["moved"])
    c_new = crt.Context(32, 32); h2.upload(c_new)
    O, D = centroid_rays(bunny["moved"], 2048)
    rays = ray_records(crt, O, D); t = to_dev(bunny["moved"])
    s = torch.cuda.Stream(device=TG.dev())
    old = ctx.find_nearest_device(rays, stream=s)
    ctx.build_bvh_device(0, t, stream=s)
    new = ctx.find_nearest_device(rays, stream=s)
    torch.cuda.synchronize()
    want_old, want_new = hits_np(crt, c_old.find_nearest_device(rays)), hits_np(crt, c_new.find_nearest_device(rays))
    torch.cuda.synchronize()
    assert any((want_old[f] != want_new[f]).any() for f in ("t", "triIdx"))
    assert_hits_equal(hits_np(crt, old), want_old, "before the build: the old tree")
    assert_hits_equal(hits_np(crt, new), want_new, "after the build: the new tree")


# 6. refusals: the named status, and the tree and the picture stay
def test_refusals_leave_the_scene(crt, bunny):
    C = crt.C
    ctx = crt.Context(32, 32)
    good = to_dev(bunny["moved"])
    with pytest.raises(crt.CrtError) as e:                                  # no scene
        ctx.build_bvh_device(0, good)
    assert e.value.code == -5
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS); hs.upload(ctx)
    uploaded = as_bvh(hs.bvh(0))
    ctx.render(1, 2, 1); picture = ctx.accumulator().copy()

    def unchanged(what):
        B.assert_bvh_equal(ctx.get_bvh(), uploaded, what)
        ctx.clear(); ctx.render(1, 2, 1)
        assert np.array_equal(ctx.accumulator().view(np.uint32), picture.view(np.uint32)), what

    bad = bunny["moved"].copy(); bad[len(bad) // 2, 1, 2] = np.nan
    inf = bunny["moved"].copy(); inf[-1, 2, 0] = np.inf
    host = np.array(bunny["moved"])
    other = torch.cuda.Stream(device=TG.dev())
    cases = [("a NaN position", lambda: ctx.build_bvh_device(0, to_dev(bad)), -1),
             ("an infinite position", lambda: ctx.build_bvh_device(0, to_dev(inf)), -1),
             ("triCount off by one", lambda: ctx.build_bvh_device(0, good[:-1].contiguous()), -1),
             ("a NULL pointer", lambda: ctx._ck(ctx.L.crt_build_bvh_device(ctx.h, C.c_uint32(0), None, C.c_uint32(len(host)), C.c_void_p(other.cuda_stream), None)), -1),
             ("a host pointer", lambda: ctx._ck(ctx.L.crt_build_bvh_device(ctx.h, C.c_uint32(0), host.ctypes.data_as(C.c_void_p), C.c_uint32(len(host)), None, None)), -1),
             ("bvh out of range", lambda: ctx.build_bvh_device(1, good), -1)]
    for what, call, code in cases:
        with pytest.raises(crt.CrtError) as e:
            call()
        assert e.value.code == code, what
        unchanged(what)
    with pytest.raises(ValueError):                                         # a CPU tensor does not get as far as the ABI
        ctx.build_bvh_device(0, torch.from_numpy(host))
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(0.0)                   # a PrimitiveScene has no BVH
    pc = crt.Context(32, 32); ps.upload(pc)
    for call in (lambda: pc.build_bvh_device(0, good), lambda: pc.get_bvh()):
        with pytest.raises(crt.CrtError) as e:
            call()
        assert e.value.code == -4
    ctx.build_bvh_device(0, good)                                           # and after all that a good call still works
    B.assert_bvh_equal(ctx.get_bvh(), bunny["built"], "a good call after the refusals")


# 7. the refusal of a tree too tall for the traversal stack.  No float mesh is 230 levels tall, so the context's LDS is made scarce instead (CRT_DEBUG_EXTRA_LDS, read by
# the upload): 59136 unused bytes leave room for a stack of 10 entries, the upload's leaf root needs 1, and the `chain` mesh builds a tree of height 18
def test_a_tree_too_tall_for_the_stack_is_refused(crt, monkeypatch):
    monkeypatch.setenv("CRT_DEBUG_EXTRA_LDS", "59136")
    p = B.chain()
    assert crt.host_bvh_build(p)["height"] == 18
    ctx = crt.Context(32, 32)
    TG.upload_described(crt, ctx, TG.leaf_root_bvh(crt, p))
    before = ctx.get_bvh(); words, geom = geometry(ctx)
    ctx.render(1, 2, 1); picture = ctx.accumulator().copy()
    with pytest.raises(crt.CrtError) as e:
        ctx.build_bvh_device(0, to_dev(p))
    assert e.value.code == -4
    B.assert_bvh_equal(ctx.get_bvh(), before, "refused")
    w2, g2 = geometry(ctx)
    assert w2.tolist() == words.tolist() and np.array_equal(g2, geom)
    ctx.clear(); ctx.render(1, 2, 1)
    assert np.array_equal(ctx.accumulator().view(np.uint32), picture.view(np.uint32))
    small = B.GENERATED["three"]()                                           # and a tree that fits is still built: height 1 over a scene of 3 triangles
    c2 = crt.Context(32, 32)
    TG.upload_described(crt, c2, TG.leaf_root_bvh(crt, small))
    c2.build_bvh_device(0, to_dev(small))
    B.assert_bvh_equal(c2.get_bvh(), crt.host_bvh_build(small), "fits")
