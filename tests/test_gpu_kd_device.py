"""crt_build_kdtree_device: KDTree::Build / BLASKDTree::Build (infra/kdtree.cpp:4-108) on the GPU from vertex positions held in a torch tensor, and crt_get_kdtree,
which reads the live tree back.  Every comparison is exact: the arrays against the host build over the same positions (which tests/test_kd_device_cpu.py holds to
the oracle's restatement of kdtree.cpp and to the reference's own), the queries, Sample and the renders against the oracle walking ITS KD-tree over the moved
triangles.  The helpers are those of tests/test_gpu_grid_device.py, whose tests these mirror."""
import numpy as np
import pytest

from conftest import ASSETS, scene_path
import kd_build_inputs as K

torch = pytest.importorskip("torch")

import test_gpu_grid_device as TG                                          # noqa: E402  (helpers only; a module object is not collected)

pytestmark = pytest.mark.gpu

KD, GRID = 1, 2
BUNNY = "bunny_scene.xml"
to_dev, ray_records, hits_np, assert_hits_equal, positions, pixel_rays = TG.to_dev, TG.ray_records, TG.hits_np, TG.assert_hits_equal, TG.positions, TG.pixel_rays


def state_error(call):
    with pytest.raises(Exception) as e:
        call()
    assert getattr(e.value, "code", None) == -5, e.value


@pytest.fixture(scope="module")
def bunny(crt):
    """the bunny scene's host BVH, its positions, and the moved positions with the host build over them (computed once, never modified)"""
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS)
    b = hs.bvh(0)
    for a in b.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    moved = K.wobble(positions(b)); moved.setflags(write=False)
    return dict(bvh=b, p0=positions(b), moved=moved, kd_moved=crt.host_kd_build(moved))


def bunny_bvh(bunny, tris=None):
    b = bunny["bvh"]
    return dict(nodes=b["nodes"], tris=b["tris"] if tris is None else tris, triIndices=b["triIndices"], nodesUsed=b["nodesUsed"])


# 1. FileScene, every mesh: the arrays equal the host build byte for byte
@pytest.mark.parametrize("name", K.NAMES)
def test_file_scene_kdtree_equals_the_host_build(crt, bunny, name):
    ctx = crt.Context(64, 64)
    if name == "bunny_moved":
        p, want = bunny["moved"], bunny["kd_moved"]
        TG.upload_described(crt, ctx, bunny_bvh(bunny))
    else:
        p = K.mesh(crt, name); want = crt.host_kd_build(p)
        TG.upload_described(crt, ctx, TG.leaf_root_bvh(crt, p))
    state_error(lambda: ctx.get_kdtree())                                   # nothing uploaded, nothing built yet
    t = to_dev(p)
    ctx.build_kdtree_device(0, t)
    first = ctx.get_kdtree()
    K.assert_kd_equal(first, want, name)
    assert first["height"] == K.depths(want["nodes"]).max()
    if name in ("bunny_moved", "zeros-neg"):                                # two runs over the same input: identical bytes
        ctx.build_kdtree_device(0, t)
        K.assert_kd_equal(ctx.get_kdtree(), first, "second run")
    # the triangle records are of these positions: a ray at each triangle's centroid, from just in front of it, gets the answer of a host-uploaded copy of the tree
    c2 = crt.Context(64, 64)
    b2 = TG.leaf_root_bvh(crt, p) if name != "bunny_moved" else bunny_bvh(bunny, TG.tri_records(crt, p))
    TG.upload_described(crt, c2, b2)
    a = crt.alt_desc(KD, b2["tris"], want)
    c2._ck(c2.L.crt_upload_alt_accel(c2.h, crt.C.byref(a)))
    cen = p.mean(axis=1)[:512]; n = np.cross(p[:512, 1] - p[:512, 0], p[:512, 2] - p[:512, 0]); ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(ln > 0, n / np.where(ln > 0, ln, 1), [0, 0, 1]).astype(np.float32)
    O = (cen + n * np.float32(0.05)).astype(np.float32); D = (-n).astype(np.float32)
    got, ref = ctx.find_nearest_alt(KD, O, D), c2.find_nearest_alt(KD, O, D)
    assert_hits_equal(got, ref, name)
    if name in ("bunny_moved", "sliver", "spanner", "three"):
        assert (ref["objIdx"] >= 2).any(), name                             # (the KD walk drops rays with a zero direction component: not every mesh's rays hit)


# 2. an uploaded tree reads back as uploaded
def test_get_kdtree_after_a_plain_upload(crt):
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS)
    kd = hs.build_alt(KD)
    ctx = crt.Context(64, 64); hs.upload(ctx)
    state_error(lambda: ctx.get_kdtree())
    hs.upload_alt(ctx, KD)
    got = ctx.get_kdtree()
    K.assert_kd_equal(got, kd, "uploaded")
    assert got["height"] == K.depths(kd["nodes"]).max()
    with pytest.raises(crt.CrtError) as e:
        ctx.get_kdtree(1)
    assert e.value.code == -1


# 3. the per-frame loop on the bunny: refit, rebuild, query / Sample / render through the KD-tree, against the oracle
def test_bunny_refit_rebuild_and_everything_through_the_kdtree(crt, orc, bunny):
    W = H = 32
    xml = scene_path(BUNNY)
    hs = crt.HostScene(xml, 0, ASSETS); hs.build_alt(KD)
    ctx = crt.Context(W, H); hs.upload(ctx); hs.upload_alt(ctx, KD)
    ctx.set_render_accel(KD)                                                # selected BEFORE the rebuild: it must stay
    moved = bunny["moved"]; t = to_dev(moved)
    ctx.refit_device(0, t)
    ctx.build_kdtree_device(0, t)
    assert ctx.L.crt_debug_render_accel(ctx.h) == KD
    o, _ = orc.load_scene(xml, 0, ASSETS); o.renderer_init(W, H)
    o.move_and_refit(0, moved)
    acc = orc.alt_accel("kd", o.bvh(0)["tris"]); orc.set_render_accel(o, acc)
    K.assert_kd_equal(ctx.get_kdtree(), acc.dump(), "oracle's KD-tree over the moved triangles")
    O, D = pixel_rays(o, W, H, 64)
    want = o.find_nearest(O, D)
    assert (want["objIdx"] >= 2).sum() > 300
    got = hits_np(crt, ctx.find_nearest_device(ray_records(crt, O, D), accel=KD))
    torch.cuda.synchronize()
    assert_hits_equal(got, want, "find_nearest_device")
    # occlusion: 1024 rays, bounded at twice the nearest hit (misses: far away)
    sub = slice(0, 4096, 4)
    tt = np.where(want["objIdx"][sub] >= 0, want["t"][sub] * np.float32(2), np.float32(100)).astype(np.float32)
    occ = ctx.is_occluded_device(ray_records(crt, O[sub], D[sub], tt, crt.SHADOW_RAY_DTYPE), accel=KD).cpu().numpy()
    want_occ = o.is_occluded(O[sub], D[sub], tt)
    assert np.array_equal(occ, want_occ) and 0 < want_occ.sum() < len(want_occ)
    # Sample
    seeds = (np.arange(1024, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)) | np.uint32(1)
    rgb, sout = ctx.sample_device(ray_records(crt, O[sub], D[sub]), seeds=torch.from_numpy(seeds.view(np.int32).copy()).to(TG.dev()), accel=KD)
    rgb = rgb.cpu().numpy(); sout = sout.cpu().numpy().view(np.uint32)
    for i in range(1024):
        w, s = o.sample(O[sub][i], D[sub][i], int(seeds[i]))
        assert np.array_equal(rgb[i].view(np.uint32), w.view(np.uint32)) and int(sout[i]) == s, i
    # a 2-frame render with the accelerator still selected from before the rebuild
    ctx.render(1, 2, 1); o.render(2, 4)
    assert np.array_equal(ctx.accumulator(), o.accumulator())
    acc.close()


# 4. ordering on one non-default stream, no host synchronisation in between: query, build, query
def test_build_is_ordered_between_two_queries_on_one_stream(crt, orc, bunny):
    xml = scene_path(BUNNY)
    hs = crt.HostScene(xml, 0, ASSETS); hs.build_alt(KD)
    ctx = crt.Context(32, 32); hs.upload(ctx); hs.upload_alt(ctx, KD)
    o, _ = orc.load_scene(xml, 0, ASSETS); o.renderer_init(32, 32)
    O, D = pixel_rays(o, 32, 32, 64)
    rays = ray_records(crt, O, D); t = to_dev(bunny["moved"])
    s = torch.cuda.Stream(device=TG.dev())
    old = ctx.find_nearest_device(rays, accel=KD, stream=s)
    ctx.build_kdtree_device(0, t, stream=s)
    new = ctx.find_nearest_device(rays, accel=KD, stream=s)
    torch.cuda.synchronize()
    a0 = orc.alt_accel("kd", o.bvh(0)["tris"]); orc.set_render_accel(o, a0)
    want_old = o.find_nearest(O, D)
    o.move_and_refit(0, bunny["moved"])
    a1 = orc.alt_accel("kd", o.bvh(0)["tris"]); orc.set_render_accel(o, a1)
    want_new = o.find_nearest(O, D)
    assert any((want_old[f] != want_new[f]).any() for f in ("t", "triIdx"))
    assert_hits_equal(hits_np(crt, old), want_old, "before the build: the old tree")
    assert_hits_equal(hits_np(crt, new), want_new, "after the build: the new tree")
    orc.set_render_accel(o, None); a0.close(); a1.close()


# 5. the grid shares the triangle records: a KD rebuild marks it absent, a grid rebuild marks the KD-tree absent
def test_kdtree_and_grid_rebuilds_mark_each_other_absent(crt, bunny):
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS); hs.build_alt(KD); hs.build_alt(GRID)
    ctx = crt.Context(32, 32); hs.upload(ctx); hs.upload_alt(ctx, KD); hs.upload_alt(ctx, GRID)
    one = (np.zeros((1, 3), np.float32), np.array([[0, 0, 1]], np.float32))
    ctx.set_render_accel(GRID)
    ctx.find_nearest_alt(GRID, *one); ctx.find_nearest_alt(KD, *one)
    t = to_dev(bunny["moved"])
    hs.build_kdtree_device(ctx, 0, t)                                       # the host front's entry: the mirror follows
    state_error(lambda: ctx.find_nearest_alt(GRID, *one))
    state_error(lambda: ctx.get_grid())
    assert ctx.L.crt_debug_render_accel(ctx.h) == 0
    mirror = hs.kdtree()
    K.assert_kd_equal(mirror, bunny["kd_moved"], "host mirror")
    assert (mirror["maxDepth"], mirror["nodesUsed"]) == (bunny["kd_moved"]["maxDepth"], bunny["kd_moved"]["nodesUsed"])
    state_error(lambda: hs.upload_alt(ctx, KD))                             # the mirror's triangles are the host's old ones: it is not uploaded as it stands
    K.assert_kd_equal(ctx.get_kdtree(), bunny["kd_moved"], "device")
    ctx.set_render_accel(KD)
    ctx.build_grid_device(0, t)                                             # ... and the reverse
    state_error(lambda: ctx.find_nearest_alt(KD, *one))
    state_error(lambda: ctx.get_kdtree())
    assert ctx.L.crt_debug_render_accel(ctx.h) == 0
    ctx.find_nearest_alt(GRID, *one)
    ctx.build_kdtree_device(0, t)                                           # a device-built tree after a device-built grid
    K.assert_kd_equal(ctx.get_kdtree(), bunny["kd_moved"], "rebuilt after the grid")
    state_error(lambda: ctx.get_grid())
    k0 = hs.build_alt(KD); hs.upload_alt(ctx, KD)                           # built from the host's triangles again: uploaded as ever
    K.assert_kd_equal(ctx.get_kdtree(), k0, "host build uploaded again")


# 6. a two-level scene: the set is dropped by a refit and live again after the rebuild
def test_two_level_set_follows_a_moved_blas(crt, orc):
    W = H = 32
    xml = scene_path("tlas_scene.xml")
    hs = crt.HostScene(xml, 1, ASSETS)
    uploaded = hs.build_alt(KD)
    n = hs.bvh_count(); assert n == 3
    ctx = crt.Context(W, H); hs.upload(ctx); hs.upload_alt(ctx, KD)
    for i in range(n):
        K.assert_kd_equal(ctx.get_kdtree(i), uploaded[i], "uploaded %d" % i)
    o, _ = orc.load_scene(xml, 1, ASSETS); o.renderer_init(W, H)
    O, D = pixel_rays(o, W, H, 64); rays = ray_records(crt, O, D)
    p = [positions(hs.bvh(i)) for i in range(n)]
    moved = K.wobble(p[1]); t1 = to_dev(moved)
    T = to_dev(np.stack([hs.blas_transform(i)[0] for i in range(n)]))
    ctx.refit_device(1, t1)
    state_error(lambda: ctx.find_nearest_device(rays, accel=KD))            # dropped, as before this entry existed
    state_error(lambda: ctx.get_kdtree(1))
    ctx.update_transforms_device(T)
    ctx.build_kdtree_device(1, t1)
    want1 = crt.host_kd_build(moved)
    K.assert_kd_equal(ctx.get_kdtree(1), want1, "the rebuilt BLAS")
    assert ctx.get_kdtree(1)["height"] == K.depths(want1["nodes"]).max()
    for i in (0, 2):
        K.assert_kd_equal(ctx.get_kdtree(i), uploaded[i], "carried over %d" % i)
    o.move_and_refit(1, moved)
    accels = orc.blas_accels(o, "kd"); orc.set_blas_accel(o, accels)
    K.assert_kd_equal(ctx.get_kdtree(1), accels[1].dump(), "oracle's KD-tree of the moved BLAS")
    want = o.find_nearest(O, D)
    assert len(set(want["objIdx"][want["objIdx"] >= 2])) >= 2
    got = hits_np(crt, ctx.find_nearest_device(rays, accel=KD))
    assert_hits_equal(got, want, "find_nearest_device through the rebuilt set")
    ctx.set_render_accel(KD)
    px = ctx.whitted_tick(); o.whitted(2)
    assert np.array_equal(px, o.screen()) and np.array_equal(ctx.accumulator(), o.accumulator())
    # CRT_UPDATE_BOUNDS (here: the host scene's original vertices again) clears every flag: the set is live only once all three have been rebuilt
    hs.update(ctx, crt.UPDATE_BOUNDS)
    for i in (2, 0):
        ctx.build_kdtree_device(i, to_dev(p[i]))
        state_error(lambda: ctx.find_nearest_device(rays, accel=KD))
    ctx.build_kdtree_device(1, to_dev(p[1]))
    for i in range(n):
        K.assert_kd_equal(ctx.get_kdtree(i), uploaded[i], "original positions, BLAS %d" % i)
    o2, _ = orc.load_scene(xml, 1, ASSETS); o2.renderer_init(W, H)
    a2 = orc.blas_accels(o2, "kd"); orc.set_blas_accel(o2, a2)
    assert_hits_equal(hits_np(crt, ctx.find_nearest_device(rays, accel=KD)), o2.find_nearest(O, D), "all three rebuilt")
    # the host front's entry refreshes its mirror of the BLAS
    hs.build_kdtree_device(ctx, 1, t1)
    K.assert_kd_equal(hs.blas_alt(KD, 1), want1, "host mirror")
    orc.set_blas_accel(o, None); orc.set_blas_accel(o2, None)
    for a in accels + a2:
        a.close()


# 7. the three device writers chained on three streams, queries in flight on a fourth, a render behind them: no host synchronisation until the end
def test_refit_transforms_and_kdtree_chain_on_separate_streams(crt, orc):
    W = H = 32
    xml = scene_path("tlas_scene.xml")
    hs = crt.HostScene(xml, 1, ASSETS); hs.build_alt(KD)
    n = hs.bvh_count(); assert n == 3
    ctx = crt.Context(W, H); hs.upload(ctx); hs.upload_alt(ctx, KD)
    o, _ = orc.load_scene(xml, 1, ASSETS); o.renderer_init(W, H)
    O, D = pixel_rays(o, W, H, 64); rays = ray_records(crt, O, D)
    moved = K.wobble(positions(hs.bvh(1))); t1 = to_dev(moved)
    T = to_dev(np.stack([hs.blas_transform(i)[0] for i in range(n)]))
    s_q, s1, s2, s3 = (torch.cuda.Stream(device=TG.dev()) for _ in range(4))
    old = ctx.find_nearest_device(rays, stream=s_q)
    ctx.refit_device(1, t1, stream=s1)
    ctx.update_transforms_device(T, stream=s2)
    ctx.build_kdtree_device(1, t1, stream=s3)
    new_bvh = ctx.find_nearest_device(rays, stream=s_q)
    new_kd = ctx.find_nearest_device(rays, accel=KD, stream=s_q)
    px, acc, energy = ctx.tick(1)
    torch.cuda.synchronize()
    want_old = o.find_nearest(O, D)
    o.move_and_refit(1, moved)
    want_bvh = o.find_nearest(O, D)
    o.render(1, 4)
    accels = orc.blas_accels(o, "kd"); orc.set_blas_accel(o, accels)
    want_kd = o.find_nearest(O, D)
    orc.set_blas_accel(o, None)
    for a in accels:
        a.close()
    old, new_bvh = hits_np(crt, old), hits_np(crt, new_bvh)
    assert any((old[f] != new_bvh[f]).any() for f in ("t", "triIdx")), "the second query never saw the update"
    assert_hits_equal(old, want_old, "in flight before the chain: the unmoved scene")
    assert_hits_equal(new_bvh, want_bvh, "behind the chain: the refitted BVH under the rebuilt TLAS")
    assert_hits_equal(hits_np(crt, new_kd), want_kd, "behind the chain: the rebuilt KD set")
    assert np.array_equal(acc, o.accumulator()), "the Tick behind the chain: one frame of the moved scene"


# 8. refusals: the named status, and the previous tree keeps answering bit-identically.  (Three refusals of the header cannot be reached with a test-sized input and
# are not provoked: more than 2^31-1 references, a two-level stack beyond the LDS budget — 21 levels + a 3-instance TLAS fit by far — and a failed allocation.)
def test_refusals_leave_the_previous_tree(crt, bunny):
    C = crt.C
    ctx = crt.Context(32, 32)
    p0 = bunny["p0"]; good = to_dev(bunny["moved"])
    state_error(lambda: ctx.build_kdtree_device(0, good))                   # no scene
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS); kd = hs.build_alt(KD)
    hs.upload(ctx); hs.upload_alt(ctx, KD)
    rng = np.random.default_rng(5)
    lo, hi = p0.reshape(-1, 3).min(0), p0.reshape(-1, 3).max(0)
    O = (rng.uniform(lo - 1, hi + 1, (1500, 3))).astype(np.float32)
    D = rng.normal(size=(1500, 3)); D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(np.float32)
    before = ctx.find_nearest_alt(KD, O, D)
    assert (before["objIdx"] >= 2).sum() > 50

    def unchanged(what):
        assert_hits_equal(ctx.find_nearest_alt(KD, O, D), before, what)
        K.assert_kd_equal(ctx.get_kdtree(), kd, what)

    bad = bunny["moved"].copy(); bad[len(bad) // 2, 1, 2] = np.nan
    inf = bunny["moved"].copy(); inf[-1, 2, 0] = np.inf
    host = np.array(bunny["moved"])                                          # (a writable copy)
    other = torch.cuda.Stream(device=TG.dev())
    cases = [("a NaN position", lambda: ctx.build_kdtree_device(0, to_dev(bad)), -1),
             ("an infinite position", lambda: ctx.build_kdtree_device(0, to_dev(inf)), -1),
             ("triCount off by one", lambda: ctx.build_kdtree_device(0, good[:-1].contiguous()), -1),
             ("a NULL pointer", lambda: ctx._ck(ctx.L.crt_build_kdtree_device(ctx.h, C.c_uint32(0), None, C.c_uint32(len(host)), C.c_void_p(other.cuda_stream))), -1),
             ("a host pointer", lambda: ctx._ck(ctx.L.crt_build_kdtree_device(ctx.h, C.c_uint32(0), host.ctypes.data_as(C.c_void_p), C.c_uint32(len(host)), None)), -1),
             ("bvh out of range", lambda: ctx.build_kdtree_device(1, good), -1)]
    if torch.cuda.device_count() > 1:                                        # memory / a stream of another device
        far = torch.from_numpy(host).to(torch.device("cuda", 1)); far_stream = torch.cuda.Stream(device=torch.device("cuda", 1))
        cases.append(("memory of another device", lambda: ctx._ck(ctx.L.crt_build_kdtree_device(ctx.h, C.c_uint32(0), C.c_void_p(far.data_ptr()), C.c_uint32(len(host)), None)), -1))
        cases.append(("a stream of another device", lambda: ctx._ck(ctx.L.crt_build_kdtree_device(ctx.h, C.c_uint32(0), C.c_void_p(good.data_ptr()), C.c_uint32(len(host)),
                                                                                                  C.c_void_p(far_stream.cuda_stream))), -1))
    for what, call, code in cases:
        with pytest.raises(crt.CrtError) as e:
            call()
        assert e.value.code == code, what
        unchanged(what)
    with pytest.raises(ValueError):                                         # a CPU tensor does not get as far as the ABI
        ctx.build_kdtree_device(0, torch.from_numpy(host))
    # a two-level scene without an uploaded KD set (a grid set does not count)
    ht = crt.HostScene(scene_path("tlas_scene.xml"), 1, ASSETS)
    ct = crt.Context(32, 32); ht.upload(ct)
    state_error(lambda: ct.build_kdtree_device(0, to_dev(positions(ht.bvh(0)))))
    ht.build_alt(GRID); ht.upload_alt(ct, GRID)
    state_error(lambda: ct.build_kdtree_device(0, to_dev(positions(ht.bvh(0)))))
    state_error(lambda: ct.get_kdtree(0))
    # a PrimitiveScene has no triangles
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(0.0)
    pc = crt.Context(32, 32); ps.upload(pc)
    with pytest.raises(crt.CrtError) as e:
        pc.build_kdtree_device(0, good)
    assert e.value.code == -4
    # and after all that a good call still works
    ctx.build_kdtree_device(0, good)
    K.assert_kd_equal(ctx.get_kdtree(), bunny["kd_moved"], "a good call after the refusals")
