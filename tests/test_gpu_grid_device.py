"""crt_build_grid_device: Grid::Build / BLASGrid::Build (infra/grid.cpp:4-50) on the GPU from vertex positions held in a torch tensor, and crt_get_grid, which reads
the live grid back.  Every comparison is exact: the arrays against the host build over the same positions (which tests/test_grid_device_cpu.py holds to the
oracle's restatement of grid.cpp), the queries, Sample and the renders against the oracle walking ITS grid over the moved triangles
(orc_bvh_move_and_refit, orc_grid_build, orc_set_render_accel / orc_set_blas_accel)."""
import numpy as np
import pytest

from conftest import ASSETS, scene_path
import grid_build_inputs as G

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FIELDS = ("t", "u", "v", "objIdx", "triIdx", "traversed", "tested")
GRID = 2
BUNNY = "bunny_scene.xml"


def dev():
    return torch.device("cuda", 0)


def to_dev(a):
    t = torch.from_numpy(np.array(a, np.float32)).to(dev())               # (a copy: the shared inputs are read-only)
    torch.cuda.synchronize()
    return t


def ray_records(crt, O, D, last=None, dtype=None):
    r = np.zeros(len(O), dtype or crt.RAY_DTYPE)
    r["O"], r["D"] = O, D
    if last is not None:
        r["t"] = last
    t = torch.from_numpy(r.view(np.float32).reshape(-1, 7).copy()).to(dev())
    torch.cuda.synchronize()
    return t


def hits_np(crt, h):
    return h.cpu().numpy().view(crt.HIT_DTYPE).reshape(-1)


def assert_hits_equal(a, b, what):
    for f in FIELDS:
        assert np.array_equal(np.asarray(a[f]).view(np.uint32), np.asarray(b[f]).view(np.uint32)), (what, f)


def positions(b):
    t = b["tris"]
    return np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1).astype(np.float32)


def pixel_rays(o, W, H, per_axis):
    """per_axis^2 primary rays of the oracle's camera, spread evenly over the W x H image"""
    u = (np.arange(per_axis, dtype=np.float32) + np.float32(0.5)) * np.float32(W / per_axis)
    v = (np.arange(per_axis, dtype=np.float32) + np.float32(0.5)) * np.float32(H / per_axis)
    xy = np.stack(np.meshgrid(u, v), axis=-1).reshape(-1, 2)
    return o.primary_rays(xy)


def tri_records(crt, p, obj=2):
    tris = np.zeros(len(p), crt.TRI_DTYPE)
    tris["vertex0"], tris["vertex1"], tris["vertex2"] = p[:, 0], p[:, 1], p[:, 2]
    for k in ("normal0", "normal1", "normal2"):
        tris[k] = [0, 0, -1]
    tris["objIdx"] = obj
    return tris


def upload_described(crt, ctx, bvh):
    """a FileScene through upload_desc (INTEGRATION path A): one object, one untextured material, small textures"""
    tex = np.full((4, 4), 0x808080, np.uint32); ident = np.eye(4, dtype=np.float32)
    lt = ident.copy(); lt[:3, 3] = (0, 3, 1); li = ident.copy(); li[:3, 3] = (0, -3, -1)
    ctx.upload_desc(crt.SCENE_FILE, [bvh], textures=[tex, tex], floor_texture=0, sky_texture=1, materials=[(0.0, 0.0, (0.0, 0.0, 0.0), -1)], light_T=lt, light_invT=li,
                    obj_mat_idx=[0])


def leaf_root_bvh(crt, p):
    """the smallest BVH the host can build over any triangle array: node 0 is a leaf with all of them, in reverse order (leaf slot j holds triangle n - 1 - j, so the
    device's triangle records have to follow the references, not the slots)"""
    nodes = np.zeros(1, crt.NODE_DTYPE)
    nodes["aabbMin"][0] = p.reshape(-1, 3).min(0); nodes["aabbMax"][0] = p.reshape(-1, 3).max(0); nodes["leftFirst"] = 0; nodes["triCount"] = len(p)
    return dict(nodes=nodes, tris=tri_records(crt, p), triIndices=np.arange(len(p), dtype=np.uint32)[::-1].copy())


@pytest.fixture(scope="module")
def bunny(crt):
    """the bunny scene's host BVH, its positions, and the moved positions with the host build over them (computed once, never modified)"""
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS)
    b = hs.bvh(0)
    for a in b.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    moved = G.wobble(positions(b)); moved.setflags(write=False)
    return dict(bvh=b, p0=positions(b), moved=moved, grid_moved=crt.host_grid_build(moved))


# 1. FileScene, every mesh: the arrays equal the host build byte for byte
@pytest.mark.parametrize("name", G.NAMES)
def test_file_scene_grid_equals_the_host_build(crt, bunny, name):
    ctx = crt.Context(64, 64)
    if name == "bunny_moved":
        p, want = bunny["moved"], bunny["grid_moved"]
        b = bunny["bvh"]
        upload_described(crt, ctx, dict(nodes=b["nodes"], tris=b["tris"], triIndices=b["triIndices"], nodesUsed=b["nodesUsed"]))
    else:
        p = G.mesh(crt, name); want = crt.host_grid_build(p)
        upload_described(crt, ctx, leaf_root_bvh(crt, p))
    with pytest.raises(crt.CrtError) as e:                                  # nothing uploaded, nothing built yet
        ctx.get_grid()
    assert e.value.code == -5
    t = to_dev(p)
    ctx.build_grid_device(0, t)
    first = ctx.get_grid()
    G.assert_grids_equal(first, want, name)
    if name == "bunny_moved":                                               # an order-dependent fill would show between two runs
        ctx.build_grid_device(0, t)
        G.assert_grids_equal(ctx.get_grid(), first, "second run")
    # the triangle records are of these positions: a ray at each triangle's centroid, from just in front of it, hits at the grid's answer of a host-uploaded copy
    c2 = crt.Context(64, 64)
    b2 = leaf_root_bvh(crt, p) if name != "bunny_moved" else dict(nodes=bunny["bvh"]["nodes"], tris=tri_records(crt, p), triIndices=bunny["bvh"]["triIndices"],
                                                                  nodesUsed=bunny["bvh"]["nodesUsed"])
    upload_described(crt, c2, b2)
    a = crt.alt_desc(GRID, b2["tris"], want)
    c2._ck(c2.L.crt_upload_alt_accel(c2.h, crt.C.byref(a)))
    cen = p.mean(axis=1)[:512]; n = np.cross(p[:512, 1] - p[:512, 0], p[:512, 2] - p[:512, 0]); ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(ln > 0, n / np.where(ln > 0, ln, 1), [0, 0, 1]).astype(np.float32)
    O = (cen + n * np.float32(0.05)).astype(np.float32); D = (-n).astype(np.float32)
    assert_hits_equal(ctx.find_nearest_alt(GRID, O, D), c2.find_nearest_alt(GRID, O, D), name)


# 2. an uploaded grid reads back as uploaded
def test_get_grid_after_a_plain_upload(crt):
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS)
    g = hs.build_alt(GRID)
    ctx = crt.Context(64, 64); hs.upload(ctx)
    with pytest.raises(crt.CrtError) as e:
        ctx.get_grid()
    assert e.value.code == -5
    hs.upload_alt(ctx, GRID)
    G.assert_grids_equal(ctx.get_grid(), g, "uploaded")
    with pytest.raises(crt.CrtError) as e:
        ctx.get_grid(1)
    assert e.value.code == -1


# 3. the per-frame loop on the bunny: refit, rebuild, query / Sample / render through the grid, against the oracle
def test_bunny_refit_rebuild_and_everything_through_the_grid(crt, orc, bunny):
    W = H = 32
    xml = scene_path(BUNNY)
    hs = crt.HostScene(xml, 0, ASSETS); hs.build_alt(GRID)
    ctx = crt.Context(W, H); hs.upload(ctx); hs.upload_alt(ctx, GRID)
    ctx.set_render_accel(GRID)                                              # selected BEFORE the rebuild: it must stay
    moved = bunny["moved"]; t = to_dev(moved)
    ctx.refit_device(0, t)
    ctx.build_grid_device(0, t)
    assert ctx.L.crt_debug_render_accel(ctx.h) == GRID
    o, _ = orc.load_scene(xml, 0, ASSETS); o.renderer_init(W, H)
    o.move_and_refit(0, moved)
    acc = orc.alt_accel("grid", o.bvh(0)["tris"]); orc.set_render_accel(o, acc)
    G.assert_grids_equal(ctx.get_grid(), acc.dump(), "oracle's grid over the moved triangles")
    O, D = pixel_rays(o, W, H, 64)
    want = o.find_nearest(O, D)
    assert (want["objIdx"] >= 2).sum() > 300
    got = hits_np(crt, ctx.find_nearest_device(ray_records(crt, O, D), accel=GRID))
    torch.cuda.synchronize()
    assert_hits_equal(got, want, "find_nearest_device")
    # occlusion: 1024 rays, bounded at twice the nearest hit (misses: far away)
    sub = slice(0, 4096, 4)
    tt = np.where(want["objIdx"][sub] >= 0, want["t"][sub] * np.float32(2), np.float32(100)).astype(np.float32)
    occ = ctx.is_occluded_device(ray_records(crt, O[sub], D[sub], tt, crt.SHADOW_RAY_DTYPE), accel=GRID).cpu().numpy()
    want_occ = o.is_occluded(O[sub], D[sub], tt)
    assert np.array_equal(occ, want_occ) and 0 < want_occ.sum() < len(want_occ)
    # Sample
    seeds = (np.arange(1024, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)) | np.uint32(1)
    rgb, sout = ctx.sample_device(ray_records(crt, O[sub], D[sub]), seeds=torch.from_numpy(seeds.view(np.int32).copy()).to(dev()), accel=GRID)
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
    hs = crt.HostScene(xml, 0, ASSETS); hs.build_alt(GRID)
    ctx = crt.Context(32, 32); hs.upload(ctx); hs.upload_alt(ctx, GRID)
    o, _ = orc.load_scene(xml, 0, ASSETS); o.renderer_init(32, 32)
    O, D = pixel_rays(o, 32, 32, 64)
    rays = ray_records(crt, O, D); t = to_dev(bunny["moved"])
    s = torch.cuda.Stream(device=dev())
    old = ctx.find_nearest_device(rays, accel=GRID, stream=s)
    ctx.build_grid_device(0, t, stream=s)
    new = ctx.find_nearest_device(rays, accel=GRID, stream=s)
    torch.cuda.synchronize()
    a0 = orc.alt_accel("grid", o.bvh(0)["tris"]); orc.set_render_accel(o, a0)
    want_old = o.find_nearest(O, D)
    o.move_and_refit(0, bunny["moved"])
    a1 = orc.alt_accel("grid", o.bvh(0)["tris"]); orc.set_render_accel(o, a1)
    want_new = o.find_nearest(O, D)
    assert any((want_old[f] != want_new[f]).any() for f in ("t", "triIdx"))
    assert_hits_equal(hits_np(crt, old), want_old, "before the build: the old grid")
    assert_hits_equal(hits_np(crt, new), want_new, "after the build: the new grid")
    orc.set_render_accel(o, None); a0.close(); a1.close()


# 5. the KD-tree shares the triangle records: a rebuild marks it absent
def test_rebuild_marks_the_kdtree_absent(crt, bunny):
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS); hs.build_alt(crt.ACCEL_KDTREE)
    ctx = crt.Context(32, 32); hs.upload(ctx); hs.upload_alt(ctx, crt.ACCEL_KDTREE)
    ctx.set_render_accel(crt.ACCEL_KDTREE)
    one = (np.zeros((1, 3), np.float32), np.array([[0, 0, 1]], np.float32))
    ctx.find_nearest_alt(crt.ACCEL_KDTREE, *one)
    hs.build_grid_device(ctx, 0, to_dev(bunny["moved"]))                    # the host front's entry: the mirror follows
    with pytest.raises(crt.CrtError) as e:
        ctx.find_nearest_alt(crt.ACCEL_KDTREE, *one)
    assert e.value.code == -5
    assert ctx.L.crt_debug_render_accel(ctx.h) == 0
    G.assert_grids_equal(hs.grid(), bunny["grid_moved"], "host mirror")
    with pytest.raises(crt.CrtError) as e:                                  # the mirror's triangles are the host's old ones: it is not uploaded as it stands
        hs.upload_alt(ctx, GRID)
    assert e.value.code == -5
    G.assert_grids_equal(ctx.get_grid(), bunny["grid_moved"], "device")
    g0 = hs.build_alt(GRID); hs.upload_alt(ctx, GRID)                       # built from the host's triangles again: uploaded as ever
    G.assert_grids_equal(ctx.get_grid(), g0, "host build uploaded again")


# 6. a two-level scene: the set is dropped by a refit and live again after the rebuild
def test_two_level_set_follows_a_moved_blas(crt, orc):
    W = H = 32
    xml = scene_path("tlas_scene.xml")
    hs = crt.HostScene(xml, 1, ASSETS)
    uploaded = hs.build_alt(GRID)
    n = hs.bvh_count(); assert n == 3
    ctx = crt.Context(W, H); hs.upload(ctx); hs.upload_alt(ctx, GRID)
    o, _ = orc.load_scene(xml, 1, ASSETS); o.renderer_init(W, H)
    O, D = pixel_rays(o, W, H, 64); rays = ray_records(crt, O, D)
    p = [positions(hs.bvh(i)) for i in range(n)]
    moved = G.wobble(p[1]); t1 = to_dev(moved)
    T = to_dev(np.stack([hs.blas_transform(i)[0] for i in range(n)]))
    ctx.refit_device(1, t1)
    with pytest.raises(crt.CrtError) as e:                                  # dropped, as before this entry existed
        ctx.find_nearest_device(rays, accel=GRID)
    assert e.value.code == -5
    with pytest.raises(crt.CrtError) as e:
        ctx.get_grid(1)
    assert e.value.code == -5
    ctx.update_transforms_device(T)
    ctx.build_grid_device(1, t1)
    G.assert_grids_equal(ctx.get_grid(1), crt.host_grid_build(moved), "the rebuilt BLAS")
    for i in (0, 2):
        G.assert_grids_equal(ctx.get_grid(i), uploaded[i], "carried over %d" % i)
    o.move_and_refit(1, moved)
    accels = orc.blas_accels(o, "grid"); orc.set_blas_accel(o, accels)
    G.assert_grids_equal(ctx.get_grid(1), accels[1].dump(), "oracle's grid of the moved BLAS")
    want = o.find_nearest(O, D)
    assert len(set(want["objIdx"][want["objIdx"] >= 2])) >= 2
    got = hits_np(crt, ctx.find_nearest_device(rays, accel=GRID))
    assert_hits_equal(got, want, "find_nearest_device through the rebuilt set")
    ctx.set_render_accel(GRID)
    px = ctx.whitted_tick(); o.whitted(2)
    assert np.array_equal(px, o.screen()) and np.array_equal(ctx.accumulator(), o.accumulator())
    # CRT_UPDATE_BOUNDS (here: the host scene's original vertices again) clears every flag: the set is live only once all three have been rebuilt
    hs.update(ctx, crt.UPDATE_BOUNDS)
    for i in (2, 0):
        ctx.build_grid_device(i, to_dev(p[i]))
        with pytest.raises(crt.CrtError) as e:
            ctx.find_nearest_device(rays, accel=GRID)
        assert e.value.code == -5
    ctx.build_grid_device(1, to_dev(p[1]))
    for i in range(n):
        G.assert_grids_equal(ctx.get_grid(i), uploaded[i], "original positions, BLAS %d" % i)
    o2, _ = orc.load_scene(xml, 1, ASSETS); o2.renderer_init(W, H)
    a2 = orc.blas_accels(o2, "grid"); orc.set_blas_accel(o2, a2)
    assert_hits_equal(hits_np(crt, ctx.find_nearest_device(rays, accel=GRID)), o2.find_nearest(O, D), "all three rebuilt")
    # the host front's entry refreshes its mirror of the BLAS
    hs.build_grid_device(ctx, 1, t1)
    G.assert_grids_equal(hs.blas_alt(GRID, 1), crt.host_grid_build(moved), "host mirror")
    orc.set_blas_accel(o, None); orc.set_blas_accel(o2, None)
    for a in accels + a2:
        a.close()


# 6b. the three device writers chained on three streams, queries in flight on a fourth, a render behind them: no host synchronisation until the end
def test_refit_transforms_and_grid_chain_on_separate_streams(crt, orc):
    W = H = 32
    xml = scene_path("tlas_scene.xml")
    hs = crt.HostScene(xml, 1, ASSETS); hs.build_alt(GRID)
    n = hs.bvh_count(); assert n == 3
    ctx = crt.Context(W, H); hs.upload(ctx); hs.upload_alt(ctx, GRID)
    o, _ = orc.load_scene(xml, 1, ASSETS); o.renderer_init(W, H)
    O, D = pixel_rays(o, W, H, 64); rays = ray_records(crt, O, D)
    moved = G.wobble(positions(hs.bvh(1))); t1 = to_dev(moved)
    T = to_dev(np.stack([hs.blas_transform(i)[0] for i in range(n)]))
    s_q, s1, s2, s3 = (torch.cuda.Stream(device=dev()) for _ in range(4))
    old = ctx.find_nearest_device(rays, stream=s_q)
    ctx.refit_device(1, t1, stream=s1)
    ctx.update_transforms_device(T, stream=s2)
    ctx.build_grid_device(1, t1, stream=s3)
    new_bvh = ctx.find_nearest_device(rays, stream=s_q)
    new_grid = ctx.find_nearest_device(rays, accel=GRID, stream=s_q)
    px, acc, energy = ctx.tick(1)
    torch.cuda.synchronize()
    want_old = o.find_nearest(O, D)
    o.move_and_refit(1, moved)
    want_bvh = o.find_nearest(O, D)
    o.render(1, 4)
    accels = orc.blas_accels(o, "grid"); orc.set_blas_accel(o, accels)
    want_grid = o.find_nearest(O, D)
    orc.set_blas_accel(o, None)
    for a in accels:
        a.close()
    old, new_bvh = hits_np(crt, old), hits_np(crt, new_bvh)
    assert any((old[f] != new_bvh[f]).any() for f in ("t", "triIdx")), "the second query never saw the update"
    assert_hits_equal(old, want_old, "in flight before the chain: the unmoved scene")
    assert_hits_equal(new_bvh, want_bvh, "behind the chain: the refitted BVH under the rebuilt TLAS")
    assert_hits_equal(hits_np(crt, new_grid), want_grid, "behind the chain: the rebuilt grid set")
    assert np.array_equal(acc, o.accumulator()), "the Tick behind the chain: one frame of the moved scene"


# 7. refusals: the named status, and the previous grid keeps answering bit-identically
def test_refusals_leave_the_previous_grid(crt, bunny):
    C = crt.C
    ctx = crt.Context(32, 32)
    p0 = bunny["p0"]; good = to_dev(bunny["moved"])
    with pytest.raises(crt.CrtError) as e:                                  # no scene
        ctx.build_grid_device(0, good)
    assert e.value.code == -5
    hs = crt.HostScene(scene_path(BUNNY), 0, ASSETS); g = hs.build_alt(GRID)
    hs.upload(ctx); hs.upload_alt(ctx, GRID)
    rng = np.random.default_rng(5)
    lo, hi = p0.reshape(-1, 3).min(0), p0.reshape(-1, 3).max(0)
    O = (rng.uniform(lo - 1, hi + 1, (1500, 3))).astype(np.float32)
    D = rng.normal(size=(1500, 3)); D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(np.float32)
    before = ctx.find_nearest_alt(GRID, O, D)

    def unchanged(what):
        assert_hits_equal(ctx.find_nearest_alt(GRID, O, D), before, what)
        G.assert_grids_equal(ctx.get_grid(), g, what)

    bad = bunny["moved"].copy(); bad[len(bad) // 2, 1, 2] = np.nan
    inf = bunny["moved"].copy(); inf[-1, 2, 0] = np.inf
    host = np.array(bunny["moved"])                                          # (a writable copy)
    for what, call, code in (
            ("a NaN position", lambda: ctx.build_grid_device(0, to_dev(bad)), -1),
            ("an infinite position", lambda: ctx.build_grid_device(0, to_dev(inf)), -1),
            ("triCount off by one", lambda: ctx.build_grid_device(0, good[:-1].contiguous()), -1),
            ("a host pointer", lambda: ctx._ck(ctx.L.crt_build_grid_device(ctx.h, C.c_uint32(0), host.ctypes.data_as(C.c_void_p), C.c_uint32(len(host)), None)), -1),
            ("bvh out of range", lambda: ctx.build_grid_device(1, good), -1)):
        with pytest.raises(crt.CrtError) as e:
            call()
        assert e.value.code == code, what
        unchanged(what)
    with pytest.raises(ValueError):                                         # a CPU tensor does not get as far as the ABI
        ctx.build_grid_device(0, torch.from_numpy(host))
    # a two-level scene without an uploaded grid set
    ht = crt.HostScene(scene_path("tlas_scene.xml"), 1, ASSETS)
    ct = crt.Context(32, 32); ht.upload(ct)
    with pytest.raises(crt.CrtError) as e:
        ct.build_grid_device(0, to_dev(positions(ht.bvh(0))))
    assert e.value.code == -5
    # a PrimitiveScene has no triangles
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(0.0)
    pc = crt.Context(32, 32); ps.upload(pc)
    with pytest.raises(crt.CrtError) as e:
        pc.build_grid_device(0, good)
    assert e.value.code == -4
    # and after all that a good call still works
    ctx.build_grid_device(0, good)
    G.assert_grids_equal(ctx.get_grid(), bunny["grid_moved"], "a good call after the refusals")
