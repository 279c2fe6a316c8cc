"""crt_trace / crt_trace_device: the Whitted Renderer::Trace(ray, 0) ("2. WhittedStyle/renderer.cpp":21-91) for arrays of rays, on host buffers and on device
buffers enqueued on a caller's stream (device/trace_query.h over device/trace_body.h).

Yardsticks the kernel was not written from: for camera rays the oracle's orc_whitted_render (through the BVH / TLAS, FileScene's KD-tree and grid, and the two-level
KD-tree / grid sets by orc.set_blas_accel) and the library's own crt_whitted_tick[_inspect]; for rays no camera produces tests/trace_restate.py, which
tests/test_trace_restate_cpu.py pins to the oracle without a GPU.  Floats are compared as bit patterns (any NaN equals any NaN), counts and counters exactly.
The scenes and cameras are trace_restate's: assets/scenes/tlas_scene.xml (dielectric torii, half-mirror teapot) and three cubes (mirror, dielectric with
absorption, half mirror), 64 x 48."""
import ctypes as C

import numpy as np
import pytest

import query_schedules as qs
import trace_restate as R
from conftest import ASSETS
from test_gpu_sample_query import deep_chain_bvh, records

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W, H = R.W, R.H
SCENES = ASSETS + "/scenes"
INVALID, UNSUPPORTED, STATE = -1, -4, -5
SWITCH = "CRT_DEBUG_QUERY_GRID"
COUNTED = ("rays", "interior_iters", "leaf_iters", "tri_tests", "tlas_iters", "blas_visits", "mesh_hits")


def dev():
    return torch.device("cuda", 0)


def host_rays(crt, O, D, inside=None):
    r = np.zeros(len(O), crt.RAY_DTYPE)
    r["O"], r["D"] = O, D
    if inside is not None:
        r["inside"] = inside
    return r


def assert_same(got, want, what):
    bad = R.differing(got, want)
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist())


class World:
    pass


class Worlds:
    """name -> context (camera set), oracle (camera and accelerator set), restatement, the oracle's Whitted image.  Names: cubes / tlas, + _kd / _grid"""

    def __init__(self, crt, orc, tmp):
        self.crt, self.orc, self.tmp, self.cache = crt, orc, tmp, {}

    def get(self, name):
        if name in self.cache:
            return self.cache[name]
        crt, orc = self.crt, self.orc
        scene, _, alt = name.partition("_")
        w = World(); w.name, w.scene = name, scene
        w.accel = {"kd": crt.ACCEL_KDTREE, "grid": crt.ACCEL_GRID}.get(alt, 0)
        w.xml, w.kind = R.scene_of(scene, self.tmp, SCENES)
        w.hs = crt.HostScene(w.xml, w.kind, ASSETS)
        if w.accel:
            w.hs.build_alt(w.accel)
        w.ctx = crt.Context(W, H)
        w.hs.upload(w.ctx)
        if w.accel:
            w.hs.upload_alt(w.ctx, w.accel)                                   # a two-level scene's set goes through crt_upload_blas_accel
        w.ctx.set_camera_state(*R.CAMERAS[scene])
        w.o, w.sh, w.tr = R.load(orc, w.xml, w.kind, ASSETS, scene)
        if w.accel and w.kind == 0:
            w.acc = orc.alt_accel(alt, w.o.bvh(0)["tris"]); orc.set_render_accel(w.o, w.acc)
        elif w.accel:
            orc.set_blas_accel(w.o, orc.blas_accels(w.o, alt))
        w.O, w.D = R.pixel_rays(w.o, W, H)
        w.o.whitted()
        w.image = w.o.accumulator().reshape(-1, 4)[:, :3].copy()
        self.cache[name] = w
        return w


@pytest.fixture(scope="module")
def worlds(crt, orc, tmp_path_factory):
    ws = Worlds(crt, orc, tmp_path_factory.mktemp("trace"))
    yield ws
    for w in ws.cache.values():
        w.ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 1 + 2. camera rays: the oracle's Whitted image, the library's own Tick, its count images and its counters
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", ["cubes", "cubes_kd", "cubes_grid", "tlas", "tlas_kd", "tlas_grid"])
def test_camera_rays_equal_the_oracle_and_the_tick(crt, worlds, world):
    w = worlds.get(world); ctx = w.ctx
    d_rays = records(crt, w.O, w.D)
    ctx.sync(); ctx.reset_counters(); c0 = ctx.counters()
    rgb, trav, tested = ctx.trace_device(d_rays, accel=w.accel, counts=True)
    torch.cuda.synchronize()
    c1 = ctx.counters()
    assert rgb.shape == (W * H, 3) and rgb.dtype == torch.float32 and trav.dtype == torch.int32 and tested.shape == (W * H,)
    assert_same(rgb.cpu().numpy(), w.image, "against orc_whitted_render")
    # the library's Tick through the same accelerator
    ctx.set_render_accel(w.accel)
    px, metrics, t_img, s_img = ctx.whitted_tick_inspect(crt.INSPECT_NONE, counts=True)
    c2 = ctx.counters()
    acc = ctx.accumulator().reshape(-1, 4)
    ctx.whitted_tick()
    acc2 = ctx.accumulator().reshape(-1, 4)
    ctx.set_render_accel(0)
    assert_same(rgb.cpu().numpy(), acc[:, :3], "against crt_whitted_tick_inspect")
    assert_same(rgb.cpu().numpy(), acc2[:, :3], "against crt_whitted_tick")
    assert np.array_equal(trav.cpu().numpy(), t_img.reshape(-1)) and np.array_equal(tested.cpu().numpy(), s_img.reshape(-1))
    assert int(trav.max()) > 0 and int(tested.max()) > 0
    d_trace = {k: c1[k] - c0[k] for k in COUNTED + ("primary",)}; d_tick = {k: c2[k] - c1[k] for k in COUNTED + ("primary",)}
    assert d_trace["primary"] == 0 and d_tick["primary"] == W * H
    assert {k: d_trace[k] for k in COUNTED} == {k: d_tick[k] for k in COUNTED} and d_trace["rays"] > W * H
    # without the counts, and through the host entry
    assert_same(ctx.trace_device(d_rays, accel=w.accel).cpu().numpy(), w.image, "no counts")
    h_rgb, h_trav, h_tested = ctx.trace(host_rays(crt, w.O, w.D), accel=w.accel, counts=True)
    assert_same(h_rgb, w.image, "host entry")
    assert np.array_equal(h_trav, t_img.reshape(-1)) and np.array_equal(h_tested, s_img.reshape(-1))


def test_depth_limit_1(crt, orc, worlds):
    w = worlds.get("cubes")
    ctx = crt.Context(W, H, depth_limit=1); w.hs.upload(ctx); ctx.set_camera_state(*R.CAMERAS["cubes"])
    o, _, _ = R.load(orc, w.xml, w.kind, ASSETS, "cubes", 1)
    o.whitted()
    want = o.accumulator().reshape(-1, 4)[:, :3]
    assert len(R.differing(want, w.image)) > 20                              # the limit matters in this image
    assert_same(ctx.trace_device(records(crt, w.O, w.D)).cpu().numpy(), want, "depthLimit 1")
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 3. rays no camera produces, against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def odd_rays(w, seed=5):
    """(O, D, inside): rays starting inside the dielectric with inside = 1, origins on surfaces (the camera rays' hit points), rays from below the floor, and
    camera rays with unnormalised directions"""
    rng = np.random.default_rng(seed)
    unit = qs.unit
    hits = w.o.find_nearest(w.O, w.D)
    # inside the dielectric: from points just behind the surface the camera sees, along the refracted-ish direction and random rising ones
    glass = np.flatnonzero((w.tr.refr[np.maximum(w.sh.hit_info(w.O, w.D, hits)["material"], 0)] > 0) & (hits["objIdx"] >= 2))
    assert len(glass) >= 5
    g = glass[rng.integers(0, len(glass), 256)]
    O1 = (w.O[g] + (hits["t"][g] + np.float32(0.02))[:, None] * w.D[g]).astype(np.float32)
    D1 = unit(w.D[g] + rng.normal(scale=0.4, size=(256, 3)))
    # on surfaces: the hit points of floor and mesh pixels, random directions
    on = np.flatnonzero(hits["objIdx"] >= 1)
    s = on[rng.integers(0, len(on), 512)]
    O2 = (w.O[s] + hits["t"][s][:, None] * w.D[s]).astype(np.float32)
    D2 = unit(rng.normal(size=(512, 3)))
    # from below the floor (the plane y = -1), up and down
    O3 = np.stack([rng.uniform(-2, 2, 256), rng.uniform(-3.0, -1.05, 256), rng.uniform(0, 5, 256)], 1).astype(np.float32)
    D3 = unit(rng.normal(size=(256, 3)))
    # unnormalised directions
    p = rng.integers(0, len(w.O), 512)
    O4 = w.O[p]; D4 = (w.D[p] * rng.uniform(0.25, 7.0, (512, 1))).astype(np.float32)
    O = np.concatenate([O1, O2, O3, O4]); D = np.concatenate([D1, D2, D3, D4])
    inside = np.zeros(len(O), np.int32); inside[:256] = 1
    return O, D, inside


@pytest.mark.parametrize("world", ["cubes", "tlas"])
def test_rays_no_camera_produces_equal_the_restatement(crt, worlds, world):
    w = worlds.get(world); ctx = w.ctx
    O, D, inside = odd_rays(w)
    counts = {}
    want = w.tr.trace(O, D, inside, counts=counts)
    assert np.isfinite(want).all() and counts["cost"].max() > 6 and len(R.differing(want[:256], w.tr.trace(O[:256], D[:256]))) > 64     # inside = 1 matters
    rgb, trav, tested = ctx.trace_device(records(crt, O, D, inside), counts=True)
    torch.cuda.synchronize()
    assert_same(rgb.cpu().numpy(), want, "trace_device")
    assert np.array_equal(trav.cpu().numpy(), counts["traversed"]) and np.array_equal(tested.cpu().numpy(), counts["tested"])
    assert_same(ctx.trace(host_rays(crt, O, D, inside)), want, "trace")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 4. lane reuse: one-trip sky rays among deep dielectric trees, bounded grids, more rays than resident lanes
# ---------------------------------------------------------------------------------------------------------------------------------------------------
N_ORD, N_WALK = 4096, 4096                                                   # ordinary rays of the pool; rays of the walker-among-idlers order (64 groups of 64)


@pytest.fixture(scope="module")
def reuse(crt, worlds):
    """the pool (<= 8192 rays), the restatement's answer for every ray of it, and the orders"""
    w = worlds.get("cubes")
    rng = np.random.default_rng(9)
    lo, hi = qs.scene_box(w.o, 0)
    # ordinary: rays from around the scene through the glass cube (deep trees: both children at every level) and the camera's rays
    c = np.float32(R.GLASS_C)
    n1 = N_ORD - W * H
    d = rng.normal(size=(n1, 3)); d[:, 1] = np.abs(d[:, 1]) * 0.5; d /= np.linalg.norm(d, axis=1, keepdims=True)
    O1 = (c + d * rng.uniform(1.5, 3.0, (n1, 1))).astype(np.float32)
    D1 = qs.unit(c + rng.uniform(-0.45, 0.45, (n1, 3)) - O1)
    O = np.concatenate([O1, w.O]); D = np.concatenate([D1, w.D])
    Oi, Di = qs.idler_rays(lo, hi, (N_WALK // qs.WAVE) * (qs.WAVE - 1), 13, up=True)
    pool = qs.Pool([("ordinary", O, D, np.zeros(len(O), np.int32)), ("idlers", Oi, Di, np.zeros(len(Oi), np.int32))], 3, sample=True)
    assert len(pool.O) <= 8192
    counts = {}
    want = w.tr.trace(pool.O, pool.D, counts=counts)
    cost = counts["cost"]
    assert (cost[pool.idlers] == 1).all() and (cost[pool.ordinary] >= 10).sum() >= N_WALK // qs.WAVE     # one-trip sky rays; a tree of 10+ traversals for every group
    everything = np.arange(len(pool.O))
    orders = {"shuffled": qs.shuffled(everything), "ascending": qs.ascending(everything, cost), "descending": qs.descending(everything, cost),
              "walker_among_idlers": qs.walker_among_idlers(pool.ordinary, cost, pool.idlers, N_WALK)}
    return w, pool, want, counts, orders


@pytest.mark.parametrize("k", [1, 3, 0])
def test_lane_reuse_in_the_schedules_orders(crt, reuse, monkeypatch, k):
    w, pool, want, counts, orders = reuse
    ctx = w.ctx
    monkeypatch.setenv(SWITCH, str(k))                                       # read by every launch; 0: no bound
    subset = np.arange(0, len(pool.O), 7)                                    # the rays held to the restatement; every ray is held to agreement across the runs
    first = None
    for name, order in orders.items():
        rgb, trav, tested = ctx.trace_device(records(crt, pool.O[order], pool.D[order]), counts=True)
        torch.cuda.synchronize()
        got = np.full((len(pool.O), 3), np.nan, np.float32); got[order] = rgb.cpu().numpy()
        seen = np.zeros(len(pool.O), bool); seen[order] = True
        sub = subset[seen[subset]]
        assert_same(got[sub], want[sub], (k, name, "against the restatement"))
        gt = np.zeros(len(pool.O), np.int32); gt[order] = trav.cpu().numpy()
        assert np.array_equal(gt[sub], counts["traversed"][sub]), (k, name)
        if first is None:
            first = got                                                     # "shuffled" holds every ray of the pool
        assert_same(got[seen], first[seen], (k, name, "agreement with the first order"))


def test_more_rays_than_resident_lanes(crt, reuse):
    w, pool, want, counts, orders = reuse
    ctx = w.ctx
    resident = ctx.trace_resident_lanes(0)
    assert resident > 0 and resident % 256 == 0
    n = resident + 77
    order = orders["shuffled"]
    reps = (n + len(order) - 1) // len(order)
    d_rays = records(crt, pool.O[order], pool.D[order]).repeat(reps, 1)[:n].contiguous()
    rgb, trav, _ = ctx.trace_device(d_rays, counts=True)
    torch.cuda.synchronize()
    rgb, trav = rgb.cpu().numpy(), trav.cpu().numpy()
    idx = np.tile(order, reps)[:n]
    assert_same(rgb, want[idx], "n just above the resident lanes")
    assert np.array_equal(trav, counts["traversed"][idx])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 5. rays that are not traced
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_rays_that_are_not_traced(crt, worlds):
    w = worlds.get("cubes"); ctx = w.ctx
    n = 1024
    O, D = w.O[1000:1000 + n].copy(), w.D[1000:1000 + n].copy()
    clean, ct, cs = ctx.trace_device(records(crt, O, D), counts=True)
    torch.cuda.synchronize()
    clean, ct, cs = clean.cpu().numpy(), ct.cpu().numpy(), cs.cpu().numpy()
    assert_same(clean, w.image[1000:1000 + n], "clean batch")
    spots = [0, 31, 63, 64, 65, 127, 128, 255, 256, 300, 511, 512, 777, 1023]
    for k, i in enumerate(spots):
        if k % 4 == 0:
            D[i, k % 3] = np.nan
        elif k % 4 == 1:
            O[i, k % 3] = np.inf if k % 8 == 1 else -np.inf
        elif k % 4 == 2:
            D[i] = (0.0, -0.0, 0.0)
        else:
            D[i, k % 3] = -np.inf
    ok = np.ones(n, bool); ok[spots] = False
    for what in ("device", "host"):
        if what == "device":
            rgb, trav, tested = [t.cpu().numpy() for t in ctx.trace_device(records(crt, O, D), counts=True)]
        else:
            rgb, trav, tested = ctx.trace(host_rays(crt, O, D), counts=True)
        b = rgb.view(np.uint32)[spots]
        assert np.isnan(rgb[spots]).all() and ((b & 0x00400000) != 0).all(), what               # quiet NaNs
        assert (trav[spots] == -1).all() and (tested[spots] == -1).all(), what
        assert_same(rgb[ok], clean[ok], what)                                                    # nobody else is affected
        assert np.array_equal(trav[ok], ct[ok]) and np.array_equal(tested[ok], cs[ok]), what
    # without count outputs, and a batch of nothing but refused rays ends too
    assert np.isnan(ctx.trace_device(records(crt, O, D)).cpu().numpy()[spots]).all()
    rgb, trav, tested = ctx.trace(host_rays(crt, O[spots], D[spots]), counts=True)
    assert np.isnan(rgb).all() and (trav == -1).all() and (tested == -1).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 6. host entry == device entry; a launch on a non-default stream fed by a tensor op on that stream
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_host_entry_equals_device_entry_and_stream_order(crt, worlds):
    w = worlds.get("tlas"); ctx = w.ctx
    base = records(crt, w.O, w.D)
    scale = torch.tensor([1, 1, 1, 3, 3, 3, 1], dtype=torch.float32, device=dev())          # D times 3: not normalised (the inside column is 0)
    side = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        big = base.repeat(64, 1)
        for _ in range(20):                                                  # work ahead of the rays on the same stream
            big = big * 1.0
        d_rays = (big[: W * H] * scale).contiguous()
        rgb, trav, tested = ctx.trace_device(d_rays, counts=True, stream=side)   # no synchronisation in between
    side.synchronize()
    h_rgb, h_trav, h_tested = ctx.trace(host_rays(crt, w.O, (w.D * np.float32(3)).astype(np.float32)), counts=True)
    assert_same(rgb.cpu().numpy(), h_rgb, "device on a side stream against host")
    assert np.array_equal(trav.cpu().numpy(), h_trav) and np.array_equal(tested.cpu().numpy(), h_tested)
    assert_same(h_rgb, w.tr.trace(w.O, (w.D * np.float32(3)).astype(np.float32)), "against the restatement")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 7. ordering against scene updates
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_ordering_against_update_scene(crt, orc, worlds):
    w = worlds.get("tlas")
    hs = crt.HostScene(w.xml, 1, ASSETS); ctx = crt.Context(W, H); hs.upload(ctx)
    o, sh, tr = R.load(orc, w.xml, 1, ASSETS, "tlas")
    m, reps = W * H, 16
    O, D = w.O, w.D
    before = w.image
    T = hs.blas_transform(0)[0].reshape(4, 4).copy()
    T[:3, 3] += np.array([0.5, 0.4, -0.5], np.float32)                      # the wok moves: its pixels, its shadow, its image in the teapot and the torii
    r = records(crt, O, D).repeat(reps, 1).contiguous()
    side = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    rgb1 = ctx.trace_device(r, stream=side)
    hs.set_transform(0, T); hs.update(ctx, crt.UPDATE_TRANSFORMS)          # no host sync in between
    rgb2 = ctx.trace_device(r, stream=side)
    side.synchronize()
    o.set_transform(0, T); sh.refresh_transforms(o)
    after = tr.trace(O, D)
    assert len(R.differing(before, after)) > 100                             # the move changes what these rays see
    rgb1, rgb2 = rgb1.cpu().numpy(), rgb2.cpu().numpy()
    for k in range(reps):
        assert_same(rgb1[k * m:(k + 1) * m], before, ("before the update", k))
        assert_same(rgb2[k * m:(k + 1) * m], after, ("after the update", k))
    ctx.close(); hs.close()


def test_ordering_against_refit_device(crt, orc, worlds):
    w = worlds.get("cubes")
    hs = crt.HostScene(w.xml, 0, ASSETS); ctx = crt.Context(W, H); hs.upload(ctx)
    o, sh, tr = R.load(orc, w.xml, 0, ASSETS, "cubes")
    m, reps = 1024, 64
    sel = np.arange(m) * (W * H // m)
    O, D = w.O[sel], w.D[sel]
    before = w.image[sel]
    t = hs.bvh(0)["tris"]
    moved = np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1).astype(np.float32)
    moved[:, :, 1] += np.float32(0.35)                                       # every cube rises off the floor
    d_moved = torch.from_numpy(moved).to(dev())
    r = records(crt, O, D).repeat(reps, 1).contiguous()
    side = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    rgb1 = ctx.trace_device(r, stream=side)
    hs.refit_device(ctx, 0, d_moved, stream=side)
    rgb2 = ctx.trace_device(r, stream=side)
    side.synchronize()
    o.move_and_refit(0, moved)
    after = tr.trace(O, D)
    assert len(R.differing(before, after)) > 10
    rgb1, rgb2 = rgb1.cpu().numpy(), rgb2.cpu().numpy()
    for k in range(reps):
        assert_same(rgb1[k * m:(k + 1) * m], before, ("before the refit", k))
        assert_same(rgb2[k * m:(k + 1) * m], after, ("after the refit", k))
    ctx.close(); hs.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(crt, worlds):
    L = crt.lib()
    w = worlds.get("cubes"); ctx = w.ctx
    n_ = 256
    O, D = w.O[:n_], w.D[:n_]
    d_rays = records(crt, O, D); d_rgb = torch.full((n_, 3), 7.0, dtype=torch.float32, device=dev())
    d_t = torch.full((n_,), 7, dtype=torch.int32, device=dev()); d_s = d_t.clone()
    h_rays = host_rays(crt, O, D); h_rgb = np.full((n_, 3), 7.0, np.float32); h_t = np.full(n_, 7, np.int32); h_s = h_t.copy()
    torch.cuda.synchronize()
    p = lambda a: C.c_void_p(a.ctypes.data)                                 # noqa: E731
    d = lambda x, off=0: C.c_void_p(x.data_ptr() + off)                      # noqa: E731
    n = C.c_size_t(n_)

    def refused(rc, code, ctxh=ctx):
        assert rc == code, (rc, code)
        assert len(L.crt_last_error(ctxh.h)) > 0

    def device(c, accel, rays, rgb, t, s, count=n):
        return L.crt_trace_device(c.h, accel, rays, rgb, t, s, count, None)

    def host(c, accel, rays, rgb, t, s, count=n):
        return L.crt_trace(c.h, accel, rays, rgb, t, s, count)

    # unknown accelerator / one that was not uploaded / too many rays
    refused(device(ctx, 7, d(d_rays), d(d_rgb), d(d_t), d(d_s)), INVALID)
    refused(host(ctx, 7, p(h_rays), p(h_rgb), p(h_t), p(h_s)), INVALID)
    refused(device(ctx, crt.ACCEL_KDTREE, d(d_rays), d(d_rgb), d(d_t), d(d_s)), STATE)
    refused(host(ctx, crt.ACCEL_GRID, p(h_rays), p(h_rgb), p(h_t), p(h_s)), STATE)
    refused(device(ctx, 0, d(d_rays), d(d_rgb), d(d_t), d(d_s), C.c_size_t(1 << 31)), UNSUPPORTED)
    refused(host(ctx, 0, p(h_rays), p(h_rgb), p(h_t), p(h_s), C.c_size_t(1 << 31)), UNSUPPORTED)
    # buffers: NULL (rays, rgb), misaligned, host memory — each of the four
    for bufs in ((None, d(d_rgb), d(d_t), d(d_s)), (d(d_rays), None, d(d_t), d(d_s)),
                 (d(d_rays, 2), d(d_rgb), d(d_t), d(d_s)), (d(d_rays), d(d_rgb, 2), d(d_t), d(d_s)), (d(d_rays), d(d_rgb), d(d_t, 1), d(d_s)), (d(d_rays), d(d_rgb), d(d_t), d(d_s, 2)),
                 (p(h_rays), d(d_rgb), d(d_t), d(d_s)), (d(d_rays), p(h_rgb), d(d_t), d(d_s)), (d(d_rays), d(d_rgb), p(h_t), d(d_s)), (d(d_rays), d(d_rgb), d(d_t), p(h_s))):
        refused(device(ctx, 0, *bufs), INVALID)
    refused(host(ctx, 0, None, p(h_rgb), p(h_t), p(h_s)), INVALID)
    refused(host(ctx, 0, p(h_rays), None, p(h_t), p(h_s)), INVALID)
    if torch.cuda.device_count() > 1:                                       # memory / a stream of another device
        other = torch.device("cuda", 1)
        refused(device(ctx, 0, d(d_rays.to(other)), d(d_rgb), d(d_t), d(d_s)), INVALID)
        refused(L.crt_trace_device(ctx.h, 0, d(d_rays), d(d_rgb), d(d_t), d(d_s), n, C.c_void_p(torch.cuda.Stream(device=other).cuda_stream)), INVALID)
    # n == 0: a no-op after the checks that need no buffer
    assert device(ctx, 0, None, None, None, None, C.c_size_t(0)) == 0 and host(ctx, 0, None, None, None, None, C.c_size_t(0)) == 0
    refused(device(ctx, 7, None, None, None, None, C.c_size_t(0)), INVALID)
    # no scene at all; the PrimitiveScene; a scene whose traversal stack does not fit the kernel's LDS
    c2 = crt.Context(W, H)
    refused(device(c2, 0, d(d_rays), d(d_rgb), d(d_t), d(d_s)), STATE, c2)
    refused(host(c2, 0, p(h_rays), p(h_rgb), p(h_t), p(h_s)), STATE, c2)
    refused(device(c2, crt.ACCEL_GRID, d(d_rays), d(d_rgb), d(d_t), d(d_s)), STATE, c2)
    prim = crt.HostPrimitiveScene(ASSETS); prim.upload(c2)
    refused(device(c2, 0, d(d_rays), d(d_rgb), d(d_t), d(d_s)), UNSUPPORTED, c2)
    refused(host(c2, 0, p(h_rays), p(h_rgb), p(h_t), p(h_s)), UNSUPPORTED, c2)
    c2.close(); prim.close()
    c3 = crt.Context(W, H)
    floor = np.full((512, 512), 0x808080, np.uint32); sky = np.full((4, 8), 0x6080c0, np.uint32)
    eye = np.eye(4, dtype=np.float32); Tl = eye.copy(); Tl[:3, 3] = (0, 3, 1); Ti = eye.copy(); Ti[:3, 3] = (0, -3, -1)
    c3.upload_desc(crt.SCENE_FILE, [deep_chain_bvh(crt, 90)], [floor, sky], 0, 1, [(0.0, 0.0, (0.0, 0.0, 0.0), -1)], Tl, Ti, obj_mat_idx=[0])
    refused(device(c3, 0, d(d_rays), d(d_rgb), d(d_t), d(d_s)), UNSUPPORTED, c3)
    refused(host(c3, 0, p(h_rays), p(h_rgb), p(h_t), p(h_s)), UNSUPPORTED, c3)
    with pytest.raises(crt.CrtError):
        c3.trace_resident_lanes(0)
    c3.close()
    # nothing was modified by any of them
    torch.cuda.synchronize()
    assert (d_rgb == 7.0).all().item() and (d_t == 7).all().item() and (d_s == 7).all().item()
    assert (h_rgb == 7.0).all() and (h_t == 7).all() and (h_s == 7).all()
    # the binding's own checks
    with pytest.raises(ValueError):
        ctx.trace_device(d_rays[:, :6])
    with pytest.raises(ValueError):
        ctx.trace_device(d_rays.cpu())
    with pytest.raises(ValueError):
        ctx.trace(np.zeros((4, 7), np.float32))
    # and the context still answers
    assert_same(ctx.trace_device(d_rays).cpu().numpy(), w.image[:n_], "after the refusals")
    assert_same(ctx.trace(h_rays), w.image[:n_], "host entry after the refusals")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 9. crt_tick's rendered-ahead frames survive a trace_device in between
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_tick_ahead_survives_a_trace(crt, worlds):
    w = worlds.get("cubes")
    a, b = crt.Context(W, H), crt.Context(W, H)                              # a: a trace between the Ticks; b: the Ticks alone
    w.hs.upload(a); w.hs.upload(b)
    d_rays = records(crt, w.O, w.D)
    for ctx in (a, b):
        ctx.tick(1); ctx.tick(2)                                            # the second still Tick renders frames ahead
        ctx.timing()                                                        # (the figures cover the launches since the previous call)
    rgb = a.trace_device(d_rays)
    got = [a.tick(3), a.tick(4)]; want = [b.tick(3), b.tick(4)]
    torch.cuda.synchronize()
    for g, x in zip(got, want):
        assert np.array_equal(g[0], x[0]) and np.array_equal(g[1], x[1]) and g[2] == x[2]
    la, lb = a.timing()["render_launches"], b.timing()["render_launches"]
    assert la == lb and la < 2, (la, lb)                                     # Ticks 3 and 4 came out of the slab rendered ahead, in both contexts
    # the trace's rays are the caller's (the cubes camera's), whatever camera the context has (here the default one)
    assert_same(rgb.cpu().numpy(), w.image, "the trace between the Ticks")
    a.close(); b.close()
