"""crt_sample / crt_sample_device: Renderer::Sample(ray, seed, 0) ("3. PathTracer/renderer.cpp":50-100) for arrays of rays with a seed each, on host buffers and
on device buffers enqueued on a caller's stream (device/sample_query.h).  Radiance, returned seed and the ray counter are compared with the CPU oracle's
orc_sample bit for bit, per world: FileScene through BVH / KD-tree / grid, TLASFileScene through TLAS-BVH / two-level KD-tree / two-level grid (the oracle walks
them through orc.set_blas_accel), PrimitiveScene.  The ray sets come from tests/sample_query_inputs.py; tests/test_sample_query_cpu.py asserts without a GPU that
they reach every branch of Sample.  The two-level worlds also take the committed rays on which the structures disagree (tests/alt_disagreement.py); those come
from assets/scenes/tlas_scene.xml and disagree there, so they are sampled in that scene too (test_sample_on_the_disagreement_rays)."""
import ctypes as C

import numpy as np
import pytest

import alt_disagreement as ad
import sample_query_inputs as si
from conftest import ASSETS, scene_path

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W, H = 64, 32                                                             # every context here: 4 x 2 tiles (the Tick test renders it)
INVALID, UNSUPPORTED, STATE = -1, -4, -5


def dev():
    return torch.device("cuda", 0)


def records(crt, O, D, inside=None):
    r = np.zeros(len(O), crt.RAY_DTYPE)
    r["O"], r["D"] = O, D
    if inside is not None:
        r["inside"] = inside
    return torch.from_numpy(r.view(np.float32).reshape(-1, 7).copy()).to(dev())


def seeds_t(s):
    return torch.from_numpy(np.ascontiguousarray(s, np.uint32).view(np.int32).copy()).to(dev())


def seeds_np(t):
    return t.cpu().numpy().view(np.uint32).copy()


def differing(a, b):
    """indices where two float32 arrays differ as bit patterns (any NaN equals any NaN)"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return np.flatnonzero(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).reshape(len(a), -1).any(axis=1))


def assert_same(rgb, seeds, want_rgb, want_seeds, what):
    bad = differing(rgb, want_rgb)
    assert len(bad) == 0, (what, "rgb", len(bad), bad[:8].tolist())
    bad = np.flatnonzero(np.asarray(seeds) != np.asarray(want_seeds))
    assert len(bad) == 0, (what, "seeds", len(bad), bad[:8].tolist())


class World:
    pass


class Worlds:
    """the scenes of this module, built once: name -> context, oracle, accelerator, ray set and the oracle's answer for it"""

    def __init__(self, crt, orc, tmp):
        self.crt, self.orc, self.xml, self.cache = crt, orc, si.scene_xml(tmp), {}

    def get(self, name):
        if name in self.cache:
            return self.cache[name]
        crt, orc = self.crt, self.orc
        w = World(); w.name = name; w.accel = {"kd": crt.ACCEL_KDTREE, "grid": crt.ACCEL_GRID, "tlas_kd": crt.ACCEL_KDTREE, "tlas_grid": crt.ACCEL_GRID}.get(name, 0)
        w.ctx = crt.Context(W, H)
        if name == "prim":
            w.hs = crt.HostPrimitiveScene(ASSETS); w.hs.set_time(1.3); w.hs.upload(w.ctx)
            w.o = orc.primitive_scene(ASSETS, 1.3)
            w.rays = si.prim_rays()
        else:
            kind = 1 if name.startswith("tlas") else 0
            w.hs = crt.HostScene(self.xml, kind, ASSETS)
            if w.accel:
                w.hs.build_alt(w.accel)
            w.hs.upload(w.ctx)
            if w.accel:
                w.hs.upload_alt(w.ctx, w.accel)
            w.o, _ = orc.load_scene(self.xml, kind, ASSETS)
            if name in ("kd", "grid"):
                w.acc = orc.alt_accel(name, w.o.bvh(0)["tris"]); orc.set_render_accel(w.o, w.acc)
            if name in ("tlas_kd", "tlas_grid"):
                orc.set_blas_accel(w.o, orc.blas_accels(w.o, name[5:]))
                w.rays = si.two_level_rays(w.o, name[5:])
            else:
                w.rays = si.triangle_rays(w.o)
        w.o.renderer_init(W, H)
        w.want = si.oracle_sample(w.o, *w.rays)
        self.cache[name] = w
        return w


@pytest.fixture(scope="module")
def worlds(crt, orc, tmp_path_factory):
    ws = Worlds(crt, orc, tmp_path_factory.mktemp("sample"))
    yield ws
    for w in ws.cache.values():
        w.ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 1 + 2. oracle parity in every world, on inputs that reach every branch
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", ["bvh", "kd", "grid", "tlas", "tlas_kd", "tlas_grid", "prim"])
def test_sample_equals_the_oracle(crt, worlds, world):
    w = worlds.get(world); ctx = w.ctx
    O, D, inside, seeds = w.rays
    want_rgb, want_seeds, cnt = w.want
    counted = ("rays", "mesh_hits", "primary")
    # host buffers
    ctx.sync(); c0 = ctx.counters()
    rgb, s = ctx.sample(O, D, seeds, inside, accel=w.accel)
    c1 = ctx.counters()
    assert_same(rgb, s, want_rgb, want_seeds, "crt_sample")
    assert {k: c1[k] - c0[k] for k in counted} == {k: cnt[k] for k in counted} and cnt["primary"] == 0
    # device buffers
    d_seeds = seeds_t(seeds)
    rgb_d, s_d = ctx.sample_device(rays=records(crt, O, D, inside), seeds=d_seeds, accel=w.accel)
    torch.cuda.synchronize()
    c2 = ctx.counters()
    assert rgb_d.shape == (len(O), 3) and rgb_d.dtype == torch.float32 and s_d.dtype == torch.int32
    assert_same(rgb_d.cpu().numpy(), seeds_np(s_d), want_rgb, want_seeds, "crt_sample_device")
    assert np.array_equal(seeds_np(d_seeds), seeds)                        # the caller's seeds are not modified
    assert {k: c2[k] - c1[k] for k in counted} == {k: cnt[k] for k in counted}
    # O / D / inside tensors instead of records
    rgb_e, s_e = ctx.sample_device(O=torch.from_numpy(O).to(dev()), D=torch.from_numpy(D).to(dev()), inside=torch.from_numpy(inside).to(dev()), seeds=d_seeds, accel=w.accel)
    torch.cuda.synchronize()
    assert_same(rgb_e.cpu().numpy(), seeds_np(s_e), want_rgb, want_seeds, "O / D form")
    # the inputs exercise the branches (the same assertion runs on the CPU: tests/test_sample_query_cpu.py)
    if world != "prim":
        si.assert_branches(w.o, O, D, inside, seeds, seeds_np(s_d))
    else:
        k = si.draws(seeds, seeds_np(s_d))
        assert (k == 0).sum() >= 100 and (k > 10).sum() >= 100


@pytest.mark.parametrize("kind", ["kd", "grid"])
def test_sample_on_the_disagreement_rays(crt, orc, kind):
    """tlas_scene.xml through the two-level structure, on the committed rays whose nearest hit there is not the TLAS-BVH's (primary rays, rays kEPS off a surface,
    rays inside the dielectric): radiance, returned seed and the counters equal orc_sample through the same structure.  The premise is asserted on the oracle's two
    answers: through the BVH most of these paths end elsewhere, so a Sample world that walked the TLAS-BVH instead would fail here."""
    xml = scene_path("tlas_scene.xml"); code = crt.ACCEL_KDTREE if kind == "kd" else crt.ACCEL_GRID
    b, a = ad.scene_pair(orc, xml, ASSETS, kind)
    O, D, inside, seeds, _ = ad.load(kind)
    want_rgb, want_seeds, cnt = si.oracle_sample(a, O, D, inside, seeds)
    bvh_rgb, bvh_seeds, _ = si.oracle_sample(b, O, D, inside, seeds)
    n_diff = len(set(differing(want_rgb, bvh_rgb)) | set(np.flatnonzero(want_seeds != bvh_seeds)))
    assert n_diff >= 50, n_diff                                            # of 180: 177 (KD-tree), 180 (grid)
    hs = crt.HostScene(xml, 1, ASSETS); hs.build_alt(code)
    ctx = crt.Context(W, H); hs.upload(ctx); hs.upload_alt(ctx, code)
    counted = ("rays", "mesh_hits", "primary")
    c0 = ctx.counters()
    rgb, s = ctx.sample(O, D, seeds, inside, accel=code)
    c1 = ctx.counters()
    assert_same(rgb, s, want_rgb, want_seeds, "crt_sample")
    assert {k: c1[k] - c0[k] for k in counted} == {k: cnt[k] for k in counted}
    rgb_d, s_d = ctx.sample_device(rays=records(crt, O, D, inside), seeds=seeds_t(seeds), accel=code)
    torch.cuda.synchronize()
    assert_same(rgb_d.cpu().numpy(), seeds_np(s_d), want_rgb, want_seeds, "crt_sample_device")
    c2 = ctx.counters()
    assert {k: c2[k] - c1[k] for k in counted} == {k: cnt[k] for k in counted}
    ctx.close(); hs.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 3. shapes: partial wavefronts, more rays than resident lanes, independence of position, two launches in flight
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def run_chunks(ctx, rays, seeds, chunk):
    """the rays in launches of `chunk` on the context's own stream, through the C entry on slices of one set of buffers"""
    n = rays.shape[0]
    s = seeds.clone(); rgb = torch.empty((n, 3), dtype=torch.float32, device=rays.device)
    torch.cuda.synchronize()
    for off in range(0, n, chunk):
        m = min(chunk, n - off)
        ctx._ck(ctx.L.crt_sample_device(ctx.h, 0, C.c_void_p(rays.data_ptr() + 28 * off), C.c_void_p(s.data_ptr() + 4 * off), C.c_void_p(rgb.data_ptr() + 12 * off), C.c_size_t(m), None))
    ctx.sync()
    return rgb.cpu().numpy(), seeds_np(s)


def test_shapes_and_independence_of_position(crt, worlds):
    w = worlds.get("bvh"); ctx = w.ctx
    O, D, inside, seeds = w.rays
    want_rgb, want_seeds, _ = w.want
    for n in (1, 63, 64, 65, 255, 257):
        r = records(crt, O[:n], D[:n], inside[:n])
        rgb, s = ctx.sample_device(rays=r, seeds=seeds_t(seeds[:n]))
        torch.cuda.synchronize()
        assert_same(rgb.cpu().numpy(), seeds_np(s), want_rgb[:n], want_seeds[:n], n)
        rgb_c, s_c = run_chunks(ctx, r, seeds_t(seeds[:n]), 64)
        assert_same(rgb_c, s_c, want_rgb[:n], want_seeds[:n], (n, "chunks"))
    # more rays than the launch has lanes: every wavefront draws from the cursor again
    resident = ctx.sample_resident_lanes(0)
    assert resident > 0 and resident % 256 == 0
    n = resident + 4099
    rng = np.random.default_rng(17)
    Ob, Db = si.camera_like(n, rng, [si.BUNNY_C, si.MIRROR_C, si.DIFFUSE_C, (0.0, -1.0, 0.8), (0.0, 3.0, 1.0), (0.0, 4.0, 6.0)])
    sb = si.seeds_for(n)
    r = records(crt, Ob, Db); st = seeds_t(sb)
    rgb, s = ctx.sample_device(rays=r, seeds=st)
    torch.cuda.synchronize()
    rgb, s = rgb.cpu().numpy(), seeds_np(s)
    sub = np.arange(2048) * (n // 2048)
    o_rgb, o_s, _ = si.oracle_sample(w.o, Ob[sub], Db[sub], np.zeros(len(sub), np.int32), sb[sub])
    assert_same(rgb[sub], s[sub], o_rgb, o_s, "strided subset against the oracle")
    assert np.isfinite(rgb).all() and si.draws(sb[:4096], s[:4096]).max() > 10
    # the same rays reversed, and in launches of 64: bit-identical per ray
    rr = torch.flip(r, [0]).contiguous(); sr = torch.flip(st, [0]).contiguous()
    # ... the two on two streams back to back: two launches in flight, each with a cursor slot of its own
    sA, sB = torch.cuda.Stream(device=dev()), torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    a_rgb, a_s = ctx.sample_device(rays=r, seeds=st, stream=sA)
    b_rgb, b_s = ctx.sample_device(rays=rr, seeds=sr, stream=sB)
    sA.synchronize(); sB.synchronize()
    assert_same(a_rgb.cpu().numpy(), seeds_np(a_s), rgb, s, "stream A")
    assert_same(b_rgb.cpu().numpy()[::-1], seeds_np(b_s)[::-1], rgb, s, "reversed, stream B")
    rgb_c, s_c = run_chunks(ctx, r, st, 64)
    assert_same(rgb_c, s_c, rgb, s, "launches of 64")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 4. Renderer::Tick rebuilt outside the library: needs the seed that comes back
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", ["bvh", "tlas", "tlas_kd", "tlas_grid", "prim"])
def test_tick_rebuilt_outside_the_library(crt, worlds, world):
    """ProcessTile (renderer.cpp:117-131) on the host: per 16 x 16 tile seed = InitSeed(tx + ty * W + spp * 1799); per pixel in order the y jitter, then the x jitter,
    the primary ray, Sample — Sample through sample_device with one ray per tile and the returned seed carried to the next pixel.  Two frames summed in frame order
    must be crt_render(1, 2)'s accumulator bit for bit.  crt_render is itself pinned to the oracle elsewhere (through the two-level KD-tree and grid:
    test_gpu_tlas_alt.py::test_render_through_the_structure_equals_the_oracle_through_it)."""
    w = worlds.get(world); ctx = w.ctx
    ctx.set_render_accel(w.accel)
    ctx.clear(); ctx.render(1, 2, 1)
    want = ctx.accumulator()
    ctx.set_render_accel(0)
    tx, ty = np.meshgrid(np.arange(W // 16, dtype=np.uint32), np.arange(H // 16, dtype=np.uint32))
    tx, ty = tx.reshape(-1), ty.reshape(-1)
    acc = np.zeros((H, W, 3), np.float32)
    for spp in (1, 2):
        seed = si.init_seed(tx + ty * np.uint32(W) + np.uint32(spp * 1799))
        for pix in range(256):
            seed, jy = si.rnd(seed)
            seed, jx = si.rnd(seed)
            x, y = tx * 16 + (pix & 15), ty * 16 + (pix >> 4)
            Op, Dp = w.o.primary_rays(np.stack([x.astype(np.float32) + jx, y.astype(np.float32) + jy], 1))
            rgb, s = ctx.sample_device(rays=records(crt, Op, Dp), seeds=seeds_t(seed), accel=w.accel)
            seed = seeds_np(s)                                              # (waits for the launch)
            acc[y, x] = acc[y, x] + rgb.cpu().numpy()
    bad = differing(acc.reshape(-1, 3), want[..., :3].reshape(-1, 3))
    assert len(bad) == 0, (len(bad), bad[:8].tolist())
    assert (want[..., 3] == 0).all() and acc.max() > 1.0


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 5. rays that are not traced
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_rays_that_are_not_traced(crt, worlds):
    w = worlds.get("bvh"); ctx = w.ctx
    n = 1024
    O, D, inside, seeds = [a[:n].copy() for a in w.rays]
    want_rgb, want_seeds = w.want[0][:n], w.want[1][:n]
    clean_rgb, clean_s = ctx.sample_device(rays=records(crt, O, D, inside), seeds=seeds_t(seeds))
    torch.cuda.synchronize()
    assert_same(clean_rgb.cpu().numpy(), seeds_np(clean_s), want_rgb, want_seeds, "clean batch")
    spots = [0, 31, 63, 64, 65, 127, 128, 300, 511, 512, 777, 1023]
    for k, i in enumerate(spots):
        if k % 4 == 0:
            seeds[i] = 0
        elif k % 4 == 1:
            D[i, k % 3] = np.nan
        elif k % 4 == 2:
            O[i, k % 3] = np.inf if k % 8 == 2 else -np.inf
        else:
            D[i] = (0.0, -0.0, 0.0)
    ok = np.ones(n, bool); ok[spots] = False
    for what in ("device", "host"):
        if what == "device":
            rgb, s = ctx.sample_device(rays=records(crt, O, D, inside), seeds=seeds_t(seeds))
            torch.cuda.synchronize()
            rgb, s = rgb.cpu().numpy(), seeds_np(s)
        else:
            rgb, s = ctx.sample(O, D, seeds, inside)
        bits = rgb.view(np.uint32)[spots]
        assert np.isnan(rgb[spots]).all() and ((bits & 0x00400000) != 0).all(), what          # quiet NaNs
        assert np.array_equal(s[spots], seeds[spots]), what                                  # the seed untouched
        assert_same(rgb[ok], s[ok], want_rgb[ok], want_seeds[ok], what)                      # nobody else is affected
    # a batch of nothing but refused rays ends too
    rgb, s = ctx.sample(O[spots], D[spots], seeds[spots], inside[spots])
    assert np.isnan(rgb).all() and np.array_equal(s, seeds[spots])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 6. ordering against scene updates
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_stream_ordering_against_scene_updates(crt, orc, worlds):
    w = worlds.get("tlas")
    hs = crt.HostScene(worlds.xml, 1, ASSETS); ctx = crt.Context(W, H); hs.upload(ctx)
    o, _ = orc.load_scene(worlds.xml, 1, ASSETS)
    m, reps = 1024, 128
    O, D, inside, seeds = [a[:m] for a in w.rays]
    before = (w.want[0][:m], w.want[1][:m])
    T = hs.blas_transform(1)[0].reshape(4, 4).copy()
    T[:3, 3] += np.array([0.4, 0.3, 1.5], np.float32)                       # the mirror cube moves back and up
    r = records(crt, O, D, inside).repeat(reps, 1).contiguous(); st = seeds_t(seeds).repeat(reps).contiguous()
    side = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    rgb1, s1 = ctx.sample_device(rays=r, seeds=st, stream=side)
    hs.set_transform(1, T); hs.update(ctx, crt.UPDATE_TRANSFORMS)          # no host sync in between
    rgb2, s2 = ctx.sample_device(rays=r, seeds=st, stream=side)
    side.synchronize()
    o.set_transform(1, T)
    after = si.oracle_sample(o, O, D, inside, seeds)
    for k in range(reps):
        sl = slice(k * m, (k + 1) * m)
        assert_same(rgb1[sl].cpu().numpy(), seeds_np(s1[sl]), before[0], before[1], ("before the update", k))
        assert_same(rgb2[sl].cpu().numpy(), seeds_np(s2[sl]), after[0], after[1], ("after the update", k))
    assert len(differing(before[0], after[0])) > 20                        # the move changes what these paths see
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def deep_chain_bvh(crt, T=60):
    """a BVH that is one long chain (height T - 1): uploads, but its traversal stack + 15 factor columns for four wavefronts exceed 64 KB of LDS"""
    tris = np.zeros(T, crt.TRI_DTYPE)
    for k in range(T):
        x = np.float32(-1.5 + 0.05 * k)
        tris["vertex0"][k] = (x, 0.0, 2.0); tris["vertex1"][k] = (x + np.float32(0.04), 0.0, 2.0); tris["vertex2"][k] = (x, 0.04, 2.0)
        tris["centroid"][k] = (tris["vertex0"][k] + tris["vertex1"][k] + tris["vertex2"][k]) / np.float32(3)
    for f in ("normal0", "normal1", "normal2"):
        tris[f] = (0.0, 0.0, -1.0)
    tris["objIdx"] = 2                                                     # FileScene numbers its objects from 2
    nodes = np.zeros(2 * T - 1, crt.NODE_DTYPE)
    lo = np.minimum(np.minimum(tris["vertex0"], tris["vertex1"]), tris["vertex2"]); hi = np.maximum(np.maximum(tris["vertex0"], tris["vertex1"]), tris["vertex2"])
    interior = 0
    for k in range(T - 1):                                                 # interior `interior` = leaf k + everything after it
        left = 2 * k + 1
        nodes[interior] = (lo[k:].min(0), hi[k:].max(0), left, 0)
        nodes[left] = (lo[k], hi[k], k, 1)
        if k == T - 2:
            nodes[left + 1] = (lo[k + 1], hi[k + 1], k + 1, 1)
        interior = left + 1
    return dict(nodes=nodes, tris=tris, triIndices=np.arange(T, dtype=np.uint32))


def test_refusals(crt, worlds):
    L = crt.lib()
    w = worlds.get("bvh"); ctx = w.ctx
    O, D, inside, seeds = [a[:256] for a in w.rays]
    want_rgb, want_seeds = w.want[0][:256], w.want[1][:256]
    d_rays = records(crt, O, D, inside); d_seeds = seeds_t(seeds); d_rgb = torch.full((256, 3), 7.0, dtype=torch.float32, device=dev())
    h_rays = d_rays.cpu().numpy().copy(); h_seeds = seeds.copy(); h_rgb = np.full((256, 3), 7.0, np.float32)
    torch.cuda.synchronize()
    p = lambda a: C.c_void_p(a.ctypes.data)                                 # noqa: E731
    d = lambda x, off=0: C.c_void_p(x.data_ptr() + off)                      # noqa: E731
    n = C.c_size_t(256)

    def refused(rc, code, ctxh=ctx):
        assert rc == code, (rc, code)
        assert len(L.crt_last_error(ctxh.h)) > 0

    # unknown accelerator / one that was not uploaded / too many rays
    refused(L.crt_sample_device(ctx.h, 7, d(d_rays), d(d_seeds), d(d_rgb), n, None), INVALID)
    refused(L.crt_sample(ctx.h, 7, p(h_rays), p(h_seeds), p(h_rgb), n), INVALID)
    refused(L.crt_sample_device(ctx.h, crt.ACCEL_KDTREE, d(d_rays), d(d_seeds), d(d_rgb), n, None), STATE)
    refused(L.crt_sample(ctx.h, crt.ACCEL_GRID, p(h_rays), p(h_seeds), p(h_rgb), n), STATE)
    refused(L.crt_sample_device(ctx.h, 0, d(d_rays), d(d_seeds), d(d_rgb), C.c_size_t(1 << 31), None), UNSUPPORTED)
    refused(L.crt_sample(ctx.h, 0, p(h_rays), p(h_seeds), p(h_rgb), C.c_size_t(1 << 31)), UNSUPPORTED)
    # buffers: NULL, misaligned, host memory — each of the three
    for bufs in ((None, d(d_seeds), d(d_rgb)), (d(d_rays), None, d(d_rgb)), (d(d_rays), d(d_seeds), None),
                 (d(d_rays, 2), d(d_seeds), d(d_rgb)), (d(d_rays), d(d_seeds, 1), d(d_rgb)), (d(d_rays), d(d_seeds), d(d_rgb, 2)),
                 (p(h_rays), d(d_seeds), d(d_rgb)), (d(d_rays), p(h_seeds), d(d_rgb)), (d(d_rays), d(d_seeds), p(h_rgb))):
        refused(L.crt_sample_device(ctx.h, 0, bufs[0], bufs[1], bufs[2], n, None), INVALID)
    refused(L.crt_sample(ctx.h, 0, None, p(h_seeds), p(h_rgb), n), INVALID)
    if torch.cuda.device_count() > 1:                                       # memory / a stream of another device
        other = torch.device("cuda", 1)
        refused(L.crt_sample_device(ctx.h, 0, d(d_rays.to(other)), d(d_seeds), d(d_rgb), n, None), INVALID)
        refused(L.crt_sample_device(ctx.h, 0, d(d_rays), d(d_seeds), d(d_rgb), n, C.c_void_p(torch.cuda.Stream(device=other).cuda_stream)), INVALID)
    # n == 0: a no-op after the checks that need no buffer
    assert L.crt_sample_device(ctx.h, 0, None, None, None, C.c_size_t(0), None) == 0 and L.crt_sample(ctx.h, 0, None, None, None, C.c_size_t(0)) == 0
    refused(L.crt_sample_device(ctx.h, 7, None, None, None, C.c_size_t(0), None), INVALID)
    # no scene at all; a scene whose traversal stack does not fit the kernel's LDS
    c2 = crt.Context(W, H)
    refused(L.crt_sample_device(c2.h, 0, d(d_rays), d(d_seeds), d(d_rgb), n, None), STATE, c2)
    refused(L.crt_sample(c2.h, 0, p(h_rays), p(h_seeds), p(h_rgb), n), STATE, c2)
    floor = np.full((512, 512), 0x808080, np.uint32); sky = np.full((4, 8), 0x6080c0, np.uint32)
    eye = np.eye(4, dtype=np.float32); Tl = eye.copy(); Tl[:3, 3] = (0, 3, 1); Ti = eye.copy(); Ti[:3, 3] = (0, -3, -1)
    c2.upload_desc(crt.SCENE_FILE, [deep_chain_bvh(crt)], [floor, sky], 0, 1, [(0.0, 0.0, (0.0, 0.0, 0.0), -1)], Tl, Ti, obj_mat_idx=[0])
    refused(L.crt_sample_device(c2.h, 0, d(d_rays), d(d_seeds), d(d_rgb), n, None), UNSUPPORTED, c2)
    refused(L.crt_sample(c2.h, 0, p(h_rays), p(h_seeds), p(h_rgb), n), UNSUPPORTED, c2)
    c2.close()
    # nothing was modified by any of them
    torch.cuda.synchronize()
    assert (d_rgb == 7.0).all().item() and np.array_equal(seeds_np(d_seeds), seeds) and (h_rgb == 7.0).all() and np.array_equal(h_seeds, seeds)
    # the binding's own checks
    for kw in (dict(rays=d_rays, seeds=d_seeds.to(torch.int64)), dict(rays=d_rays, seeds=d_seeds[:100]), dict(rays=d_rays, seeds=seeds), dict(rays=d_rays, seeds=d_seeds.cpu()),
               dict(rays=d_rays, seeds=d_seeds.repeat(2)[::2]), dict(rays=d_rays[:, :6], seeds=d_seeds), dict(rays=d_rays, O=d_rays[:, :3], D=d_rays[:, 3:6], seeds=d_seeds)):
        with pytest.raises(ValueError):
            ctx.sample_device(**kw)
    with pytest.raises(ValueError):
        ctx.sample(O, D, seeds[:100], inside)
    # and the context still answers
    rgb, s = ctx.sample_device(rays=d_rays, seeds=d_seeds)
    torch.cuda.synchronize()
    assert_same(rgb.cpu().numpy(), seeds_np(s), want_rgb, want_seeds, "after the refusals")
    rgb, s = ctx.sample(O, D, seeds, inside)
    assert_same(rgb, s, want_rgb, want_seeds, "host entry after the refusals")
