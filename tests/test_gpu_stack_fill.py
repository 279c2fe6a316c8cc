"""Every kernel that owns a traversal stack, with rays that fill the stack to the last entry the library allots (tests/stack_fill.py; the criterion is settled
on the CPU oracle by tests/test_stack_fill_cpu.py).  An off-by-one in a height, in the marker's slot or in the address of what lies behind the stack shows only
on such a ray: it overwrites a neighbour's state or lands outside the allocation, and the later pop returns something else.  Every comparison is exact: hit
records with their traversed / tested counts against the oracle's, accumulators and ray counts against the oracle's render.  Each test first asserts that what
the library allots (stack_fill.allotted) is what the CPU module established for its rays, so a change of the sizing cannot make it vacuous.

The filling rays are mixed one to one with rays that end at the root, and the query launches are also bounded to one workgroup (CRT_DEBUG_QUERY_GRID=1), so that
lanes take their next ray beside a lane that holds a full stack."""
import ctypes as C

import numpy as np
import pytest

import stack_fill as S
from conftest import ASSETS
from render_views_inputs import oracle_view

torch = pytest.importorskip("torch")

import test_gpu_grid_device as TG                                          # noqa: E402  (helpers only; a module object is not collected)
from test_gpu_bvh_device import assert_same_scene, described               # noqa: E402

pytestmark = pytest.mark.gpu

SWITCH = "CRT_DEBUG_QUERY_GRID"
KD = 1
N_MIX = 512
ACCELS = ("bvh", "kd")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_hits(got, want, what):
    for f in S.FIELDS:
        a, b = bits(got[f]), bits(want[f])
        assert np.array_equal(a, b), (what, f, int((a != b).sum()), np.flatnonzero(a != b)[:8].tolist())


def same_floats(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


class Truth:
    """a world on the CPU: the oracle's scene, the restated walks, the kept filling rays mixed with short ones, and the oracle's answers through both structures.
    Made once per world and never changed."""

    def __init__(self, orc, name, tmp):
        self.name, self.kind, self.tmp = name, S.KIND[name], tmp
        self.o = S.load_oracle(orc, name, tmp)
        self.walk = {a: S.World(orc, self.o, a) for a in ACCELS}
        O, D = S.fill_rays(name)
        k = S.kept(self.walk["bvh"], O, D, orc.HIT_DTYPE, self.walk["bvh"].entries())
        assert k["keep"].sum() >= S.MIN_FILLING and (k["fill"] & ~k["keep"]).sum() <= k["fill"].sum() // 4
        self.attained = {"bvh": int(k["held"].max())}
        fill = {"bvh": (O[k["keep"]], D[k["keep"]]), "kd": S.kd_rays(name)}
        _, occ = self.walk["kd"].find_nearest_many(*fill["kd"], orc.HIT_DTYPE)
        self.attained["kd"] = max(x.kd_held for x in occ)
        self.kd_tlas = max(x.tlas_held for x in occ)
        Os, Ds = S.short_rays(N_MIX // 2)
        self.rays, self.want, self.shadow_t, self.occluded, self.is_fill = {}, {}, {}, {}, {}
        for a in ACCELS:
            Of, Df = fill[a]
            pick = np.arange(N_MIX // 2) % len(Of)
            O2 = np.empty((N_MIX, 3), np.float32); D2 = np.empty((N_MIX, 3), np.float32)
            O2[0::2], D2[0::2], O2[1::2], D2[1::2] = Of[pick], Df[pick], Os, Ds
            t = np.where(np.arange(N_MIX) % 4 < 2, np.float32(1e30), np.float32(0.5)).astype(np.float32)
            S.through(orc, self.o, a)
            self.rays[a] = (O2, D2); self.want[a] = self.o.find_nearest(O2, D2); self.shadow_t[a] = t; self.occluded[a] = self.o.is_occluded(O2, D2, t)
            self.is_fill[a] = np.arange(N_MIX) % 2 == 0
            for x in (O2, D2, t):
                x.setflags(write=False)
        S.through(orc, self.o, "bvh")
        self._camera = {}

    def camera(self, orc, accel):
        """the camera on the x axis: the oracle's records of the pixels' primary rays through `accel`, its Whitted image, and the BVH walk's entries held"""
        if accel not in self._camera:
            cam = S.CAMERA; o = self.o
            o.renderer_init(cam["W"], cam["H"]); o.set_camera_state(cam["pos"], cam["target"])
            O, D = S.camera_pixels(o, cam["W"], cam["H"])
            S.through(orc, o, accel)
            h = o.find_nearest(O, D)
            o.whitted(4)
            e = dict(O=O, D=D, hits=h, acc=o.accumulator(), screen=o.screen())
            S.through(orc, o, "bvh")
            if accel == "bvh":
                _, occ = self.walk["bvh"].find_nearest_many(O, D, orc.HIT_DTYPE)
                e["held"] = np.array([x.held for x in occ])
            self._camera[accel] = e
        return self._camera[accel]


@pytest.fixture(scope="module")
def truths(orc, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stack_fill_gpu")
    made = {}

    def get(name):
        if name not in made:
            made[name] = Truth(orc, name, tmp)
        return made[name]
    return get


def chain_tris(crt):
    return TG.tri_records(crt, S.mesh("chain"))


def upload_chain_kd(crt, ctx):
    tris, tree = chain_tris(crt), crt.host_kd_build(S.mesh("chain"))        # (alive until the call returns: the description holds pointers into them)
    a = crt.alt_desc(KD, tris, tree)
    ctx._ck(ctx.L.crt_upload_alt_accel(ctx.h, C.byref(a)))


def open_world(crt, t, accel, W=32, H=32, placement=None, **cfg):
    """(context, host scene or None) of a world as the host front builds it, with its KD-trees uploaded where `accel` asks for them"""
    ctx = crt.Context(W, H, **cfg)
    if t.name == "chain":
        p = S.mesh("chain")
        TG.upload_described(crt, ctx, described(crt, p, crt.host_bvh_build(p)))
        if accel == "kd":
            upload_chain_kd(crt, ctx)
        return ctx, None
    hs = crt.HostScene(S.scene_file(t.name, t.tmp), t.kind, ASSETS)
    if t.kind == 1:
        S.place(hs, placement or t.name)
    if accel == "kd":
        hs.build_alt(KD)
    hs.upload(ctx)
    if accel == "kd":
        hs.upload_alt(ctx, KD)
    return ctx, hs


def assert_allotted(ctx, t, accel, n_bvh=None):
    """what the library allots is what the rays reach (BVH, TLAS part) or, for the KD part, one more than any ray can hold and than these rays hold where the CPU
    module says so"""
    n = n_bvh or (7 if t.kind == 1 else 1)
    a = S.allotted(ctx, accel, n)
    w = t.walk[accel]
    assert a["tlas"] == (w.tlas_height + 1 if t.kind == 1 else 0), a
    if accel == "bvh":
        assert a["entries"] == S.BVH_ENTRIES[t.name] == t.attained["bvh"], (a, t.attained)
    else:
        assert (a["bvh"], t.attained["kd"]) == S.KD_ENTRIES[t.name], (a, t.attained)
        if t.kind == 1:
            assert t.kd_tlas == a["tlas"] - 1
    return a


def code(accel):
    return KD if accel == "kd" else 0


def query_all_ways(crt, ctx, t, accel, what):
    """find_nearest, find_nearest_device, is_occluded, is_occluded_device (and find_nearest_alt for a FileScene's KD-tree) against the oracle"""
    (O, D), want, ts, occ = t.rays[accel], t.want[accel], t.shadow_t[accel], t.occluded[accel]
    a = code(accel)
    dev = TG.hits_np(crt, ctx.find_nearest_device(TG.ray_records(crt, O, D), accel=a)); torch.cuda.synchronize()
    assert_hits(dev, want, (what, "find_nearest_device"))
    if a == 0:
        assert_hits(ctx.find_nearest(O, D), want, (what, "find_nearest"))
    elif t.kind == 0:
        assert_hits(ctx.find_nearest_alt(KD, O, D), want, (what, "find_nearest_alt"))
    assert np.array_equal(np.asarray(ctx.is_occluded(O, D, ts, accel=a)) != 0, occ != 0), (what, "is_occluded")
    d = ctx.is_occluded_device(TG.ray_records(crt, O, D, ts, crt.SHADOW_RAY_DTYPE), accel=a).cpu().numpy()
    assert np.array_equal(d != 0, occ != 0), (what, "is_occluded_device")
    assert (occ[t.is_fill[accel]] == 0).sum() >= S.MIN_FILLING               # shadow rays that miss every triangle walk the whole ray: the full stack


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 1. the query entries
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", S.WORLDS)
def test_query_entries_at_the_bound(crt, orc, truths, monkeypatch, name, accel):
    t = truths(name)
    ctx, _ = open_world(crt, t, accel)
    assert_allotted(ctx, t, accel)
    query_all_ways(crt, ctx, t, accel, (name, accel, "unbounded"))
    monkeypatch.setenv(SWITCH, "1")                                         # one workgroup works through all 512 rays: every lane takes 8 of them
    query_all_ways(crt, ctx, t, accel, (name, accel, "one workgroup"))
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 2. the ray-array integrators
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", S.WORLDS)
def test_sample_and_trace_at_the_bound(crt, orc, truths, monkeypatch, name, accel):
    t = truths(name)
    ctx, _ = open_world(crt, t, accel)
    assert_allotted(ctx, t, accel)
    (O, D), want, a = t.rays[accel], t.want[accel], code(accel)
    seeds = (np.arange(N_MIX, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)) | np.uint32(1)
    S.through(orc, t.o, accel)
    try:
        ref = [t.o.sample(O[i], D[i], int(seeds[i])) for i in range(N_MIX)]
    finally:
        S.through(orc, t.o, "bvh")
    ref_rgb = np.stack([r[0] for r in ref]); ref_seed = np.array([r[1] for r in ref], np.uint32)
    rays = np.zeros(N_MIX, crt.RAY_DTYPE); rays["O"], rays["D"] = O, D
    d_rays = TG.ray_records(crt, O, D)
    d_seeds = torch.from_numpy(seeds.view(np.int32).copy()).to(TG.dev())
    for k in (None, "1"):
        if k:
            monkeypatch.setenv(SWITCH, k)
        rgb, s = ctx.sample(O, D, seeds, accel=a)
        assert same_floats(rgb, ref_rgb) and np.array_equal(s, ref_seed), (name, accel, k, "sample")
        rgb_d, s_d = ctx.sample_device(d_rays, seeds=d_seeds, accel=a); torch.cuda.synchronize()
        assert same_floats(rgb_d.cpu().numpy(), ref_rgb) and np.array_equal(s_d.cpu().numpy().view(np.uint32), ref_seed), (name, accel, k, "sample_device")
        # Trace: the depth-0 ray's counts are FindNearest's; the colours of the two entries agree (the camera rays' are held to the oracle's image in test 3)
        rgb_t, trav, tested = ctx.trace(rays, accel=a, counts=True)
        assert np.array_equal(trav, want["traversed"]) and np.array_equal(tested, want["tested"]), (name, accel, k, "trace")
        rgb_td, trav_d, tested_d = ctx.trace_device(d_rays, accel=a, counts=True); torch.cuda.synchronize()
        assert np.array_equal(trav_d.cpu().numpy(), want["traversed"]) and np.array_equal(tested_d.cpu().numpy(), want["tested"]), (name, accel, k, "trace_device")
        assert same_floats(rgb_td.cpu().numpy(), rgb_t) and np.isfinite(rgb_t).all()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 3. the Whitted Tick and its inspection, the camera on the axis; Trace of the same rays
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", ["compact", "tlas_compact"])
def test_whitted_tick_at_the_bound(crt, orc, truths, name, accel):
    t = truths(name); cam = S.CAMERA; W, H = cam["W"], cam["H"]
    held = t.camera(orc, "bvh")["held"]
    assert (held == S.BVH_ENTRIES[name]).sum() >= S.MIN_FILLING              # pixels whose unjittered primary ray fills the BVH world's stack
    e = t.camera(orc, accel)
    ctx, _ = open_world(crt, t, accel, W, H)
    assert_allotted(ctx, t, accel)
    ctx.set_camera_state(cam["pos"], cam["target"]); ctx.set_render_accel(code(accel))
    px = ctx.whitted_tick()
    assert np.array_equal(px, e["screen"]) and same_floats(ctx.accumulator()[..., :3], e["acc"][..., :3])
    px2, m, tr, te = ctx.whitted_tick_inspect(crt.INSPECT_NONE, counts=True)
    assert np.array_equal(px2, e["screen"])
    assert np.array_equal(tr.reshape(-1), e["hits"]["traversed"]) and np.array_equal(te.reshape(-1), e["hits"]["tested"])
    rgb, trav, tested = ctx.trace_device(TG.ray_records(crt, e["O"], e["D"]), accel=code(accel), counts=True); torch.cuda.synchronize()
    assert same_floats(rgb.cpu().numpy(), e["acc"].reshape(-1, 4)[:, :3])
    assert np.array_equal(trav.cpu().numpy(), e["hits"]["traversed"]) and np.array_equal(tested.cpu().numpy(), e["hits"]["tested"])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 4. the render kernels
# ---------------------------------------------------------------------------------------------------------------------------------------------------
#            name            environment                                                             frames  kernel
RENDERS = [("tiles",         {"CRT_RENDER_KERNEL": "tiles"},                                              4, "tiles"),
           ("pool64",        {"CRT_RENDER_KERNEL": "pool_always"},                                        6, "pool"),
           ("pool128",       {"CRT_RENDER_KERNEL": "pool_always", "CRT_POOL_WAVE_FRAMES": "256"},       130, "pool"),
           ("pool_ref32",    {"CRT_RENDER_KERNEL": "pool_always", "CRT_DEBUG_NO_REF16": "1"},             6, "pool"),
           ("pool_rootref",  {"CRT_RENDER_KERNEL": "pool_always", "CRT_DEBUG_NO_ROOTPAIR": "1"},          6, "pool"),
           ("kd",            {},                                                                          4, "seq")]
CAMERA2 = ((-1.5, 0.45, 0.55), (0.0, 0.45, 0.55))                          # a second camera near the axis for render_views


@pytest.fixture(scope="module")
def oracle_renders(orc, truths):
    """the oracle's accumulator and counters of a (world, structure, camera, frames), rendered once"""
    memo = {}

    def get(name, accel, camera, frames):
        key = (name, accel, camera, frames)
        if key not in memo:
            t = truths(name); o = t.o
            o.renderer_init(S.CAMERA["W"], S.CAMERA["H"])
            S.through(orc, o, accel)
            try:
                memo[key] = oracle_view(o, camera, 1, frames, 1)
            finally:
                S.through(orc, o, "bvh")
        return memo[key]
    return get


@pytest.mark.parametrize("config", RENDERS, ids=[r[0] for r in RENDERS])
@pytest.mark.parametrize("name", ["compact", "tlas_compact"])
def test_render_kernels_at_the_bound(crt, orc, truths, oracle_renders, monkeypatch, name, config):
    label, env, frames, kernel = config
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = truths(name); cam = S.CAMERA; W, H = cam["W"], cam["H"]
    assert (t.camera(orc, "bvh")["held"] == S.BVH_ENTRIES[name]).sum() >= S.MIN_FILLING
    accel = "kd" if label == "kd" else "bvh"
    ctx, _ = open_world(crt, t, accel, W, H, max_frames_per_launch=4096)
    assert_allotted(ctx, t, accel)
    ctx.set_camera_state(cam["pos"], cam["target"])
    if accel == "kd":
        ctx.set_render_accel(KD)
        assert ctx.L.crt_debug_render_accel(ctx.h) == KD
    ctx.render(1, frames, 1)
    tm = ctx.timing()
    if kernel == "seq":                                                     # neither the tiles nor the pool kernel: render_seq_kernel, whose launches are not timed
        assert tm["render_launches"] == 0 and tm["pool_launches"] == 0, tm
    else:
        assert tm["render_launches"] >= 1 and (tm["pool_launches"] >= 1) == (kernel == "pool"), tm
    if kernel == "pool":
        assert ctx.pool_lds(frames)[2] == (32 if label == "pool_ref32" else 16)
        ctx.L.crt_debug_pool_long_waves.restype = C.c_int
        assert (ctx.L.crt_debug_pool_long_waves(ctx.h) > 0) == (label == "pool128")     # wavefronts that own more than 128 frames: 128 stream slots, two refills
    want, counters = oracle_renders(name, accel, (cam["pos"], cam["target"]), frames)
    assert np.array_equal(bits(ctx.accumulator()), bits(want)), (name, label)
    assert ctx.counters()["rays"] == counters["rays"]
    ctx.close()


@pytest.mark.parametrize("name", ["compact", "tlas_compact"])
def test_render_views_at_the_bound(crt, orc, truths, oracle_renders, name):
    t = truths(name); cam = S.CAMERA; W, H = cam["W"], cam["H"]
    assert (t.camera(orc, "bvh")["held"] == S.BVH_ENTRIES[name]).sum() >= S.MIN_FILLING
    ctx, _ = open_world(crt, t, "bvh", W, H)
    assert_allotted(ctx, t, "bvh")
    cams = ((cam["pos"], cam["target"]), CAMERA2)
    got = ctx.render_views(crt.camera_records(W, H, cams), 1, 4)
    for k, c in enumerate(cams):
        assert np.array_equal(bits(got[k]), bits(oracle_renders(name, "bvh", c, 4)[0])), (name, k)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 5. the sizing after device-side writes
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_build_bvh_device_sizes_the_stack_for_the_new_tree(crt, orc, truths):
    t = truths("chain"); p = S.mesh("chain")
    ctx = crt.Context(32, 32)
    TG.upload_described(crt, ctx, TG.leaf_root_bvh(crt, p))
    assert S.allotted(ctx)["entries"] == 1                                  # a leaf root: the smallest stack there is
    ctx.build_bvh_device(0, TG.to_dev(p))
    assert_allotted(ctx, t, "bvh")
    c2, _ = open_world(crt, t, "bvh")                                       # a second context that uploaded the host-built tree
    assert_same_scene(ctx, c2, "chain, device-built")
    query_all_ways(crt, ctx, t, "bvh", "chain, device-built")
    O, D = t.rays["bvh"]
    assert_hits(ctx.find_nearest(O, D), c2.find_nearest(O, D), "against the host-built scene")
    ctx.clear(); c2.clear(); ctx.render(1, 2, 1); c2.render(1, 2, 1)
    assert np.array_equal(bits(ctx.accumulator()), bits(c2.accumulator()))
    ctx.close(); c2.close()


def test_build_kdtree_device_sizes_the_stack_for_the_new_tree(crt, orc, truths):
    t = truths("chain"); p = S.mesh("chain")
    ctx, _ = open_world(crt, t, "bvh")
    ctx.build_kdtree_device(0, TG.to_dev(p))
    assert_allotted(ctx, t, "kd")
    query_all_ways(crt, ctx, t, "kd", "chain, device-built KD-tree")
    c2, _ = open_world(crt, t, "kd")
    O, D = t.rays["kd"]
    assert_hits(ctx.find_nearest_alt(KD, O, D), c2.find_nearest_alt(KD, O, D), "against the host-built KD-tree")
    ctx.close(); c2.close()


def test_update_transforms_device_sizes_the_stack_for_the_new_tlas(crt, orc, truths, tmp_path):
    """the instances of the deep two-level scene from the lattice (TLAS height 3, 12 entries) to the line (height 6, 15 entries) and back, the filling rays
    after each move, against the oracle in the same placement and against a second context that uploaded the host-built scene (adopt_tlas)"""
    t = truths("tlas_deep")
    O, D = t.rays["bvh"]
    flat = S.load_oracle(orc, "tlas_deep", tmp_path, placement="tlas_deep_flat")
    w_flat = S.World(orc, flat, "bvh")
    want = {"tlas_deep": t.want["bvh"], "tlas_deep_flat": flat.find_nearest(O, D)}
    entries = {"tlas_deep": 15, "tlas_deep_flat": 12}
    assert w_flat.entries() == 12
    ctx, _ = open_world(crt, t, "bvh", placement="tlas_deep_flat")
    assert S.allotted(ctx)["entries"] == 12
    for placement in ("tlas_deep", "tlas_deep_flat", "tlas_deep"):
        nodes = ctx.update_transforms_device(TG.to_dev(S.transforms(placement)))
        assert nodes.tobytes() == (t.o if placement == "tlas_deep" else flat).tlas()[0].tobytes(), placement
        a = S.allotted(ctx)
        assert (a["entries"], a["bvh"]) == (entries[placement], 8), (placement, a)
        c2, _ = open_world(crt, t, "bvh", placement=placement)
        assert S.scene_words(ctx).tolist() == S.scene_words(c2).tolist(), placement     # offsets, root reference, root pair flag, stack depths, LDS bytes
        got = TG.hits_np(crt, ctx.find_nearest_device(TG.ray_records(crt, O, D))); torch.cuda.synchronize()
        assert_hits(got, want[placement], (placement, "find_nearest_device"))
        assert_hits(ctx.find_nearest(O, D), c2.find_nearest(O, D), (placement, "against the host-built scene"))
        ctx.clear(); c2.clear(); ctx.render(1, 2, 1); c2.render(1, 2, 1)
        assert np.array_equal(bits(ctx.accumulator()), bits(c2.accumulator())), placement
        c2.close()
    assert_allotted(ctx, t, "bvh")
    query_all_ways(crt, ctx, t, "bvh", "the line, after two moves")
    ctx.close()
