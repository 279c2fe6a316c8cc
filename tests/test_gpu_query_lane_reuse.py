"""The steady state of the persistent query kernels, held to the oracle: find_nearest_kernel, is_occluded_kernel, find_nearest_alt_kernel<1|2>,
is_occluded_alt_kernel<1|2>, tlas_alt_query_kernel<1|2, false|true> and sample_query_kernel in every world.  A lane that finishes its ray takes the next one of
the launch-wide cursor and reuses its registers, its LDS stack column and its counters; at the sizes the other tests use there is a workgroup per 64 (256) rays,
so hardly any lane ever takes a second ray.  Here CRT_DEBUG_QUERY_GRID=k bounds a launch to k workgroups — k = 1: one workgroup works through all n rays, a
deterministic schedule; k = 3: wavefronts also contend for the cursor — so that every lane holds 24 (Sample: 8) rays on average, and the rays come in the orders
of tests/query_schedules.py, which tests/test_query_schedules_cpu.py checks without a GPU.

Expected values never depend on the order: they are the per-ray answers of the oracle (oracle/orc.py), of its restatements of the KD-tree / grid, of
tests/tlas_alt_restate.py and of test_gpu_scene_queries.quad_occluded, indexed by the order; the two-level KD-tree / grid Sample worlds' are orc_sample through the
same structure (orc.set_blas_accel).  Floats are compared as bit patterns (any NaN equals any NaN), counters exactly.  One comparison is an AGREEMENT check between
two runs of the product and says so where it stands: the switch test's bounded against unbounded launch."""
import numpy as np
import pytest

import alt_disagreement as ad
import query_schedules as qs
import sample_query_inputs as si
from conftest import ASSETS, scene_path
from probe_inputs import differing
from test_gpu_golden_and_edges import write_scene
from test_gpu_sample_query import Worlds, records, seeds_np, seeds_t
from test_gpu_scene_queries import FIELDS, LIGHT, hits_np, light_of, ray_records, shadow_records

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SWITCH = "CRT_DEBUG_QUERY_GRID"
COUNTED = ("rays", "interior_iters", "leaf_iters", "tri_tests", "tlas_iters", "blas_visits", "mesh_hits")     # as test_gpu_parity.test_find_nearest_bit_exact


@pytest.fixture(scope="module")
def cases():
    """the pools and the oracle's answers, made once per (kernel, scene) and never changed"""
    memo = {}

    def get(key, make):
        if key not in memo:
            memo[key] = make()
        return memo[key]
    return get


def assert_fields(got, want, fields, what, sel=None):
    for f in fields:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        if sel is not None:
            a, b = a[sel], b[sel]
        bad = differing(a, b.astype(a.dtype)) if a.dtype == np.float32 else np.flatnonzero(a != b)
        assert len(bad) == 0, (what, f, len(bad), bad[:8].tolist())


def launches(pool, k, cost):
    """(name, order) of every launch of one (kernel, scene, k): each schedule at the base size, `shuffled` also at the tail sizes (prefixes of one order)"""
    n0 = pool.n0(k)
    lanes = (256 if pool.sample else 64) * k
    assert n0 // lanes == (8 if pool.sample else 24) and n0 % lanes == 0     # rays per lane, on average
    for name, order in pool.orders(k, cost).items():
        if name == "shuffled":
            for r in qs.TAILS:
                yield "shuffled + %d" % r, order[: n0 + r]
        else:
            yield name, order


def start(crt, xml, kind, accels=()):
    hs = crt.HostScene(xml, kind, ASSETS)
    ctx = crt.Context(64, 64)
    for a in accels:
        hs.build_alt(a)
    hs.upload(ctx)
    for a in accels:
        hs.upload_alt(ctx, a)
    return hs, ctx


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the switch itself
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_switch_bounds_the_launch_and_is_dead_without_hooks(crt, orc, cases, monkeypatch):
    """One workgroup answers all 64 * 24 rays and counts each once.  The comparison with the unbounded launch is an AGREEMENT check between two runs of the product
    (the oracle comparison of the bounded launch is test_find_nearest_lane_reuse).  With the hooks off the variable is not read: the library's results and
    counters are those of the unbounded launch."""
    case = cases(("fn", "bunny_scene.xml", 0), lambda: qs.find_nearest_case(orc, scene_path("bunny_scene.xml"), 0, ASSETS))
    hs, ctx = start(crt, scene_path("bunny_scene.xml"), 0)
    pool = case.pool
    n = 64 * 24
    order = qs.shuffled(pool.ordinary[:n])
    O, D, inside = pool.O[order], pool.D[order], pool.last[order]

    def run():
        ctx.reset_counters()
        return ctx.find_nearest(O, D, inside), ctx.counters()
    free, c_free = run()
    monkeypatch.setenv(SWITCH, "1")
    one, c_one = run()
    assert c_one["rays"] == n
    assert_fields(one, free, FIELDS, "bounded against unbounded (agreement)")
    assert c_one == c_free
    assert_fields(one, case.want[order], FIELDS, "bounded against the oracle")
    crt.lib().crt_debug_enable_hooks(0)
    try:
        off, c_off = run()
    finally:
        crt.lib().crt_debug_enable_hooks(1)
    assert_fields(off, free, FIELDS, "hooks off (agreement)")
    assert c_off == c_free
    monkeypatch.setenv(SWITCH, "0")                                         # 0: no bound
    zero, c_zero = run()
    assert_fields(zero, free, FIELDS, "k = 0 (agreement)")
    assert c_zero == c_free
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# find_nearest_kernel
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("xml,kind", [("cube_scene.xml", 0), ("bunny_scene.xml", 0), ("tlas_scene.xml", 1)])
def test_find_nearest_lane_reuse(crt, orc, cases, monkeypatch, xml, kind, k):
    case = cases(("fn", xml, kind), lambda: qs.find_nearest_case(orc, scene_path(xml), kind, ASSETS))
    hs, ctx = start(crt, scene_path(xml), kind)
    pool, o = case.pool, case.o
    monkeypatch.setenv(SWITCH, str(k))
    for name, order in launches(pool, k, case.cost):
        O, D, inside = pool.O[order], pool.D[order], pool.last[order]
        o.reset_counters(); o.find_nearest(O, D, inside); oc = o.counters()
        assert oc["rays"] == len(order)
        for entry in ("host", "device"):
            ctx.reset_counters()
            if entry == "host":
                got = ctx.find_nearest(O, D, inside)
            else:
                got = hits_np(crt, ctx.find_nearest_device(ray_records(O, D, inside))); torch.cuda.synchronize()
            assert_fields(got, case.want[order], FIELDS, (xml, k, name, entry))
            gc = ctx.counters()
            assert {c: gc[c] for c in COUNTED} == {c: oc[c] for c in COUNTED}, (xml, k, name, entry)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# is_occluded_kernel
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def occlusion_launches(ctx, case, k, accel, what):
    pool = case.pool
    for name, order in launches(pool, k, case.cost):
        O, D, t = pool.O[order], pool.D[order], pool.last[order]
        want = case.want[order]
        got = ctx.is_occluded(O, D, t, accel=accel)
        assert np.array_equal(got, want), (what, k, name, "host", np.flatnonzero(got != want)[:8].tolist())
        got = ctx.is_occluded_device(shadow_records(O, D, t), accel=accel).cpu().numpy()
        assert set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got != 0, want), (what, k, name, "device", np.flatnonzero((got != 0) != want)[:8].tolist())


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("scene", ["bunny", "tlas"])
def test_is_occluded_lane_reuse(crt, orc, cases, monkeypatch, tmp_path_factory, scene, k):
    if scene == "bunny":
        xml, kind, light = cases(("xml", "bunny"), lambda: write_scene(tmp_path_factory.mktemp("reuse"), "bunny")), 0, LIGHT
    else:
        xml, kind, light = scene_path("tlas_scene.xml"), 1, light_of(scene_path("tlas_scene.xml"))
    case = cases(("occ", scene), lambda: qs.occlusion_case(orc, xml, kind, ASSETS, light))
    hs, ctx = start(crt, xml, kind)
    monkeypatch.setenv(SWITCH, str(k))
    occlusion_launches(ctx, case, k, 0, scene)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# find_nearest_alt_kernel<1|2>, is_occluded_alt_kernel<1|2>
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("kind", ["kd", "grid"])
def test_alt_accel_lane_reuse(crt, orc, cases, monkeypatch, tmp_path_factory, kind, k):
    """FindNearest tests the light quad and the floor before the accelerator, the restatement is the accelerator alone over the whole ray: where the device reports
    a miss the whole record, visit counters included, is the restatement's; a mesh hit is the same hit (test_gpu_alt_accel.test_alt_accel_edge_cases_and_errors).
    Rays without a zero direction component must also get the BVH's answer, here the oracle's FindNearest."""
    xml = cases(("xml", "bunny"), lambda: write_scene(tmp_path_factory.mktemp("reuse"), "bunny"))
    fn, oc = cases(("alt", kind), lambda: qs.alt_cases(orc, xml, kind, ASSETS, LIGHT))
    code = crt.ACCEL_KDTREE if kind == "kd" else crt.ACCEL_GRID
    hs, ctx = start(crt, xml, 0, (code,))
    monkeypatch.setenv(SWITCH, str(k))
    pool = fn.pool
    for name, order in launches(pool, k, fn.cost):
        O, D, inside = pool.O[order], pool.D[order], pool.last[order]
        want, bvh = fn.want[order], fn.bvh[order]
        general = np.all(D != 0, axis=1)
        for entry in ("host", "device"):
            if entry == "host":
                got = ctx.find_nearest_alt(code, O, D)
            else:
                got = hits_np(crt, ctx.find_nearest_device(ray_records(O, D, inside), accel=code)); torch.cuda.synchronize()
            what = (kind, k, name, entry)
            miss, mesh = got["objIdx"] == -1, got["objIdx"] >= 2
            assert_fields(got, want, FIELDS, what + ("miss",), miss)
            assert_fields(got, want, ("t", "u", "v", "triIdx"), what + ("mesh",), mesh)
            assert_fields(got, bvh, ("t", "u", "v", "objIdx", "triIdx"), what + ("BVH answer",), general)
            if name.startswith("shuffled"):
                assert miss.sum() > 50 and mesh.sum() > 50 and (~general).sum() > 50, what
    occlusion_launches(ctx, oc, k, code, kind)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# tlas_alt_query_kernel<1|2, false|true>
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["kd", "grid"])
def test_tlas_alt_lane_reuse(crt, orc, cases, monkeypatch, kind):
    """the restatement is Python per ray: one workgroup (k = 1) and at most 1 600 rays a launch"""
    xml = scene_path("tlas_scene.xml")
    fn, oc = cases(("tlas_alt", kind), lambda: qs.tlas_alt_cases(orc, xml, kind, ASSETS, light_of(xml)))
    code = crt.ACCEL_KDTREE if kind == "kd" else crt.ACCEL_GRID
    hs, ctx = start(crt, xml, 1, (code,))
    monkeypatch.setenv(SWITCH, "1")
    pool = fn.pool
    for name, order in launches(pool, 1, fn.cost):
        assert len(order) <= 1600
        O, D, inside = pool.O[order], pool.D[order], pool.last[order]
        assert_fields(ctx.find_nearest_alt(code, O, D), fn.want[order], FIELDS, (kind, name, "host"))
        got = hits_np(crt, ctx.find_nearest_device(ray_records(O, D, inside), accel=code)); torch.cuda.synchronize()
        assert_fields(got, fn.want[order], FIELDS, (kind, name, "device"))
    occlusion_launches(ctx, oc, 1, code, "tlas " + kind)
    ctx.close(); hs.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# sample_query_kernel
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worlds(crt, orc, tmp_path_factory):
    ws = Worlds(crt, orc, tmp_path_factory.mktemp("reuse_sample"))
    yield ws
    for w in ws.cache.values():
        w.ctx.close()


def sample_both(crt, ctx, pool, order, accel):
    """(entry, rgb, seeds out, growth of the rays / mesh_hits counters) through crt_sample and crt_sample_device"""
    O, D, inside, seeds = pool.O[order], pool.D[order], pool.last[order], pool.seeds[order]
    ctx.sync(); c0 = ctx.counters()
    rgb, s = ctx.sample(O, D, seeds, inside, accel=accel)
    c1 = ctx.counters()
    yield "host", rgb, s, {c: c1[c] - c0[c] for c in ("rays", "mesh_hits")}
    rgb, s = ctx.sample_device(rays=records(crt, O, D, inside), seeds=seeds_t(seeds), accel=accel)
    torch.cuda.synchronize()
    c2 = ctx.counters()
    yield "device", rgb.cpu().numpy(), seeds_np(s), {c: c2[c] - c1[c] for c in ("rays", "mesh_hits")}


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("world", ["bvh", "kd", "grid", "tlas", "prim"])
def test_sample_lane_reuse(crt, cases, worlds, monkeypatch, world, k):
    w = worlds.get(world)
    case = cases(("sample", world), lambda: qs.sample_case(w.o, world))
    pool = case.pool
    monkeypatch.setenv(SWITCH, str(k))
    for name, order in launches(pool, k, case.cost):
        counted = {c: int(pool.counted[c][order].sum()) for c in ("rays", "mesh_hits")}
        for entry, rgb, s, grown in sample_both(crt, w.ctx, pool, order, w.accel):
            what = (world, k, name, entry)
            bad = differing(rgb, case.want[0][order])
            assert len(bad) == 0, (what, "rgb", len(bad), bad[:8].tolist())
            bad = np.flatnonzero(s != case.want[1][order])
            assert len(bad) == 0, (what, "seeds", len(bad), bad[:8].tolist())
            assert grown == counted, what


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("world", ["tlas_kd", "tlas_grid"])
def test_sample_two_level_alt_bounded_equals_unbounded(crt, cases, worlds, monkeypatch, world, k):
    """the two-level KD-tree / grid Sample worlds against orc_sample through the same structure: the bounded launch (every lane reused) and the same world's
    unbounded launch of the same rays (a workgroup per 256 rays: hardly a lane reused) both give the oracle's radiance, seeds and counter growth, bit for bit"""
    w = worlds.get(world)
    case = cases(("sample", world), lambda: qs.sample_case(w.o, world))
    pool = case.pool
    for name, order in launches(pool, k, case.cost):
        counted = {c: int(pool.counted[c][order].sum()) for c in ("rays", "mesh_hits")}
        monkeypatch.delenv(SWITCH, raising=False)
        free = list(sample_both(crt, w.ctx, pool, order, w.accel))
        monkeypatch.setenv(SWITCH, str(k))
        for (entry, rgb, s, grown), (_, rgb0, s0, grown0) in zip(sample_both(crt, w.ctx, pool, order, w.accel), free):
            what = (world, k, name, entry)
            assert len(differing(rgb, rgb0)) == 0 and np.array_equal(s, s0) and grown == grown0, what
            bad = differing(rgb, case.want[0][order])
            assert len(bad) == 0, (what, "rgb", len(bad), bad[:8].tolist())
            bad = np.flatnonzero(s != case.want[1][order])
            assert len(bad) == 0, (what, "seeds", len(bad), bad[:8].tolist())
            assert grown == counted, what
            lead = qs.refused(pool.O[order], pool.D[order], pool.seeds[order])
            assert np.isnan(rgb[lead]).all() and np.isfinite(rgb[~lead]).all() and np.array_equal(s[lead], pool.seeds[order][lead]), what


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("kind", ["kd", "grid"])
def test_sample_lane_reuse_on_the_disagreement_rays(crt, orc, cases, monkeypatch, kind, k):
    """tlas_scene.xml through the two-level structure, k workgroups, 8 rays a lane: primary rays of the default camera with the committed rays on which the
    structures disagree spread evenly among them, so a reused lane carries a path that parts from the TLAS-BVH's path next to ordinary ones.  Against orc_sample
    through the same structure; the premise (through the TLAS-BVH most of those paths end elsewhere) is asserted on the oracle's two answers."""
    xml = scene_path("tlas_scene.xml"); code = crt.ACCEL_KDTREE if kind == "kd" else crt.ACCEL_GRID

    def make():
        b, a = ad.scene_pair(orc, xml, ASSETS, kind)
        a.renderer_init(64, 64)
        n = 256 * 8 * 3
        rng = np.random.default_rng(31)
        O, D = a.primary_rays(np.stack([rng.uniform(0, 64, n), rng.uniform(0, 64, n)], 1).astype(np.float32))
        inside = np.zeros(n, np.int32); seeds = si.seeds_for(n)
        Oa, Da, ia, sa, _ = ad.load(kind)
        at = (np.arange(len(Oa)) * n) // len(Oa)
        O[at], D[at], inside[at], seeds[at] = Oa, Da, ia, sa
        want = si.oracle_sample(a, O, D, inside, seeds)
        bvh = si.oracle_sample(b, O[at], D[at], inside[at], seeds[at])
        assert (want[1][at] != bvh[1]).sum() >= 50
        return O, D, inside, seeds, want
    O, D, inside, seeds, want = cases(("sample disagreement", kind), make)
    n = 256 * 8 * k                                                          # a prefix: a third of the spread rays for k = 1, all of them for k = 3
    hs, ctx = start(crt, xml, 1, (code,))
    monkeypatch.setenv(SWITCH, str(k))
    for r in (0, 17):
        m = n - r
        rgb, s = ctx.sample(O[:m], D[:m], seeds[:m], inside[:m], accel=code)
        assert len(differing(rgb, want[0][:m])) == 0 and np.array_equal(s, want[1][:m]), (kind, k, r, "host")
        rgb, s = ctx.sample_device(rays=records(crt, O[:m], D[:m], inside[:m]), seeds=seeds_t(seeds[:m]), accel=code)
        torch.cuda.synchronize()
        assert len(differing(rgb.cpu().numpy(), want[0][:m])) == 0 and np.array_equal(seeds_np(s), want[1][:m]), (kind, k, r, "device")
    ctx.close(); hs.close()
