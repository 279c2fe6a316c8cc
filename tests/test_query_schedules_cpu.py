"""The premise of tests/test_gpu_query_lane_reuse.py, checked with the CPU oracle alone: every ray order of tests/query_schedules.py is what it claims to be, on
the scenes the GPU test uses.
  * every order names distinct rays of its pool, as many as the launch takes; shuffled / ascending / descending / degenerate_mixed are permutations of the rays
    they are given, walker_among_idlers and leading_done_at_refill of the rays they select;
  * walker_among_idlers: one walker per 64 rays, at position (7 g) mod 64 of group g; every idler has tested == 0 and the smallest traversed the scene's walk
    reports; every walker costs at least 20 times what an idler costs (an idler's cost counted as at least 1: a ray outside the grid's box costs 0);
  * leading_done_at_refill: every leading shadow ray is quad-occluded by test_gpu_scene_queries.quad_occluded; every leading Sample ray meets a refusal rule;
  * ascending / descending are sorted by the oracle's cost; degenerate_mixed leaves no long stretch without a flagged ray.
Run with -s to see the measured values."""
import numpy as np
import pytest

import query_schedules as qs
import sample_query_inputs as si
from conftest import ASSETS, scene_path
from test_gpu_golden_and_edges import write_scene
from test_gpu_scene_queries import LIGHT, light_of

W, H = 64, 32                                                             # as tests/test_gpu_sample_query.py


def check_orders(case, ks, what, idler_hits=True):
    pool, cost = case.pool, case.cost
    for k in ks:
        n0 = pool.n0(k)
        lanes = (256 if pool.sample else 64) * k
        assert n0 == lanes * (8 if pool.sample else 24)                    # every lane holds 8 / 24 rays on average
        orders = pool.orders(k, cost)
        assert set(orders) >= {"shuffled", "ascending", "descending", "walker_among_idlers", "degenerate_mixed"}
        for name, order in orders.items():
            want_len = n0 + max(qs.TAILS) if name == "shuffled" else n0
            assert len(order) == want_len and len(np.unique(order)) == want_len and order.min() >= 0 and order.max() < len(pool.O), (what, k, name)
        given = pool.ordinary[:n0]
        for name in ("ascending", "descending", "degenerate_mixed"):
            assert np.array_equal(np.sort(orders[name]), given), (what, k, name)
        assert np.array_equal(np.sort(orders["shuffled"]), pool.ordinary[: n0 + max(qs.TAILS)])
        assert not np.array_equal(orders["shuffled"], np.sort(orders["shuffled"]))
        assert (np.diff(cost[orders["ascending"]]) >= 0).all() and (np.diff(cost[orders["descending"]]) <= 0).all()
        assert cost[orders["ascending"]][-1] > cost[orders["ascending"]][0]
        # degenerate rays: present, and spread
        flagged = int(pool.flags[given].sum())
        assert flagged >= n0 // 16, (what, k, flagged)
        gap = qs.largest_gap(orders["degenerate_mixed"], pool.flags)
        assert gap <= -(-n0 // flagged), (what, k, gap, flagged)
        # walker_among_idlers
        order = orders["walker_among_idlers"]
        pos = qs.walker_positions(n0)
        assert len(pos) == n0 // 64 and (pos // 64 == np.arange(n0 // 64)).all()      # one walker per 64 rays
        is_walker = np.zeros(n0, bool); is_walker[pos] = True
        walkers, idlers = order[is_walker], order[~is_walker]
        assert np.isin(walkers, pool.ordinary).all() and np.isin(idlers, pool.idlers).all()
        if idler_hits:
            assert (case.walk["tested"][idlers] == 0).all() and (case.walk["traversed"][idlers] == case.least).all(), (what, k)
        idler_cost = max(int(cost[idlers].max()), 1)
        assert cost[walkers].min() >= 20 * idler_cost, (what, k, int(cost[walkers].min()), idler_cost)
        print("%s k=%d: n0 %d, idlers traversed %s tested 0 cost %d..%d, walkers' cost %d..%d, flagged %d largest gap %d" % (
            what, k, n0, case.least if idler_hits else "-", cost[idlers].min(), cost[idlers].max(), cost[walkers].min(), cost[walkers].max(), flagged, gap))
        # leading_done_at_refill
        if "leading_done_at_refill" in orders:
            lead = orders["leading_done_at_refill"][: 2 * lanes]
            assert np.isin(lead, pool.leading).all()
            assert not np.isin(orders["leading_done_at_refill"][2 * lanes:], pool.leading).any()
            if pool.sample:
                assert qs.refused(pool.O[lead], pool.D[lead], pool.seeds[lead]).all(), (what, k)
                assert not qs.refused(pool.O[pool.ordinary], pool.D[pool.ordinary], pool.seeds[pool.ordinary]).any()
                kinds = [int(((pool.seeds[lead] == 0)).sum()), int(np.isnan(pool.D[lead]).any(axis=1).sum()), int(np.isinf(pool.O[lead]).any(axis=1).sum()),
                         int((pool.D[lead] == 0).all(axis=1).sum())]
                assert min(kinds) >= len(lead) // 8, kinds
            else:
                assert case.quad[lead].all(), (what, k)                    # by the quad_occluded restatement
                assert (pool.last[lead] == np.float32(1e34)).all()
            print("%s k=%d: %d leading rays, all %s" % (what, k, len(lead), "refused" if pool.sample else "quad-occluded"))


@pytest.mark.parametrize("xml,kind", [("cube_scene.xml", 0), ("bunny_scene.xml", 0), ("tlas_scene.xml", 1)])
def test_find_nearest_orders(orc, xml, kind):
    case = qs.find_nearest_case(orc, scene_path(xml), kind, ASSETS)
    assert (case.pool.D == 0).any(axis=1).sum() >= 100 and (case.want["objIdx"] == 0).sum() >= 50 and (case.pool.last != 0).sum() >= 100
    check_orders(case, (1, 3), "find_nearest %s" % xml)


@pytest.mark.parametrize("scene", ["bunny", "tlas"])
def test_occlusion_orders(orc, tmp_path, scene):
    xml, kind, light = (write_scene(tmp_path, "bunny"), 0, LIGHT) if scene == "bunny" else (scene_path("tlas_scene.xml"), 1, light_of(scene_path("tlas_scene.xml")))
    case = qs.occlusion_case(orc, xml, kind, ASSETS, light)
    m = case.walk["objIdx"][case.pool.ordinary] >= 2; q = case.quad[case.pool.ordinary]
    for name, sel in (("quad only", q & ~m), ("mesh only", ~q & m), ("both", q & m), ("neither", ~q & ~m)):
        assert sel.sum() >= 20, (name, int(sel.sum()))
    assert not case.quad[case.pool.idlers].any()                          # an idler is not done in the refill: it takes its one trip
    check_orders(case, (1, 3), "is_occluded %s" % scene)


@pytest.mark.parametrize("kind", ["kd", "grid"])
def test_alt_orders(orc, tmp_path, kind):
    fn, oc = qs.alt_cases(orc, write_scene(tmp_path, "bunny"), kind, ASSETS, LIGHT)
    check_orders(fn, (1, 3), "find_nearest_alt %s" % kind)
    assert not oc.quad[oc.pool.idlers].any()
    check_orders(oc, (1, 3), "is_occluded_alt %s" % kind)


@pytest.mark.parametrize("kind", ["kd", "grid"])
def test_tlas_alt_orders(orc, kind):
    xml = scene_path("tlas_scene.xml")
    fn, oc = qs.tlas_alt_cases(orc, xml, kind, ASSETS, light_of(xml))
    assert len(fn.pool.O) - len(fn.pool.idlers) <= 1600 and fn.pool.n0(1) + max(qs.TAILS) <= 1600
    check_orders(fn, (1,), "tlas_alt find_nearest %s" % kind)
    assert not oc.quad[oc.pool.idlers].any()
    check_orders(oc, (1,), "tlas_alt is_occluded %s" % kind)


@pytest.mark.parametrize("world", ["bvh", "kd", "grid", "tlas", "tlas_kd", "tlas_grid", "prim"])
def test_sample_orders(orc, tmp_path, world):
    if world == "prim":
        o = orc.primitive_scene(ASSETS, 1.3)
    else:
        o, _ = orc.load_scene(si.scene_xml(tmp_path), 1 if world.startswith("tlas") else 0, ASSETS)
        if world in ("kd", "grid"):
            orc.set_render_accel(o, orc.alt_accel(world, o.bvh(0)["tris"]))
        if world in ("tlas_kd", "tlas_grid"):
            orc.set_blas_accel(o, orc.blas_accels(o, world[5:]))
    o.renderer_init(W, H)
    case = qs.sample_case(o, world)
    pool = case.pool
    assert (case.cost[pool.idlers] == 0).all()                             # an idler's path ends in its first trip: no number drawn
    assert np.array_equal(case.want[1][pool.idlers], pool.seeds[pool.idlers]) and np.isfinite(case.want[0][pool.idlers]).all()
    assert np.isnan(case.want[0][pool.leading]).all() and np.array_equal(case.want[1][pool.leading], pool.seeds[pool.leading])
    check_orders(case, (1, 3), "sample %s" % world, idler_hits=False)
    if world in ("tlas_kd", "tlas_grid"):                                   # the committed disagreement rays sit among the ordinary rays of every launch, as they are
        import alt_disagreement as ad
        Oa, Da, _, sa, _ = ad.load(world[5:])
        held = {(O.tobytes(), D.tobytes(), int(s)) for O, D, s in zip(pool.O[pool.ordinary], pool.D[pool.ordinary], pool.seeds[pool.ordinary])}
        assert all((O.tobytes(), D.tobytes(), int(s)) in held for O, D, s in zip(Oa, Da, sa))
        for k in (1, 3):
            first = {(O.tobytes(), D.tobytes()) for O, D in zip(pool.O[pool.ordinary[:pool.n0(k)]], pool.D[pool.ordinary[:pool.n0(k)]])}
            assert sum((O.tobytes(), D.tobytes()) in first for O, D in zip(Oa, Da)) >= len(Oa) * k // 3 - 1
