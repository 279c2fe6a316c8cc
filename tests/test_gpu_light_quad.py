"""The light quad of a look — turned, resized (render_looks_inputs.quad_looks) — on the GPU, against what is not the library:
  the float64 truth of tests/mesh_truth.py (World(light_T=, light_half=)) on the rays of tests/light_quad_inputs.py, with the criterion, tolerances and caps that
  tests/test_mesh_truth_cpu.py settles on the oracle: find_nearest / find_nearest_device / find_nearest_alt, is_occluded(accel) and its device entry, get_hit_info;
  the oracle with set_light_quad (pinned to the reference's own Quad by tests/test_oracle_pinning.py), bit for bit: the same queries through the BVH / TLAS, the
  KD-tree and the grid and their two-level sets, Sample ray by ray, the Whitted image, crt_render through the tiles kernel, the pool kernel and its 32-bit form,
  and one crt_render_looks job of all the quads;
  tests/hit_info_restate.py under the look, bit for bit: get_hit_info's records and get_light;
  for the two quads of exact cells, light_quad_inputs.axis_form (a float32 one-liner) and the exactly parallel / exactly in-plane rays.
Each look is applied by update_look on a live scene and by a fresh upload of the scene with that look; both must give the same."""
import numpy as np
import pytest

import hit_info_restate as hr
import light_quad_inputs as lq
import mesh_truth as mt
import mesh_truth_scenes as MC
import render_looks_inputs as li
from conftest import ASSETS, scene_path

torch = pytest.importorskip("torch")

from test_gpu_hit_info import assert_info_equal                            # noqa: E402
from test_gpu_mesh_truth import check_queries, nearest_all_ways, same_bits  # noqa: E402
from test_gpu_render_looks import same                                     # noqa: E402

pytestmark = pytest.mark.gpu

W, H = li.W, li.H
NAMES = {s: ("z25", "zyx", "y45", "quarter_z", "half_x", "zyx_size_0.9") + tuple("size_%g" % x for x in li.SIZES[s]) for s in li.SCENES}
CASES = [(s, n) for s in sorted(li.SCENES) for n in NAMES[s]]
FRAMES = 3


class Rig:
    """a scene on a live context per accelerator (the look arrives by update_look) and one that is uploaded anew per look; the oracle's scene and the
    restatement's; every look's rays and truth, computed once"""

    def __init__(self, crt, orc, scene):
        self.crt, self.orc, self.scene = crt, orc, scene
        xml, self.kind = li.SCENES[scene]
        self.hs, self.hs_fresh = crt.HostScene(scene_path(xml), self.kind, ASSETS), crt.HostScene(scene_path(xml), self.kind, ASSETS)
        self.base = crt.look_dicts(self.hs.look())[0]
        self.looks = li.quad_looks(scene, self.base)
        assert set(self.looks) == set(NAMES[scene])
        self.rec = {n: crt.look_records([k])[0] for n, k in self.looks.items()}
        self.accels = {"": 0, "kd": crt.ACCEL_KDTREE, "grid": crt.ACCEL_GRID}
        self.live = {}
        for w, accel in self.accels.items():
            ctx = crt.Context(W, H); self.hs.upload(ctx)
            if accel:
                self.hs.build_alt(accel); self.hs.upload_alt(ctx, accel)
            self.live[w] = ctx
        self.fresh = crt.Context(W, H)
        self.o, self.sc = orc.load_scene(scene_path(xml), self.kind, ASSETS)
        self.o.renderer_init(W, H)
        self.sh = hr.SceneShading(orc, self.o, self.sc, self.kind, ASSETS)
        self._cases = {}

    def world_name(self, w):
        return (w or "bvh") if self.kind == 0 else ("tlas_" + w if w else "tlas")

    def case(self, name):
        if name not in self._cases:
            self._cases[name] = lq.Case(self.orc, self.scene, name, self.looks[name], self.hs)
        return self._cases[name]

    def oracle(self, name, world=""):
        """the oracle's scene with the look's quad, walked through `world`'s structure"""
        look = self.looks[name]
        self.o.set_light_quad(look["light_T"], look["light_invT"], look["light_size"])
        self.sh.set_look(look)
        return MC.through(self.orc, self.o, self.world_name(world))

    def upload_fresh(self, name, ctx=None):
        self.hs_fresh.set_look(self.rec[name]); self.hs_fresh.upload(ctx or self.fresh)
        return ctx or self.fresh

    def close(self):
        for x in list(self.live.values()) + [self.fresh]:
            x.close()


@pytest.fixture(scope="module")
def rigs(crt, orc):
    cache = {}

    def get(scene):
        if scene not in cache:
            cache[scene] = Rig(crt, orc, scene)
        return cache[scene]
    yield get
    for r in cache.values():
        r.close()


# 1: the queries, against the truth, the oracle and the restatement
@pytest.mark.parametrize("scene,name", CASES)
def test_queries_under_a_quad_look(crt, rigs, scene, name):
    r = rigs(scene); c = r.case(name); look = r.looks[name]
    front, back = c.light_faces()
    assert front >= 50 and back >= 50, (front, back)
    o = r.oracle(name)
    want = o.find_nearest(c.O, c.D); want_occ = o.is_occluded(c.O, c.D, c.ts) != 0
    want_info = r.sh.hit_info(c.O, c.D, want)
    q = o.light()
    assert np.array_equal(q["pos"].view(np.uint32), r.sh.light_pos().view(np.uint32))
    seeds = (np.arange(len(c.O), dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)) | np.uint32(1)
    exact = lq.exact_rays(np.asarray(look["light_T"], np.float32), look["light_size"], 5) if name in ("quarter_z", "half_x") else None
    r.live[""].update_look(r.rec[name])
    for how, ctx in (("update_look", r.live[""]), ("fresh upload", r.upload_fresh(name))):
        what = "%s under %s, %s" % (scene, name, how)
        hits, n = check_queries(crt, ctx, r.kind, 0, c.O, c.D, c.tr, c.ti, c.ts, c.occ, what)        # the truth: every find-nearest entry, is_occluded, get_hit_info
        assert n >= 0.7 * len(c.O)
        assert same_bits(hits, want, slice(None)), (what, "find_nearest against the oracle")
        assert np.array_equal(np.asarray(ctx.is_occluded(c.O, c.D, c.ts)), want_occ), (what, "is_occluded against the oracle")
        assert_info_equal(ctx.get_hit_info(c.O, c.D, hits), want_info, what)
        pos, col = ctx.get_light()
        assert np.array_equal(pos.view(np.uint32), q["pos"].view(np.uint32)) and np.array_equal(col, np.float32([24, 24, 22])), (what, "get_light")
        got, seed_out = ctx.sample(c.O, c.D, seeds.copy())[:2]
        # Sample's first hit against the truth: where the nearest candidate is robustly the light, the light's colour whatever the seed (renderer.cpp:69);
        # where there is no candidate at all, the sky's colour for the direction (the restatement's GetSkyColor)
        lit = (c.tr["kind_hi"] == 0) & (c.tr["kind"] == 0) & c.tr["unique"] & ~c.tr["uninformative"]
        none = ~np.isfinite(c.tr["t_lo"])
        assert lit.sum() >= 300 and none.sum() >= 100
        assert (got[lit] == np.float32([24, 24, 22])).all(), (what, "sample: a ray whose first hit is the light")
        assert same(got[none], r.sh.sky(c.D[none])), (what, "sample: a ray that meets nothing")
        for i in range(0, len(c.O), 8):                                     # ... and against the oracle's Sample, seed for seed
            rgb, s = o.sample(c.O[i], c.D[i], int(seeds[i]))
            assert same(got[i], rgb) and int(seed_out[i]) == s, (what, "sample", i)
        if name in ("quarter_z", "half_x"):
            cand, t = lq.axis_form(name, np.asarray(look["light_T"], np.float32), look["light_size"], c.O, c.D)
            lit = hits["objIdx"] == 0
            assert lit.sum() >= 150 and cand[lit].all() and np.array_equal(hits["t"][lit].view(np.uint32), t[lit].view(np.uint32)), (what, "the one-liner")
            assert (hits["t"][cand & ~lit] < t[cand & ~lit]).all()
            eh = ctx.find_nearest(*exact)
            assert not (eh["objIdx"] == 0).any() and same_bits(eh, o.find_nearest(*exact), slice(None)), (what, "parallel and in-plane rays")
            assert np.array_equal(np.asarray(ctx.is_occluded(exact[0], exact[1], 3.0)), o.is_occluded(exact[0], exact[1], 3.0) != 0), what
    # the KD-tree and the grid (kind 0), the two-level sets (kind 1): the look arrives behind the structure's upload
    for w in ("kd", "grid"):
        ctx, accel = r.live[w], r.accels[w]
        ctx.update_look(r.rec[name])
        ow = r.oracle(name, w)
        want_w = ow.find_nearest(c.O, c.D)
        what = "%s under %s through %s" % (scene, name, r.world_name(w))
        hits = nearest_all_ways(crt, ctx, r.kind, accel, c.O, c.D)
        assert same_bits(hits, want_w, slice(None)), (what, "find_nearest against the oracle")
        assert np.array_equal(np.asarray(ctx.is_occluded(c.O, c.D, c.ts, accel=accel)), ow.is_occluded(c.O, c.D, c.ts) != 0), (what, "is_occluded")
        if r.world_name(w) != "tlas_kd":                                    # (the two-level KD-tree loses hits, as the reference's does: mesh_truth.TLAS_KD_VIOLATIONS)
            viol = mt.nearest_violations(c.tr, hits)
            assert not viol, MC.report(what, viol, c.O, c.D, hits, c.tr)
        lightv = {k: v[c.tr["kind"][v] == 0] for k, v in mt.nearest_violations(c.tr, hits).items()}
        assert not any(len(v) for v in lightv.values()), (what, "a ray whose nearest candidate is the light", lightv)
    r.oracle(name)


# 2: the images
@pytest.mark.parametrize("scene,name", CASES)
def test_renders_under_a_quad_look(crt, rigs, monkeypatch, scene, name):
    r = rigs(scene); o = r.oracle(name)
    ctx = r.live[""]
    ctx.update_look(r.rec[name])
    fresh = r.upload_fresh(name)
    for cam in (li.CAMERAS[scene], li.QUAD_CAMERAS[scene]):
        want = li.oracle_render(o, cam, 1, FRAMES, 1)
        for how, x in (("update_look", ctx), ("fresh upload", fresh)):
            x.set_camera_state(*cam); x.clear(); x.render(1, FRAMES, 1)
            assert same(x.accumulator(), want), (scene, name, how, cam)
    # the Whitted image: the point light under the quad's centre, the quad itself, its shadow rays; and the trace query on the image's own rays (the oracle
    # traces its camera's rays through integer pixel coordinates, 2. WhittedStyle/renderer.cpp:144)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    for cam in (li.CAMERAS[scene], li.QUAD_CAMERAS[scene]):
        o.set_camera_state(*cam); o.whitted(4)
        want = o.accumulator()
        O, D = o.primary_rays(np.stack([xs.ravel(), ys.ravel()], axis=1))
        rays = np.zeros(len(O), crt.RAY_DTYPE); rays["O"], rays["D"] = O, D
        for how, x in (("update_look", ctx), ("fresh upload", fresh)):
            x.set_camera_state(*cam); x.whitted_tick()
            assert same(x.accumulator(), want), (scene, name, how, "whitted_tick")
            assert same(np.asarray(x.trace(rays)), want.reshape(-1, 4)[:, :3]), (scene, name, how, "trace")
    # the pool kernel and its 32-bit form
    cam = li.QUAD_CAMERAS[scene]
    want = li.oracle_render(o, cam, 1, 8, 1)
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")
    for ref16 in (True, False):
        if not ref16:
            monkeypatch.setenv("CRT_DEBUG_NO_REF16", "1")
        a = crt.Context(W, H, max_frames_per_launch=4096)
        r.hs.upload(a); a.update_look(r.rec[name])
        a.set_camera_state(*cam); a.render(1, 8, 1)
        t = a.timing()
        assert t["render_launches"] == 1 and t["pool_launches"] == 1, t
        assert same(a.accumulator(), want), (scene, name, "pool kernel", "16-bit" if ref16 else "32-bit")
        a.close()


# 3: one job of all the quads
@pytest.mark.parametrize("scene", sorted(li.SCENES))
def test_one_render_looks_job_of_all_the_quads(crt, rigs, scene):
    r = rigs(scene); names = list(NAMES[scene])
    cams = [(li.CAMERAS[scene], li.QUAD_CAMERAS[scene])[k % 2] for k in range(len(names))]
    ctx = r.live[""]
    ctx.update_look(r.rec[names[0]])                                        # the live look is one of them; the job leaves it alone
    acc = ctx.render_looks(crt.camera_records(W, H, cams), np.stack([r.rec[n] for n in names]), 1, FRAMES, 1)
    assert acc.shape == (len(names), H, W, 4)
    for k, n in enumerate(names):
        assert same(acc[k], li.oracle_render(r.oracle(n), cams[k], 1, FRAMES, 1)), (scene, n)
    ctx.set_camera_state(*cams[0]); ctx.clear(); ctx.render(1, FRAMES, 1)
    assert same(ctx.accumulator(), acc[0])


# 4: the floor's texel under a look that selects another floor texture: the uv scale stays the uploaded texture's
@pytest.mark.parametrize("scene", sorted(li.SCENES))
def test_floor_records_under_another_floor_texture(crt, rigs, scene):
    r = rigs(scene)
    looks = li.looks(scene, r.base)
    o, sc = r.orc.load_scene(scene_path(li.SCENES[scene][0]), r.kind, ASSETS)
    sh = hr.SceneShading(r.orc, o, sc, r.kind, ASSETS)
    O, D = li.floor_rays(sh.floor_invto)
    ctx = r.live[""]
    for name in ("floor", "all"):
        look = looks[name]; rec = crt.look_records([look])[0]
        sh.set_look(look)
        ol = li.make_oracle(r.orc, scene, look)
        want_hits = ol.find_nearest(O, D)
        want = sh.hit_info(O, D, want_hits)
        ctx.update_look(rec)
        r.hs_fresh.set_look(rec); r.hs_fresh.upload(r.fresh)
        for how, x in (("update_look", ctx), ("fresh upload", r.fresh)):
            hits = x.find_nearest(O, D)
            assert same_bits(hits, want_hits, slice(None)), (scene, name, how)
            assert (hits["objIdx"] == 1).sum() >= 0.7 * len(O)
            assert_info_equal(x.get_hit_info(O, D, hits), want, "%s under %s, %s" % (scene, name, how))
    ctx.update_look(r.rec[NAMES[scene][0]])
    r.hs_fresh.set_look(crt.look_records([r.base])[0])
