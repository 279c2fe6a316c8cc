"""The Whitted renderer's traversal inspection and per-Tick metrics on the GPU (crt_whitted_tick_inspect, Renderer::TickWhitted with the two inspect flags).
Expected values never come from the library: per-pixel Ray::traversed / Ray::tested from the CPU oracle's FindNearest on the pixel grid's primary rays (through
its own KD-tree / grid for FileScene; for the two-level KD-tree / grid through tests/tlas_alt_restate.py at 64 x 48 and through the oracle's own two-level walk,
orc.set_blas_accel, at 320 x 192), sky pixels and the shaded image from Oracle.whitted() (at 320 x 192 through the same two-level structure),
the running peak and GetTraverseCountColor from tests/inspect_restate.py (itself pinned to the reference's helper.h by test_whitted_inspect_cpu.py).
Everything is compared with np.array_equal, floats as bits."""
import re

import numpy as np
import pytest

from conftest import ASSETS, scene_path
import inspect_restate as IR
import tlas_alt_restate as TR

pytestmark = pytest.mark.gpu
NAME = {1: "kd", 2: "grid"}


def light_of(xml):
    m = re.search(r"<light_position><x>([^<]+)</x><y>([^<]+)</y><z>([^<]+)</z>", open(xml).read())
    return tuple(float(v) for v in m.groups())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def expected(crt, orc, xml, kind, accel, W, H, camera=None, two_level="restatement"):
    """the primary rays' records of the oracle, in row-major pixel order: traversed, tested (H, W) int32, hit (H, W) bool, and the oracle's Whitted
    accumulator / screen / counters of the same Tick (sky pixels, the shaded image)"""
    path = scene_path(xml)
    o, _ = orc.load_scene(path, kind, ASSETS)
    o.renderer_init(W, H)
    if camera:
        o.set_camera_state(*camera)
    ys, xs = np.mgrid[0:H, 0:W]
    O, D = o.primary_rays(np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32))      # GetPrimaryRay((float)x, (float)y)
    keep = None
    if accel == 0:
        h = o.find_nearest(O, D)
    elif kind == 0:
        keep = orc.alt_accel(NAME[accel], o.bvh(0)["tris"])
        orc.set_render_accel(o, keep)
        h = o.find_nearest(O, D)
    elif two_level == "oracle":                                                           # the C++ oracle walks TLASKDTree / TLASGrid: counts and Whitted image through it
        orc.set_blas_accel(o, orc.blas_accels(o, NAME[accel]))
        h = o.find_nearest(O, D)
    else:
        h = TR.Scene(orc, o, NAME[accel], light_of(path)).find_nearest_many(O, D, crt.HIT_DTYPE)
        hb = o.find_nearest(O, D)
        assert np.array_equal(hb["objIdx"] == -1, h["objIdx"] == -1)                      # the sky pixels of the oracle's image below are this structure's misses
    o.reset_counters()
    o.whitted(4)
    e = dict(traversed=h["traversed"].reshape(H, W).astype(np.int32), tested=h["tested"].reshape(H, W).astype(np.int32), hit=(h["objIdx"] != -1).reshape(H, W),
             acc=o.accumulator(), screen=o.screen(), counters=o.counters(), mesh_hits=int((h["objIdx"] >= 2).sum()))
    if keep is not None:
        orc.set_render_accel(o, None); keep.close()
    return e


def upload(crt, xml, kind, accel, W, H):
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    ctx = crt.Context(W, H)
    hs.upload(ctx)
    if accel:
        hs.build_alt(accel); hs.upload_alt(ctx, accel); ctx.set_render_accel(accel)
    return hs, ctx


def guards(e, tlas):
    """the inputs exercise the feature (asserted on the EXPECTED data, for both counts)"""
    for name in ("traversed", "tested"):
        peaks, _ = IR.running_peak(e[name], 0)
        hit = e["hit"]
        assert ((e[name] > peaks) & (peaks >= 10) & hit).sum() >= 3, name              # clamped hit pixels: blend == 1
        assert len(np.unique(peaks)) >= 5, name
        assert ((peaks >= 10) & hit).sum() > 0, name
        if tlas:
            assert ((peaks < 10) & hit).sum() > 0, name                                 # hit pixels still green under a running peak below 10


def check_mode(ctx, e, mode, pt, ps, sky):
    """one Tick in an inspect mode against the restatement; returns the peaks carried out"""
    ctx.reset_counters()
    px, m, tr, te = ctx.whitted_tick_inspect(mode, pt, ps, counts=True)
    assert np.array_equal(tr, e["traversed"]) and np.array_equal(te, e["tested"]), mode
    assert m == IR.metrics(e["traversed"], e["tested"], pt, ps), (mode, m)
    count, pin = (e["traversed"], pt) if mode == 1 else (e["tested"], ps)
    acc, screen, _, _ = IR.heat_map(count, e["hit"], sky, pin)
    got = ctx.accumulator()
    assert np.array_equal(bits(got), bits(acc)), (mode, pt, ps, int((bits(got) != bits(acc)).any(axis=-1).sum()))
    assert np.array_equal(px, screen), (mode, pt, ps)
    assert np.array_equal(bits(got[~e["hit"]]), bits(e["acc"][~e["hit"]]))              # sky pixels are Oracle.whitted()'s
    c = ctx.counters()
    n = count.size
    assert c["rays"] == n and c["primary"] == n and c["mesh_hits"] == e["mesh_hits"], c  # one ray per pixel
    return m["peakTraversal"], m["peakTests"]


CONFIGS = [("bunny_scene.xml", 0, 0, 320, 192, (57, 18)), ("bunny_scene.xml", 0, 1, 320, 192, (202, 75)), ("bunny_scene.xml", 0, 2, 320, 192, (57, 153)),
           ("tlas_scene.xml", 1, 0, 320, 192, (128, 62)), ("tower_scene.xml", 0, 0, 200, 120, (188, 98)),
           ("tlas_scene.xml", 1, 1, 64, 48, (392, 232)), ("tlas_scene.xml", 1, 2, 64, 48, (101, 382)),
           ("tlas_scene.xml", 1, 1, 320, 192, (442, 690)), ("tlas_scene.xml", 1, 2, 320, 192, (104, 557))]


@pytest.mark.parametrize("xml,kind,accel,W,H,peaks", CONFIGS)
def test_counts_metrics_and_heat_maps(crt, orc, xml, kind, accel, W, H, peaks):
    """per-pixel traversed / tested, hit count, totals and peaks in modes 0 / 1 / 2; the heat maps of a first Tick (peaks 0 / 0), of a second Tick with the
    peaks the first returned (every hit pixel scaled by the global maximum) and of a Tick with carried-in peaks larger than the frame's maxima"""
    e = expected(crt, orc, xml, kind, accel, W, H, two_level="restatement" if (W, H) == (64, 48) else "oracle")
    assert (int(e["traversed"].max()), int(e["tested"].max())) == peaks                   # the reference values this case was chosen for
    guards(e, xml == "tlas_scene.xml")
    if (xml, accel) == ("bunny_scene.xml", 0):
        assert (int(e["traversed"].sum()), int(e["tested"].sum())) == (154932, 15578) and len(np.unique(IR.running_peak(e["traversed"], 0)[0])) == 20
    if (xml, accel) == ("bunny_scene.xml", 2):
        assert int((e["traversed"] > 0).sum()) == 7055                                    # rayHitCount != W*H
    hs, ctx = upload(crt, xml, kind, accel, W, H)
    sky = e["acc"]
    # mode 0: the shaded image, the counts and the metrics; the peaks passed in come back raised
    px, m, tr, te = ctx.whitted_tick_inspect(0, 3, 100000, counts=True)
    assert np.array_equal(tr, e["traversed"]) and np.array_equal(te, e["tested"])
    assert m == IR.metrics(e["traversed"], e["tested"], 3, 100000) and m["peakTests"] == 100000 and m["peakTraversal"] == peaks[0]
    assert np.array_equal(bits(ctx.accumulator()), bits(e["acc"])) and np.array_equal(px, e["screen"])
    for mode in (1, 2):
        pt, ps = check_mode(ctx, e, mode, 0, 0, sky)
        assert (pt, ps) == peaks
        assert check_mode(ctx, e, mode, pt, ps, sky) == (pt, ps)
        big = (pt + 41, ps + 1000)
        assert check_mode(ctx, e, mode, *big, sky) == big
    # the pixels-only form of the call (no count images, no metrics) leaves the same picture
    px2, _ = ctx.whitted_tick_inspect(1, 0, 0)
    assert np.array_equal(px2, IR.heat_map(e["traversed"], e["hit"], sky, 0)[1])
    ctx.close(); hs.close()


def test_scan_tail_on_a_33_by_17_image(crt, orc):
    """an image that fills neither a wavefront nor a block of the scan"""
    W, H = 33, 17
    e = expected(crt, orc, "bunny_scene.xml", 0, 0, W, H)
    hs, ctx = upload(crt, "bunny_scene.xml", 0, 0, W, H)
    for mode in (1, 2):
        pt, ps = check_mode(ctx, e, mode, 0, 0, e["acc"])
        check_mode(ctx, e, mode, pt, ps, e["acc"])
        check_mode(ctx, e, mode, 12, 11, e["acc"])
    ctx.close(); hs.close()


def test_peak_under_ten_is_green(crt, orc):
    """BASELINE config 1 (cube, 640 x 360): the reference peaks are 9 / 4, so every hit pixel is exactly `green` in both modes, on the first and the second Tick"""
    W, H = 640, 360
    e = expected(crt, orc, "cube_scene.xml", 0, 0, W, H)
    assert (int(e["traversed"].max()), int(e["tested"].max())) == (9, 4)
    hs, ctx = upload(crt, "cube_scene.xml", 0, 0, W, H)
    green = np.array(IR.GREEN + (np.float32(0),), np.float32)
    for mode in (1, 2):
        pt, ps = check_mode(ctx, e, mode, 0, 0, e["acc"])
        assert (pt, ps) == (9, 4)
        assert np.all(bits(ctx.accumulator()[e["hit"]]) == bits(green))
        check_mode(ctx, e, mode, pt, ps, e["acc"])
        assert np.all(bits(ctx.accumulator()[e["hit"]]) == bits(green)) and e["hit"].sum() > 1000
    ctx.close(); hs.close()


@pytest.mark.parametrize("xml,kind,W,H", [("cube_scene.xml", 0, 640, 360), ("tlas_scene.xml", 1, 320, 192), ("tlas_scene.xml", 0, 160, 96), ("tower_scene.xml", 0, 200, 120)])
def test_mode_0_is_the_shaded_image(crt, orc, xml, kind, W, H):
    """accumulator, screen and counters of CRT_INSPECT_NONE equal crt_whitted_tick's and the oracle's (the cases of test_whitted_tick_matches_oracle)"""
    e = expected(crt, orc, xml, kind, 0, W, H)
    hs, ctx = upload(crt, xml, kind, 0, W, H)
    px0 = ctx.whitted_tick(); acc0 = ctx.accumulator(); c0 = ctx.counters()
    ctx.clear(); ctx.reset_counters()
    px, m, tr, te = ctx.whitted_tick_inspect(0, 0, 0, counts=True)
    acc = ctx.accumulator(); c = ctx.counters()
    assert np.array_equal(bits(acc), bits(acc0)) and np.array_equal(px, px0) and c == c0
    assert np.array_equal(bits(acc), bits(e["acc"])) and np.array_equal(px, e["screen"])
    for k in c:
        assert c[k] == e["counters"][k], (k, c[k], e["counters"][k])
    assert np.array_equal(tr, e["traversed"]) and np.array_equal(te, e["tested"]) and m == IR.metrics(e["traversed"], e["tested"])
    ctx.close(); hs.close()


def test_precedence_and_facade(crt, orc):
    """HostRenderer: both flags set give the traversal map; three Ticks in a row carry the peaks; set_camera resets them; the averages"""
    W, H = 320, 192
    cam = ((0.3, 0.4, -2.5), (0.1, 0.0, 0.0))
    e = expected(crt, orc, "bunny_scene.xml", 0, 0, W, H, camera=cam)
    assert e["traversed"].max() >= 10 and e["tested"].max() >= 10
    hs = crt.HostScene(scene_path("bunny_scene.xml"), 0, ASSETS)
    r = crt.HostRenderer(hs, W, H); r.init()
    r.set_camera(*cam)
    r.tick_whitted()                                                                      # both flags off: the shaded image, and the metrics all the same
    assert np.array_equal(bits(r.accumulator()), bits(e["acc"])) and np.array_equal(r.screen(), e["screen"])
    want = IR.metrics(e["traversed"], e["tested"])
    m = r.whitted_metrics()
    assert {k: m[k] for k in want} == want
    assert bits(m["averageTraversal"]) == bits(np.float32(want["totalTraversal"]) / np.float32(want["rayHitCount"]))
    assert bits(m["averageTests"]) == bits(np.float32(want["totalTests"]) / np.float32(want["rayHitCount"]))
    first = IR.heat_map(e["traversed"], e["hit"], e["acc"], 0)
    carried = IR.heat_map(e["traversed"], e["hit"], e["acc"], want["peakTraversal"])
    assert not np.array_equal(first[0], carried[0])
    r.set_camera(*cam)                                                                    # resets peaks and averages
    z = r.whitted_metrics()
    assert z["peakTraversal"] == 0 and z["peakTests"] == 0 and z["averageTraversal"] == 0 and z["averageTests"] == 0
    r.set_inspect(True, True)                                                             # traversal wins
    r.tick_whitted()
    assert np.array_equal(bits(r.accumulator()), bits(first[0])) and np.array_equal(r.screen(), first[1])
    for _ in range(2):
        r.tick_whitted()
        assert np.array_equal(bits(r.accumulator()), bits(carried[0])) and np.array_equal(r.screen(), carried[1])
        m = r.whitted_metrics()
        assert {k: m[k] for k in want} == want
    r.set_camera(*cam)
    r.tick_whitted()                                                                      # equals a first Tick again
    assert np.array_equal(bits(r.accumulator()), bits(first[0])) and np.array_equal(r.screen(), first[1])
    r.set_inspect(False, True)                                                            # the tests map, with the tests peak carried from the Tick before
    r.tick_whitted()
    t = IR.heat_map(e["tested"], e["hit"], e["acc"], want["peakTests"])
    assert np.array_equal(bits(r.accumulator()), bits(t[0])) and np.array_equal(r.screen(), t[1])
    r.close(); hs.close()


def test_refusals_leave_the_accumulator(crt, orc):
    W, H = 64, 48
    ctx = crt.Context(W, H)
    with pytest.raises(crt.CrtError) as x:
        ctx.whitted_tick_inspect(1)                                                       # no scene
    assert x.value.code == -5
    with pytest.raises(crt.CrtError) as y:
        ctx.whitted_tick()
    assert y.value.code == x.value.code                                                   # refused as crt_whitted_tick refuses it
    hs = crt.HostScene(scene_path("bunny_scene.xml"), 0, ASSETS); hs.upload(ctx)
    ctx.whitted_tick()
    before = ctx.accumulator(); px_before = ctx.resolve_screen(1.0)[0]
    for args in ((3, 0, 0), (-1, 0, 0), (1, -1, 0), (2, 0, -5), (0, -1, -1)):
        with pytest.raises(crt.CrtError) as x:
            ctx.whitted_tick_inspect(*args)
        assert x.value.code == -1, args
        assert np.array_equal(bits(ctx.accumulator()), bits(before)), args
    assert np.array_equal(ctx.resolve_screen(1.0)[0], px_before)
    ps = crt.HostPrimitiveScene(ASSETS); ps.upload(ctx)
    ctx.clear(); ctx.render(1, 1, 1)
    before = ctx.accumulator()
    codes = []
    for call in (lambda: ctx.whitted_tick_inspect(1), lambda: ctx.whitted_tick_inspect(0), ctx.whitted_tick):
        with pytest.raises(crt.CrtError) as x:
            call()
        codes.append(x.value.code)
        assert np.array_equal(bits(ctx.accumulator()), bits(before))
    assert codes[0] == codes[1] == codes[2]
    ctx.close(); hs.close()
