"""render_pool_kernel's throughput-factor path: the BOUNCE pass stores a bounce's factor in the wavefront's rows of the factor scratch (workgroup-scope
atomics: one wavefront writes and reads them), the END pass fetches the levels a path reached — level k + 1 inside level k's region — and multiplies them
on the unwind, innermost first.  Every depth limit 0 .. 5 makes another level of that nest the deepest one, so each is rendered and held to the oracle bit
for bit, with and without the statistics build.  32 x 32 x 192 frames are 4 tiles of 128 slots plus a refilled partial range: a slot's factor rows are
written by one stream and then by the stream that takes the slot over."""
import numpy as np
import pytest

from conftest import ASSETS, scene_path

pytestmark = pytest.mark.gpu

W, H, FRAMES = 32, 32, 192
SCENES = [("bunny_scene.xml", 0), ("cube_scene.xml", 0), ("tlas_scene.xml", 1)]
DEPTHS = range(6)
CASES = [(xml, kind, d, 1) for xml, kind in SCENES for d in DEPTHS] + [("bunny_scene.xml", 0, 5, 2)]


@pytest.fixture(scope="module")
def want(orc):
    """the oracle's accumulator and counters of every case, rendered once (one oracle per scene) and left unchanged"""
    out = {}
    for xml, kind in SCENES:
        o, _ = orc.load_scene(scene_path(xml), kind, ASSETS)
        o.renderer_init(W, H)
        for x, k, depth, passes in CASES:
            if x != xml:
                continue
            o.set_params(depth, passes)
            o.clear(); o.reset_counters()
            o.render(FRAMES, 4)
            acc = o.accumulator(); acc.setflags(write=False)
            out[(xml, depth, passes)] = (acc, o.counters())
    return out


@pytest.fixture(scope="module")
def host_scenes(crt):
    return {xml: crt.HostScene(scene_path(xml), kind, ASSETS) for xml, kind in SCENES}


@pytest.mark.parametrize("xml,kind", SCENES)
def test_every_depth_limit_reaches_another_level(want, xml, kind):
    """from the oracle alone: each step of the depth limit changes the image, so at these sizes paths end at every depth 0 .. 5 and every level of the
    fetch / unwind nest is the deepest one of some path (a scene edit cannot quietly turn the deep levels into dead code)"""
    for d in range(1, 6):
        a, b = want[(xml, d - 1, 1)][0], want[(xml, d, 1)][0]
        changed = int((a != b).any(axis=2).sum())
        print("%s depth limit %d -> %d: %d pixels change" % (xml, d - 1, d, changed))
        assert changed > 0, (xml, d)


@pytest.mark.parametrize("stats", [True, False], ids=["stats", "plain"])
@pytest.mark.parametrize("xml,kind,depth,passes", CASES)
def test_factor_path_matches_oracle(crt, want, host_scenes, monkeypatch, xml, kind, depth, passes, stats):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")
    ctx = crt.Context(W, H, depth_limit=depth, collect_stats=stats, max_frames_per_launch=4096)
    try:
        host_scenes[xml].upload(ctx)
        ctx.render(1, FRAMES, passes)
        acc = ctx.accumulator()
        assert ctx.timing()["pool_launches"] == 1
        ref, cnt = want[(xml, depth, passes)]
        assert np.array_equal(acc, ref)
        if stats:
            assert ctx.counters() == cnt
        else:
            assert ctx.counters()["rays"] == cnt["rays"]
    finally:
        ctx.close()
