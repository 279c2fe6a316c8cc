"""render_pool_kernel's control diet ("control diet"): the loop's wave-uniform decisions as scalar compares, the slab-test choice made once
per trip, the shading passes' lane sets as compare masks.  All of it is control and address arithmetic, so nothing here has a tolerance: every case renders one
small job with the pool kernel and is held to the oracle bit for bit — the accumulator, and in a statistics context every counter.

The cases are the frame counts at which that control takes another path (64 x 32 pixels = 8 tiles each):
  1              the wave is starving from the first trip; the exit with a single stream
  63, 64         queues that never reach 64 entries, or reach 64 exactly                              (64 stream slots)
  65, 127, 128   the pass threshold from both sides; ring indices past 127                            (128 slots)
  129 | 256      one wavefront per tile that refills exactly one frame
  300 | 256      ... and a short last range
  128, 2 passes  the `passes != 1` arms of the END pass
  128, sky       a raised camera: some tiles are sky tiles (every new ray is a finished path), with the class table on and off
  128, wide      the 32-bit reference form"""
import numpy as np
import pytest

from conftest import ASSETS, scene_path

pytestmark = pytest.mark.gpu

W, H = 64, 32
SCENES = [("cube_scene.xml", 0), ("tlas_scene.xml", 1)]
RAISED = ((0.0, 1.0, -5.0), (0.0, 2.5, 0.0))       # looks up across the scene: the lower tile row sees floor and meshes, the upper one light and sky
#        frames passes wave  camera  wide   slots
CASES = [(1,    1, None, None,   False, 64),
         (63,   1, None, None,   False, 64),
         (64,   1, None, None,   False, 64),
         (65,   1, None, None,   False, 128),
         (127,  1, None, None,   False, 128),
         (128,  1, None, None,   False, 128),
         (129,  1, 256,  None,   False, 128),
         (300,  1, 256,  None,   False, 128),
         (128,  2, None, None,   False, 128),
         (128,  1, None, RAISED, False, 128),
         (128,  1, None, None,   True,  128)]
IDS = ["1", "63", "64", "65", "127", "128", "129_wave256", "300_wave256", "128_two_passes", "128_sky_tiles", "128_wide"]
_oracle = {}


def oracle_render(orc, xml, kind, frames, passes, camera):
    """(accumulator, counters) of the oracle's render: computed once per case, shared by the plain and the statistics context, never written to"""
    key = (xml, kind, frames, passes, camera)
    if key not in _oracle:
        o, _ = orc.load_scene(scene_path(xml), kind, ASSETS)
        o.renderer_init(W, H); o.set_params(5, passes)
        if camera: o.set_camera_state(*camera)
        o.render(frames, 8)
        acc = o.accumulator(); acc.setflags(write=False)
        _oracle[key] = (acc, o.counters())
    return _oracle[key]


def pool_render(crt, xml, kind, frames, passes, camera, stats):
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    ctx = crt.Context(W, H, collect_stats=stats, max_frames_per_launch=4096)
    hs.upload(ctx)
    if camera: ctx.set_camera_state(*camera)
    ctx.render(1, frames, passes)
    out = ctx.accumulator(), ctx.counters(), ctx.timing(), ctx.tile_classes(), ctx.pool_lds(frames)
    ctx.close()
    return out


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("frames,passes,wave,camera,wide,slots", CASES, ids=IDS)
@pytest.mark.parametrize("xml,kind", SCENES, ids=["cube", "tlas"])
def test_pool_job_equals_oracle(crt, orc, monkeypatch, xml, kind, frames, passes, wave, camera, wide, slots, stats):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")
    if wave: monkeypatch.setenv("CRT_POOL_WAVE_FRAMES", str(wave))
    if wide: monkeypatch.setenv("CRT_DEBUG_NO_REF16", "1")
    want, wc = oracle_render(orc, xml, kind, frames, passes, camera)

    def check(what):
        acc, cnt, tm, cls, lds = pool_render(crt, xml, kind, frames, passes, camera, stats)
        assert tm["render_launches"] == tm["pool_launches"] == 1, (what, tm)
        assert crt.lib().crt_pool_streams(frames) == slots and lds[2] == (32 if wide else 16), what
        assert np.array_equal(acc, want), "%s: accumulator differs from the oracle's in %d of %d values" % (what, int((acc != want).sum()), acc.size)
        if stats: assert cnt == wc, what
        else: assert cnt["rays"] == wc["rays"] and cnt["primary"] == wc["primary"], what
        return cls

    cls = check("table on")
    if camera:
        print("tiles by class:", np.bincount(cls, minlength=8).tolist())
        assert (cls == crt.TILE_SKY).any() and (cls != crt.TILE_SKY).any()          # sky tiles next to tiles whose rays are queued three ways
        monkeypatch.setenv("CRT_DEBUG_NO_TILE_CLASS", "1")
        check("table off")
