"""render_pool_kernel's slot refill: a wavefront that owns more frames of its tile than it has stream slots hands a slot whose stream has rendered its 256
pixels the range's next frame.  Which slot renders a (tile, frame) stream changes nothing about its samples, so every case is bit-for-bit the oracle's image
(or the image of the launch with 128 frames per wavefront, which never refills).  The range length is forced with CRT_POOL_WAVE_FRAMES except in the last
case, where the planner chooses it per tile from the measured tile costs (abi.cpp pool_wave_plan)."""
import ctypes as C

import numpy as np
import pytest

from conftest import ASSETS, scene_path

pytestmark = pytest.mark.gpu


def long_waves(ctx):
    ctx.L.crt_debug_pool_long_waves.restype = C.c_int
    return ctx.L.crt_debug_pool_long_waves(ctx.h)


# bunny: one refilled range of 256 frames, then a partial range of 44 (statistics build: every counter)
# two-level scene, passes 2: the range (1024) is longer than the job — 72 refills, then the population runs out
# cube: four generations of 128 in the range of 512, then 188 frames with 60 refills
@pytest.mark.parametrize("xml,kind,W,H,frames,passes,wave,stats,want_long", [("bunny_scene.xml", 0, 64, 48, 300, 1, 256, True, 12), ("tlas_scene.xml", 1, 64, 48, 200, 2, 1024, True, 12),
                                                                            ("cube_scene.xml", 0, 32, 32, 700, 1, 512, False, 8)])
def test_refilled_wavefronts_match_the_oracle(crt, orc, monkeypatch, xml, kind, W, H, frames, passes, wave, stats, want_long):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always"); monkeypatch.setenv("CRT_POOL_WAVE_FRAMES", str(wave))
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    ctx = crt.Context(W, H, collect_stats=stats, max_frames_per_launch=4096)
    hs.upload(ctx)
    ctx.render(1, frames, passes)
    acc = ctx.accumulator()
    tm = ctx.timing()
    assert tm["render_launches"] == 1 and tm["pool_launches"] == 1
    assert long_waves(ctx) == want_long                                       # tiles x wavefronts that own more than 128 frames
    o, _ = orc.load_scene(scene_path(xml), kind, ASSETS)
    o.renderer_init(W, H)
    o.set_params(5, passes)
    o.render(frames, 4)
    assert np.array_equal(acc, o.accumulator())
    got, want = ctx.counters(), o.counters()
    if stats: assert got == want
    else: assert got["rays"] == want["rays"]
    px, energy = ctx.resolve_screen(1.0 / (1 + frames * passes))
    assert np.array_equal(px, o.screen()) and np.float32(energy) == np.float32(o.energy())


def test_refill_with_tile_ownership_and_frame_batches(crt, orc, monkeypatch):
    """two interleaved tile owners, launches of 96 frames (S = 128 slots, 96 streams, nothing to refill with) under a forced range of 256: summed == oracle"""
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always"); monkeypatch.setenv("CRT_POOL_WAVE_FRAMES", "256")
    W, H, frames = 96, 64, 200
    hs = crt.HostScene(scene_path("bunny_scene.xml"), 0, ASSETS)
    tiles = (W // 16) * (H // 16)
    total = np.zeros((H, W, 4), np.float32)
    for r in range(2):
        first, stride, count = crt.tile_partition(r, 2, tiles)
        ctx = crt.Context(W, H, tile_first=first, tile_stride=stride, tile_count=count, max_frames_per_launch=96)
        hs.upload(ctx)
        ctx.render(1, frames, 1)
        total += ctx.accumulator()
        ctx.close()
    o, _ = orc.load_scene(scene_path("bunny_scene.xml"), 0, ASSETS)
    o.renderer_init(W, H)
    o.render(frames, 4)
    assert np.array_equal(total, o.accumulator())


@pytest.mark.parametrize("split", [None, "3"])
def test_ranges_of_512_frames_against_128(crt, monkeypatch, split):
    """bunny 320x192, 512 frames: one refilled wavefront per tile against four that never refill; with CRT_SPLIT_FORCE the second job of each context is a split one
    (three tiles through the block table, the pool launch starts at rank 3)"""
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always"); monkeypatch.setenv("CRT_PLAN_NO_TRIAL", "1")
    if split: monkeypatch.setenv("CRT_SPLIT_FORCE", split)
    W, H, frames = 320, 192, 512
    hs = crt.HostScene(scene_path("bunny_scene.xml"), 0, ASSETS)
    out = {}
    for wave in (512, 128):
        monkeypatch.setenv("CRT_POOL_WAVE_FRAMES", str(wave))
        ctx = crt.Context(W, H, max_frames_per_launch=4096)
        hs.upload(ctx)
        jobs = 2 if split else 1
        for i in range(jobs):
            ctx.clear(); ctx.reset_counters(); ctx.render(1, frames, 1); ctx.sync()
        tm = ctx.timing()
        assert tm["pool_launches"] == jobs and tm["split_launches"] == (1 if split else 0)
        assert long_waves(ctx) == ((240 - (3 if split else 0)) if wave == 512 else 0)
        out[wave] = (ctx.accumulator(), ctx.counters()["rays"])
        ctx.close()
    assert np.array_equal(out[512][0], out[128][0]) and out[512][1] == out[128][1]


def test_planner_lengthens_wavefronts_of_a_large_job(crt, monkeypatch):
    """no hook for the range length: 1280x720 bunny, an 8-window job (measures the tile costs) then a 64-window job on one context — the planner gives the tiles that
    can afford it longer ranges; same accumulator as the same sequence with 128 frames per wavefront everywhere"""
    hs = crt.HostScene(scene_path("bunny_scene.xml"), 0, ASSETS)
    out = {}
    for wave in (None, "128"):
        if wave: monkeypatch.setenv("CRT_POOL_WAVE_FRAMES", wave)
        ctx = crt.Context(1280, 720, max_frames_per_launch=4096)
        hs.upload(ctx)
        ctx.reserve(64 * 64, 1)
        ctx.render(1, 8 * 64, 1); ctx.sync()
        ctx.render(1 + 8 * 64, 64 * 64, 1); ctx.sync()
        n = long_waves(ctx)
        print("wavefronts of the 64-window job that own more than 128 frames:", n)
        if wave is None: assert n > 0
        else: assert n == 0
        out[wave] = (ctx.accumulator(), ctx.counters()["rays"])
        ctx.close()
    assert np.array_equal(out[None][0], out["128"][0]) and out[None][1] == out["128"][1]
