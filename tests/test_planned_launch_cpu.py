"""The cost recipes of tests/planned_launch_inputs.py held to the library's own planner (crt_debug_sky_split, crt_debug_plan_job, crt_debug_pool_wave_plan: no GPU
needed), on the tile classes of the images tests/test_gpu_planned_launch.py renders (recorded there, asserted there against the context's).  Each recipe has the
plan it was made for as a precondition here — the GPU tests install the same costs and hold the launch to the oracle; a recipe that stopped producing its plan would
leave them checking a plain launch.  And for every plan: render_pool_kernel's block search, restated in Python (planned_launch_inputs.replay), maps every block of
the table to one (rank, group) and gives every (rank, frame) of the launch to exactly one wavefront across the long and the short part, sky entries included."""
import numpy as np
import pytest

import planned_launch_inputs as I
from planned_launch_inputs import S, SKY

BUNNY_SMALL, BUNNY, CUBE, TLAS, BUNNY4 = (("bunny_scene.xml", 64, 48), ("bunny_scene.xml", 96, 64), ("cube_scene.xml", 32, 32), ("tlas_scene.xml", 64, 48),
                                          ("bunny4_scene.xml", 96, 64))
ALL = [BUNNY_SMALL, BUNNY, CUBE, TLAS, BUNNY4]


@pytest.fixture(autouse=True)
def guard(monkeypatch):
    for k in ("CRT_SKY_PLACEMENT", "CRT_POOL_REFILL_SAFETY", "CRT_POOL_REFILL_SHARE", "CRT_POOL_REFILL_OFF", "CRT_POOL_WAVE_FRAMES", "CRT_SPLIT_FORCE", "CRT_SPLIT_OFF"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CRT_POOL_REFILL_GUARD", I.GUARD)


def cls_of(key): return np.array(I.CLASSES[key], np.uint8)


def planned(crt, key, recipe, frames, **kw):
    cls = cls_of(key)
    cost, pool_ticks, sky_ticks = recipe(cls, frames, **kw)
    p = I.plan(crt, cls, cost, frames, pool_ticks, sky_ticks)
    assert p["blocks"] > 0 and p["long_waves"] > 0, "no wave table"
    assert I.replay(p, frames) == p["blocks"] + (p["rank_end"] - p["head"]) * ((frames - p["long_frames"] + S - 1) // S)
    return cls, cost, p


def test_the_guard_is_what_keeps_a_small_job_plain(crt, monkeypatch):
    """the same costs without the hook: nothing is lengthened (12 x 4096 wavefronts are out of a small image's reach)"""
    monkeypatch.delenv("CRT_POOL_REFILL_GUARD")
    cls = cls_of(BUNNY)
    cost, pool_ticks, sky_ticks = I.mixed(cls, 1189)
    p = I.plan(crt, cls, cost, 1189, pool_ticks, sky_ticks)
    assert p["blocks"] == 0 and p["long_waves"] == 0 and (p["wf"] == S).all()


def test_recorded_images_have_the_tiles_the_cases_need():
    for key in (BUNNY_SMALL, BUNNY):
        cls = cls_of(key)
        assert (cls == SKY).sum() >= 2 and (cls == I.FLOOR_ONLY).sum() >= 2 and ((cls & I.NO_TREE) == 0).sum() >= 4, key
        assert len(cls) == (key[1] // 16) * (key[2] // 16)
    assert len(cls_of(CUBE)) == 4 and not (cls_of(CUBE) == SKY).any()


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("key,placement", [(BUNNY_SMALL, "behind"), (BUNNY_SMALL, "ahead"), (BUNNY, "behind"), (BUNNY, "ahead"), (TLAS, "behind"), (BUNNY4, "behind")])      # (the GPU cases)
def test_mixed_lengths_with_a_sky_tail(crt, monkeypatch, key, reverse, placement):
    """(a) + (b): all four lengths, two ranks or more of each, and >= 2 sky ranks behind them whose table entries say `blocks`"""
    if placement == "ahead": monkeypatch.setenv("CRT_SKY_PLACEMENT", "ahead")
    cls, cost, p = planned(crt, key, I.mixed, 1189, reverse=reverse)
    n_sky = int((cls == SKY).sum())
    assert p["head"] == 0 and p["long_frames"] == 1024
    got = I.lengths(p)
    assert sorted(got) == [S, 2 * S, 4 * S, 8 * S] and min(got.values()) >= 2, got
    assert p["sky"] == n_sky and p["sky_launches"] == (1 if n_sky else 0)
    if key in (BUNNY_SMALL, BUNNY): assert n_sky >= 2
    assert len(p["tab"]) == p["n"] and (p["tab"][p["rank_end"]:, 0] == p["blocks"]).all() and (p["tab"][p["rank_end"]:, 1] == S).all()
    # the dispatch order: the recipe's ranking in front, the sky tiles behind it in tile order
    ranked = np.flatnonzero(cls != SKY)
    assert np.array_equal(p["order"][:p["rank_end"]], ranked[::-1] if reverse else ranked) and np.array_equal(p["order"][p["rank_end"]:], np.flatnonzero(cls == SKY))
    if reverse: assert not np.array_equal(p["order"], np.arange(p["n"]))


def test_sky_placement_changes_the_plan(crt, monkeypatch):
    """the sky launch's time is the pool launch's tail (behind) or its start (ahead): case 1's two runs are two plans"""
    _, _, behind = planned(crt, BUNNY_SMALL, I.mixed, 1189)
    monkeypatch.setenv("CRT_SKY_PLACEMENT", "ahead")
    _, _, ahead = planned(crt, BUNNY_SMALL, I.mixed, 1189)
    assert not np.array_equal(behind["wf"], ahead["wf"])


def test_four_tiles_four_lengths(crt):
    cls, cost, p = planned(crt, CUBE, I.mixed, 1189)
    assert p["head"] == 0 and p["sky"] == 0 and p["wf"].tolist() == [S, 2 * S, 4 * S, 8 * S]


@pytest.mark.parametrize("frames", [1024, 2048])
@pytest.mark.parametrize("key", [BUNNY_SMALL, BUNNY])
def test_jobs_without_a_short_part(crt, key, frames):
    """frames == longFrames: the launch is the table's blocks alone; at 2048 frames one table holds ranks of two blocks (1024 frames each) and of sixteen"""
    cls, cost, p = planned(crt, key, I.mixed, frames, span=I.SPAN_NO_SHORT_PART)
    assert p["head"] == 0 and p["long_frames"] == frames and p["sky"] >= 2
    got = I.lengths(p)
    assert S in got and 8 * S in got, got
    if frames == 2048: assert set((frames // p["wf"]).tolist()) >= {2, 16}


@pytest.mark.parametrize("key", [BUNNY_SMALL, BUNNY])
def test_head_and_wave_table_in_one_job(crt, key):
    """(c): plan_job's own head, with narrow wavefronts and a partial last window; the job then keeps no sky launch and its sky tiles are the pool launch's last ranks"""
    frames = 1189
    cls, cost, p = planned(crt, key, I.head_and_table, frames)
    n_sky = int((cls == SKY).sum())
    assert n_sky >= 2 and p["head"] == 2 and p["sky"] == 0 and p["sky_launches"] == 0 and p["split_launches"] == 1 and p["rank_end"] == p["n"]
    assert (cls[p["order"][p["n"] - n_sky:]] == SKY).all() and (p["wf"][-n_sky:] > S).all()
    assert len(p["tab"]) == p["n"] - 2
    assert len(set(p["wf"][:-n_sky].tolist())) >= 2                                       # mixed lengths among the tiles that are not sky
    head, table = I.head_table(crt, cost, frames, I.P)
    assert head == 2 and len(table) > 0 and set(table[:, 0].tolist()) == set(p["order"][:2].tolist())
    assert (table[:, 2] < 64).any()                                                         # narrow wavefronts
    last = table[table[:, 3] == (frames - 1) // 64]
    assert len(last) and (last[:, 1] < frames - (frames - 1) // 64 * 64).all() and len(last) < len(table[table[:, 3] == 0])   # the partial last window


@pytest.mark.parametrize("key", ALL)
def test_every_rank_the_same_long_range(crt, key):
    cls, cost, p = planned(crt, key, I.uniform_long, 1189)
    assert p["head"] == 0 and (p["wf"] == 8 * S).all() and p["long_waves"] == p["rank_end"]


@pytest.mark.parametrize("key", ALL)
def test_only_the_last_pool_rank_is_lengthened(crt, key):
    cls, cost, p = planned(crt, key, I.last_rank_only, 1189)
    assert p["head"] == 0 and (p["wf"][:-1] == S).all() and p["wf"][-1] > S and p["long_waves"] == 1024 // p["wf"][-1]


def test_strided_owners_plan_their_own_tiles(crt):
    """case 9: two interleaved owners of the 96 x 64 bunny, each with a recipe over its own tiles"""
    cls = cls_of(BUNNY)
    for r in range(2):
        first, stride, count = crt.tile_partition(r, 2, len(cls))
        own = cls[first::stride][:count]
        cost, pool_ticks, sky_ticks = I.mixed(own, 1189, reverse=bool(r))
        p = I.plan(crt, own, cost, 1189, pool_ticks, sky_ticks)
        assert p["long_waves"] > 0 and len(I.lengths(p)) >= 3 and p["sky"] >= 2 and p["head"] == 0
        I.replay(p, 1189)
