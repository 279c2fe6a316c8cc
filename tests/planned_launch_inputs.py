"""Tile costs that make the planner give a SMALL job a wave table (tests/test_planned_launch_cpu.py holds every recipe to the library's own planner without a GPU;
tests/test_gpu_planned_launch.py installs them with Context.set_job_costs and holds the launch they plan to the oracle).

What the planner sees (abi.cpp plan_job, plan_pool_waves, pool_wave_plan): the cost of every owned tile, P = the machine time of one window of the image under the
pool, and the machine time of a window of the sky launch.  The cost of one unit is P / sum(cost), so only the costs' shares of their sum and the ratio c / P count:
rank r of the pool launch gets the largest k <= 3 with  start(r) + 2.4 c_r 2^k <= aim,  aim = windows x P x (the planned ranks' share) + the sky launch's time,
start(r) = longFrames / 64 x P x (the share of the ranks in front).  A tile with 2.4 c > aim leaves the pool launch for the block table (the head), so a recipe
without a head keeps its most expensive tile below aim / 2.4, and one whose first rank stays at 128 frames keeps it above aim / 4.8.
The launch's size guard (12 x 4096 wavefronts) is what no small job passes: the tests set CRT_POOL_REFILL_GUARD to a value just above 0.

A recipe is a function of the context's own tile classes (one byte per owned tile) and returns (cost, P, sky window ticks); `plan` asks the library what it
makes of them and `replay` restates render_pool_kernel's block -> (rank, frame range) search over the returned table."""
import ctypes as C

import numpy as np

S = 128                         # frames per wavefront of the short part (and of a launch without a plan)
SKY = 7                         # layout.h kTileSky
FLOOR_ONLY = 5                  # kTileNoLight | kTileNoTree
NO_TREE = 4
GUARD = "1e-9"                  # CRT_POOL_REFILL_GUARD
P = 5000.0                      # pool window ticks of every recipe
SPAN_NO_SHORT_PART = 2000.0     # recipe (a)'s span for a job that is all long part: its last ranks start when the aim is nearly used up, and afford 1024 frames only when they cost next to nothing
SKY_TICKS = 200.0               # ... and the sky launch's ticks per window (looked at only when the job has a sky launch)
# the tile classes (kTileNo* bits) of the images the GPU tests render, default camera: (scene, W, H) -> one byte per tile.  test_gpu_planned_launch.py asserts
# that a context reports these; test_planned_launch_cpu.py checks the recipes on them.
CLASSES = {
    ("bunny_scene.xml", 64, 48): [7, 3, 3, 7, 5, 1, 1, 5, 5, 1, 1, 5],                       # 2 sky, 4 floor-only, 6 the mesh can show in: the smallest such image
    ("bunny_scene.xml", 96, 64): [7] * 6 + [5, 1, 1, 1, 5, 5] * 3,
    ("cube_scene.xml", 32, 32): [1, 1, 1, 1],
    ("tlas_scene.xml", 64, 48): [7] * 4 + [1] * 8,
    ("bunny4_scene.xml", 96, 64): [3] * 6 + [1] * 18,                                         # (no sky tile: the job has no sky launch)
}
ENV = {"CRT_RENDER_KERNEL": "pool_always", "CRT_PLAN_NO_TRIAL": "1", "CRT_POOL_REFILL_GUARD": GUARD}


def split(crt, cost, cls, frames, pool_ticks, sky_ticks=0.0):
    """crt_debug_sky_split for a job of `frames` frames"""
    f = crt.lib().crt_debug_sky_split
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double] + [C.c_void_p] * 7
    n = len(cls)
    cls = np.ascontiguousarray(cls, np.uint8)
    c = np.ascontiguousarray(cost, np.uint32)
    assert len(c) == n
    order = np.zeros(n, np.uint32); tab = np.zeros(2 * n, np.uint32)
    sky_first, head, ranks, blocks, long_frames = (C.c_uint32(0) for _ in range(5))
    rc = f(c.ctypes.data, cls.ctypes.data, n, (frames + 63) // 64, frames, float(pool_ticks), float(sky_ticks), order.ctypes.data, C.addressof(sky_first), C.addressof(head),
           C.addressof(ranks), tab.ctypes.data, C.addressof(blocks), C.addressof(long_frames))
    assert rc >= 0
    return dict(sky=rc, order=order, sky_first=sky_first.value, head=head.value, ranks=ranks.value, tab=tab.reshape(n, 2), blocks=blocks.value, long_frames=long_frames.value)


def plan(crt, cls, cost, frames, pool_ticks, sky_ticks=0.0):
    """The job the library plans for these costs, as install_job_plan decides: the split crt_debug_sky_split reports — or, when that plan has a head and a sky tail,
    the plan of the same costs without a sky launch (the sky tiles stay in the pool launch, at the end of its order).
    Returns n, order, head, rank_end (the pool launch renders the ranks [head, rank_end)), sky (ranks of the sky launch), blocks, long_frames, tab (one row per
    rank from head to n: first block, frames per wavefront), wf (frames per wavefront of the ranks [head, rank_end); S where there is no table), and the launch
    shape the context must report: long_waves, split_launches, sky_launches."""
    cls = np.ascontiguousarray(cls, np.uint8); n = len(cls)
    r = split(crt, cost, cls, frames, pool_ticks, sky_ticks)
    sky = r["sky"]
    if r["head"] and sky:
        again = split(crt, cost, np.zeros(n, np.uint8), frames, pool_ticks, 0.0)
        # (that entry orders the tiles by cost alone; the context's order keeps the sky tiles last — the same order when those are the cheapest, ties in tile order)
        assert np.array_equal(again["order"], r["order"]), "a recipe with a head gives its sky tiles the lowest costs"
        r, sky = again, 0
    head, rank_end = r["head"], n - sky
    assert r["ranks"] == rank_end - head
    tab = r["tab"][:n - head] if r["blocks"] else np.zeros((0, 2), np.uint32)
    wf = tab[:rank_end - head, 1].astype(np.int64) if r["blocks"] else np.full(rank_end - head, S, np.int64)
    long_waves = int((r["long_frames"] // wf[wf > S]).sum())
    return dict(n=n, order=r["order"], head=head, rank_end=rank_end, sky=sky, blocks=r["blocks"], long_frames=r["long_frames"], tab=tab, wf=wf,
                long_waves=long_waves, split_launches=1 if head else 0, sky_launches=1 if sky else 0)


def head_table(crt, cost, frames, pool_ticks):
    """crt_debug_plan_job: the block table of the plan's head as (tile, first frame, lanes, window) rows, for costs whose order needs no sky tail (plan())"""
    f = crt.lib().crt_debug_plan_job
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_double, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    c = np.ascontiguousarray(cost, np.uint32); n = len(c)
    cap = n * _windows(frames) * 64
    table = np.zeros(cap, np.uint32); order = np.zeros(n, np.uint32); head = C.c_uint32(0)
    nb = f(c.ctypes.data, n, _windows(frames), frames, 1, float(pool_ticks), table.ctypes.data, cap, C.addressof(head), order.ctypes.data)
    assert nb >= 0
    d = table[:nb]
    return head.value, np.stack([d & 0xffff, (d >> 16) & 63, 1 << ((d >> 22) & 7), d >> 25], axis=1)


def lengths(p):
    """{frames per wavefront: ranks} of a plan's pool launch"""
    v, c = np.unique(p["wf"], return_counts=True)
    return dict(zip(v.tolist(), c.tolist()))


def replay(p, frames):
    """render_pool_kernel's block -> (rank, frame range) mapping (render_pool.hip, the search over waveTab and the short part behind it) for every block of the
    launch's grid, as crt_launch_render_pool sizes it.  Asserts that every block below `blocks` lands on one (rank, group) of the long part, no two on the same, and
    that every frame of every rank the launch renders is owned exactly once across both parts, none of any other rank.  Returns the number of wavefronts that own
    frames."""
    n, head, rank_end, blocks, long_frames, tab = p["n"], p["head"], p["rank_end"], p["blocks"], p["long_frames"], p["tab"]
    assert blocks > 0 and 0 < long_frames <= frames and len(tab) == n - head
    groups = (frames - long_frames + S - 1) // S
    grid = blocks + (rank_end - head) * groups
    owned = np.zeros((n, frames), np.int32)
    seen, waves = set(), 0
    for b in range(grid):
        if b < blocks:
            lo, hi = 0, n - head
            while hi - lo > 1:
                mid = (lo + hi) >> 1
                if tab[mid, 0] <= b: lo = mid
                else: hi = mid
            rank0, grp, wf, first, limit = lo, b - int(tab[lo, 0]), int(tab[lo, 1]), 0, long_frames
            assert rank0 + head < rank_end and wf % S == 0 and long_frames % wf == 0 and grp < long_frames // wf, (b, rank0, grp, wf)
            assert (rank0, grp) not in seen
            seen.add((rank0, grp))
        else:
            rank0, grp = divmod(b - blocks, groups)
            wf, first, limit = S, long_frames, frames
        rank = rank0 + head
        if rank >= n: continue
        frame0 = first + grp * wf
        if frame0 >= limit: continue
        own = min(limit - frame0, wf)
        owned[rank, frame0:frame0 + own] += 1
        waves += 1
    assert len(seen) == blocks
    assert (owned[head:rank_end] == 1).all() and (owned[:head] == 0).all() and (owned[rank_end:] == 0).all()
    return waves


# ---------------------------------------------------------------------------------------------------------------------------------------------
# recipes: cost per owned tile from the tile classes.  `ranked` lists the tiles that are not sky in the dispatch order the recipe wants; the sky tiles cost 0,
# as a measuring job with a sky launch leaves them.

def _ranked(cls, reverse):
    idx = np.flatnonzero(np.asarray(cls) != SKY)
    return idx[::-1] if reverse else idx


def _costs(cls, ranked, values):
    cost = np.zeros(len(cls), np.uint32)
    cost[ranked] = np.asarray(values, np.float64).astype(np.uint32)
    assert (np.diff(cost[ranked].astype(np.int64)) <= 0).all() and (cost[ranked] > 0).all()      # (equal costs dispatch in tile order: only `ranked` ascending may hold any)
    return cost


def _windows(frames): return (frames + 63) // 64


def _fall(m, frames, span=80.0):
    """m costs falling geometrically from 0.305 x the aim (between aim / 4.8 and aim / 2.4: the first rank stays at 128 frames, no tile leaves the pool) to 1 / span of that"""
    return 0.305 * _windows(frames) * P * (1.0 / span) ** (np.arange(m) / max(1, m - 1))


def mixed(cls, frames, reverse=False, span=80.0):
    """(a) + (b): a geometric fall over the tiles that are not sky, in tile order (reverse: against it).  All four lengths; the sky tiles, if any, are the sky launch's."""
    ranked = _ranked(cls, reverse)
    return _costs(cls, ranked, _fall(len(ranked), frames, span)), P, SKY_TICKS


def head_and_table(cls, frames, outliers=(4.2, 3.2), span=2000.0):
    """(c): two outliers far above the makespan aim — plan_job gives them narrow wavefronts through the block table — in front of recipe (a)'s fall for the rest.
    The sky tiles keep cost 0: the lowest, so the order without a sky launch is the order with one."""
    ranked = _ranked(cls, False)
    m = len(ranked) - len(outliers)
    assert m >= 4
    return _costs(cls, ranked, [o * _windows(frames) * P for o in outliers] + list(_fall(m, frames, span))), P, SKY_TICKS


def uniform_long(cls, frames):
    """(d): every tile that is not sky at the same small cost: every rank affords 1024 frames per wavefront"""
    ranked = _ranked(cls, False)
    return _costs(cls, ranked, np.full(len(ranked), P / 100.0)), P, SKY_TICKS


def last_rank_only(cls, frames):
    """(e): every rank too expensive for 256 frames but the last, which costs next to nothing"""
    ranked = _ranked(cls, False)
    v = np.full(len(ranked), 0.315 * _windows(frames) * P); v[-1] = 50.0
    return _costs(cls, ranked, v), P, SKY_TICKS
