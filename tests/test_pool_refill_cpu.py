"""The pool launch's frames per wavefront (abi.cpp pool_wave_plan, through crt_debug_pool_wave_plan: no GPU needed).  Tile costs are given in dispatch order (most
expensive first).  The plan has a long part — the frames [0, longFrames) of every tile, in ranges of 128 2^k frames chosen per tile — and a short part, the rest of the
frames in ranges of S = 128 dispatched behind it.  Checked for random cost vectors and frame counts: a tile's ranges cover its frames exactly once and in order, all but
the last are whole groups of S frames, nothing is lengthened without costs or below the size guard, and no lengthened wavefront is predicted to end after the job's
makespan aim."""
import ctypes as C

import numpy as np
import pytest

S, RESIDENT = 128, 4096


def plan(crt, cost, frames, per_cost=1.0 / 4096, start=0.0, resident=RESIDENT, safety=0.0, guard=0.0, share=0.0, n=None):
    L = crt.lib()
    f = L.crt_debug_pool_wave_plan
    f.restype = C.c_longlong
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n = len(cost) if cost is not None else n
    wf = np.zeros(n, np.uint32); st = np.zeros(n, np.float64); aim = C.c_double(0); lf = C.c_uint32(0)
    c = np.ascontiguousarray(cost, np.uint32) if cost is not None else None
    waves = f(c.ctypes.data if c is not None else None, n, frames, per_cost, start, resident, safety, guard, share, wf.ctypes.data, C.addressof(lf), st.ctypes.data, C.addressof(aim))
    return int(waves), wf, int(lf.value), st, aim.value


def terms(crt):
    L = crt.lib()
    out = (C.c_double * 5)()
    L.crt_debug_pool_wave_terms.restype = None
    L.crt_debug_pool_wave_terms(out)
    return dict(poolLong=out[0], load=out[1], safety=out[2], guard=out[3], share=out[4])


def ranges(frames, wf, long_frames):
    """the kernel's block -> frame range mapping of one tile: the long part's wavefront g owns [g wf, (g + 1) wf) below long_frames, the short part's wavefront g
    [long_frames + g S, min(frames, long_frames + (g + 1) S))"""
    assert long_frames % wf == 0 and long_frames <= frames
    return [(g * wf, (g + 1) * wf) for g in range(long_frames // wf)] + [(long_frames + g * S, min(frames, long_frames + (g + 1) * S)) for g in range((frames - long_frames + S - 1) // S)]


def random_costs(rng, n):
    """a few expensive tiles, a body, a cheap tail (sky): 100 MHz ticks per 64 streams, most expensive first"""
    c = np.concatenate([rng.uniform(1e6, 3.5e6, n // 10), rng.uniform(1e5, 1e6, n - n // 10 - n // 4), rng.uniform(2e4, 1e5, n // 4)])
    return np.sort(c.astype(np.uint32))[::-1]


@pytest.mark.parametrize("seed", range(6))
def test_ranges_cover_every_frame_once_and_respect_the_aim(crt, seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(300, 4000))
    frames = int(rng.integers(129, 4097))
    cost = random_costs(rng, n)
    tm = terms(crt)
    safety = float(rng.choice([0.0, 1.0, 2.0])); guard = float(rng.choice([0.0, 1.0, 3.0])); share = float(rng.choice([0.0, 0.5, 1.0]))
    waves, wf, lf, st, aim = plan(crt, cost, frames, safety=safety, guard=guard, share=share)
    sh = share if share > 0 else tm["share"]
    assert lf in (0, int(frames * sh) // 1024 * 1024)
    windows = (frames + 63) // 64
    total = 0
    for r in range(n):
        assert wf[r] in (S, 2 * S, 4 * S, 8 * S)
        rs = ranges(frames, int(wf[r]), lf)
        total += len(rs)
        assert rs[0][0] == 0 and rs[-1][1] == frames and all(a[1] == b[0] for a, b in zip(rs, rs[1:]))      # [0, frames) once, in order
        assert all((b - a) % S == 0 for a, b in rs[:-1]) and 0 < rs[-1][1] - rs[-1][0] <= max(S, wf[r])     # whole groups of S but for the last
        if wf[r] > S:
            assert lf > 0
            end = st[r] + tm["poolLong"] * tm["load"] * float(cost[r]) * float(wf[r]) / 128.0
            assert end <= aim * (1 + 1e-12), (r, end, aim)
    assert total == waves
    # the expected start is the machine time of the long part of the tiles dispatched before, the aim the machine time of everything
    mt = cost.astype(np.float64) / 4096
    if int(frames * sh) >= 1024:
        assert np.allclose(st, np.concatenate([[0.0], np.cumsum(mt * (int(frames * sh) // 1024 * 16))[:-1]]), rtol=1e-9) and np.isclose(aim, windows * mt.sum(), rtol=1e-9)
    else: assert lf == 0
    g = guard if guard > 0 else tm["guard"]
    if (wf > S).any(): assert waves >= g * RESIDENT


def test_unknown_costs_leave_every_range_at_S(crt):
    for frames in (129, 512, 1000, 4096):
        waves, wf, lf, st, aim = plan(crt, None, frames, n=3600)
        assert (wf == S).all() and lf == 0 and waves == 3600 * ((frames + S - 1) // S)


def test_launch_below_the_size_guard_is_left_as_it_is(crt):
    rng = np.random.default_rng(7)
    N = 8000
    cost = random_costs(rng, N)
    g = terms(crt)["guard"]
    # N tiles x ceil(frames / 128) wavefronts: below guard x resident nothing is lengthened; above it the tiles that can afford it are, and the launch still keeps that many
    n = int(g * RESIDENT / 12) - 1                       # tiles of a 1536-frame job just below the guard
    assert n <= N
    waves, wf, lf, _, _ = plan(crt, cost[:n], 1536)
    assert n * 12 < g * RESIDENT and (wf == S).all() and lf == 0 and waves == n * 12
    waves, wf, lf, _, _ = plan(crt, cost, 1536)
    assert (wf > S).any() and lf == 1024 and g * RESIDENT <= waves < N * 12
    waves, wf, lf, _, _ = plan(crt, cost, 4096)
    assert (wf > S).any() and lf == int(4096 * terms(crt)["share"]) // 1024 * 1024 and g * RESIDENT <= waves < N * 32
    # a stricter guard than the launch can keep -> nothing
    waves, wf, lf, _, _ = plan(crt, cost, 4096, guard=N * 32 / RESIDENT + 1)
    assert (wf == S).all() and lf == 0 and waves == N * 32
    # a job of fewer than 1024 frames within the long part's share has no long part
    waves, wf, lf, _, _ = plan(crt, cost, 1280, share=0.5)
    assert (wf == S).all() and lf == 0 and waves == N * 10
    waves, wf, lf, _, _ = plan(crt, cost, 1023)
    assert (wf == S).all() and lf == 0 and waves == N * 8


def test_frames_that_fit_the_slots_are_never_lengthened(crt):
    cost = np.full(8000, 1000, np.uint32)
    for frames in (1, 64, 65, 128):
        waves, wf, lf, _, _ = plan(crt, cost, frames)
        assert (wf == (64 if frames <= 64 else S)).all() and lf == 0 and waves == 8000
