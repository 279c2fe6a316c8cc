"""How the host splits a job's tile ranks between its pool launch and its sky launch (abi.cpp sky_to_tail / job_order / plan_job / plan_pool_waves, through
crt_debug_sky_split: no GPU needed).  The kTileSky tiles are the tail of every order, before and after the costs are known, in the relative order they had; the
block table's head and the pool launch's wave plan cover exactly the ranks in front of that tail; and a wave table, which the kernel searches over every rank up
to the end of the order, keeps every wavefront of its long part in front of the tail."""
import ctypes as C

import numpy as np
import pytest

S = 128
SKY = 7


def split(crt, cost, cls, windows=64, frames=4096, pool_ticks=0.0, sky_ticks=0.0):
    f = crt.lib().crt_debug_sky_split
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double] + [C.c_void_p] * 7
    n = len(cls)
    cls = np.ascontiguousarray(cls, np.uint8)
    c = np.ascontiguousarray(cost, np.uint32) if cost is not None else None
    order = np.zeros(n, np.uint32); tab = np.zeros(2 * n, np.uint32)
    sky_first, head, ranks, blocks, long_frames = (C.c_uint32(0) for _ in range(5))
    rc = f(c.ctypes.data if c is not None else None, cls.ctypes.data, n, windows, frames, pool_ticks, sky_ticks, order.ctypes.data, C.addressof(sky_first), C.addressof(head),
           C.addressof(ranks), tab.ctypes.data, C.addressof(blocks), C.addressof(long_frames))
    assert rc >= 0
    return dict(sky=rc, order=order, sky_first=sky_first.value, head=head.value, ranks=ranks.value, tab=tab.reshape(n, 2), blocks=blocks.value, long_frames=long_frames.value)


def image(rng, n, sky_share):
    """classes and costs of an image: a few expensive tiles, a body, and sky tiles — which a measuring job with a sky launch leaves at cost 0"""
    cls = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6], np.uint8), n)
    cls[rng.random(n) < sky_share] = SKY
    cost = np.where(rng.random(n) < 0.1, rng.uniform(1e6, 3.5e6, n), rng.uniform(1e5, 1e6, n)).astype(np.uint32)
    cost[cls == SKY] = 0
    return cls, cost


@pytest.mark.parametrize("n,sky_share", [(60, 0.3), (3600, 0.45), (3600, 0.0), (97, 1.0)])
def test_sky_tiles_are_the_tail_before_the_costs_are_known(crt, n, sky_share):
    cls, _ = image(np.random.default_rng(n), n, sky_share)
    r = split(crt, None, cls)
    sky = np.flatnonzero(cls == SKY); rest = np.flatnonzero(cls != SKY)
    assert r["sky"] == len(sky) and r["sky_first"] == n - len(sky)
    assert np.array_equal(r["order"][:r["sky_first"]], rest) and np.array_equal(r["order"][r["sky_first"]:], sky)      # both parts in the order they had
    assert r["head"] == r["ranks"] == r["blocks"] == 0                                                                 # nothing is planned without costs


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("n,windows,sky_share", [(3600, 64, 0.45), (3600, 64, 0.0), (3600, 20, 0.45), (60, 3, 0.3), (8160, 64, 0.2)])
def test_the_plan_covers_exactly_the_ranks_in_front_of_the_tail(crt, n, windows, sky_share, seed):
    rng = np.random.default_rng(1000 * seed + n + windows)
    cls, cost = image(rng, n, sky_share)
    if seed == 3: cost[cls == SKY] = rng.uniform(2e4, 1e5, int((cls == SKY).sum())).astype(np.uint32)      # costs measured without a sky launch: the tail is still the class's
    frames = 64 * windows
    r = split(crt, cost, cls, windows, frames, pool_ticks=float(cost.sum()) / 4096.0, sky_ticks=2000.0)
    order, k = r["order"], r["sky_first"]
    assert sorted(order.tolist()) == list(range(n))
    assert r["sky"] == int((cls == SKY).sum()) == n - k
    assert (cls[order[:k]] != SKY).all() and (cls[order[k:]] == SKY).all()
    # most expensive first in front of the tail, ties in tile order; the tail in the order the same sort gives it
    for part in (order[:k], order[k:]):
        c = cost[part].astype(np.int64)
        assert (np.diff(c) <= 0).all() and all(a < b for a, b, same in zip(part[:-1], part[1:], np.diff(c) == 0) if same)
    # the head goes to the block table, the wave plan covers the rest of the ranks in front of the tail: together exactly those
    assert r["head"] < k and r["head"] + r["ranks"] == k
    if r["blocks"]:
        tab = r["tab"][:n - r["head"]]                         # one entry per rank from the head to the END of the order: the kernel's search range
        wf, first = tab[:r["ranks"], 1].astype(np.int64), tab[:r["ranks"], 0].astype(np.int64)
        assert r["long_frames"] % (8 * S) == 0 and 0 < r["long_frames"] <= frames
        assert (wf % S == 0).all() and (r["long_frames"] % wf == 0).all() and (wf > S).any()
        assert first[0] == 0 and np.array_equal(np.diff(first), (r["long_frames"] // wf)[:-1]) and first[-1] + r["long_frames"] // wf[-1] == r["blocks"]
        assert (tab[r["ranks"]:, 0] == r["blocks"]).all()      # the tail's entries lie behind the long part's last wavefront: the search never lands on a sky rank


def test_a_plan_of_this_size_lengthens_wavefronts(crt):
    """(the case the table checks above need: 64 windows of a 1080p image with 20 % sky — the ranks in front of the tail keep the launch above the planner's size guard)"""
    cls, cost = image(np.random.default_rng(5), 8160, 0.2)
    r = split(crt, cost, cls, 64, 4096, pool_ticks=float(cost.sum()) / 4096.0)
    assert r["blocks"] > 0 and r["sky"] > 1000


def test_an_image_of_sky_tiles_only_has_no_plan(crt):
    cls = np.full(12, SKY, np.uint8)
    r = split(crt, np.zeros(12, np.uint32), cls, 64, 4096)
    assert r["sky"] == 12 and r["sky_first"] == 0 and r["head"] == r["ranks"] == r["blocks"] == 0
    assert np.array_equal(r["order"], np.arange(12))
