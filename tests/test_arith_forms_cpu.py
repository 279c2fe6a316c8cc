"""The short accept predicate of the slab test (dev_common.h slab_accept) against the three-compare conjunction it stands for, in numpy float32 with denormals
kept:   tmax >= tmin && tmin < tray && tmax > 0   <=>   max(tmin, dmin) <= min(tmax, pred(tray)),   dmin the smallest denormal, pred(tray) = bits - 1.
The identity holds for every non-NaN tmin / tmax and every tray whose bit pattern, as a signed integer, is >= 2 (tray_tame: a positive float above dmin, +inf
included); the kernel routes every other tray to box_exact, and the last test shows that it has to.  (The device's own evaluation of both forms, the short
quotients and the guarded sky lookup: tests/test_gpu_arith_forms.py.)"""
import ctypes as C
import itertools

import numpy as np

DMIN = np.array([1], np.uint32).view(np.float32)[0]


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def boundary_values():
    """+-0, +-denorm_min, the largest denormal, FLT_MIN, 1e-4, 1, 1e30 and 1e34 with their two neighbours, FLT_MAX, +-inf — and the negatives of all of them"""
    pos = [0x00000000, 0x00000001, 0x007fffff, 0x00800000]
    for v in (1e-4, 1.0):
        pos.append(int(np.array([v], np.float32).view(np.uint32)[0]))
    for v in (1e30, 1e34):
        b = int(np.array([v], np.float32).view(np.uint32)[0])
        pos += [b - 1, b, b + 1]
    pos += [0x7f7fffff, 0x7f800000]
    return f32(pos + [b | 0x80000000 for b in pos])


def old_form(tmin, tmax, tray):
    return (tmax >= tmin) & (tmin < tray) & (tmax > 0)


def new_form(tmin, tmax, tray):
    pred = (tray.view(np.uint32) - np.uint32(1)).view(np.float32)
    with np.errstate(invalid="ignore"):
        return np.maximum(tmin, DMIN) <= np.minimum(tmax, pred)


def tray_tame(tray):
    return tray.view(np.int32) >= 2


def test_numpy_keeps_denormals():
    assert DMIN > 0 and np.float32(DMIN * np.float32(1)) == DMIN and np.maximum(np.float32(0), DMIN) == DMIN


def test_predicate_on_the_boundary_cross_product():
    v = boundary_values()
    t = np.array(list(itertools.product(v, v, v)), np.float32)
    tmin, tmax, tray = np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1]), np.ascontiguousarray(t[:, 2])
    tame = tray_tame(tray)
    assert tame.sum() > len(t) // 3 and (~tame).sum() > 0
    bad = np.flatnonzero((old_form(tmin, tmax, tray) != new_form(tmin, tmax, tray)) & tame)
    assert len(bad) == 0, "first: tmin %r tmax %r tray %r" % (tmin[bad[0]], tmax[bad[0]], tray[bad[0]])
    assert old_form(tmin, tmax, tray)[tame].sum() > 100                            # the conjunction is not vacuously false on the list


def random_triples(n, seed):
    """any non-NaN tmin / tmax, any positive non-NaN tray; in three of four triples tmax and / or tray lie within two bit patterns of tmin (|tmin| for tray)"""
    rng = np.random.default_rng(seed)
    def no_nan(b):
        return np.where((b & 0x7fffffff) > 0x7f800000, b & 0xff800000, b).astype(np.uint32)
    a = no_nan(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
    b = no_nan(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
    c = no_nan(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)) & np.uint32(0x7fffffff)
    k = np.arange(n)
    near = rng.integers(0, 5, n).astype(np.uint32) - np.uint32(2)
    b = np.where(k & 1, no_nan(a + near), b)
    near = rng.integers(0, 5, n).astype(np.uint32) - np.uint32(2)
    c = np.where(k & 2, no_nan((a & np.uint32(0x7fffffff)) + near) & np.uint32(0x7fffffff), c)
    return f32(a), f32(b), f32(c)


def test_predicate_on_random_triples():
    tmin, tmax, tray = random_triples(10 ** 7, 5)
    tame = tray_tame(tray)
    old, new = old_form(tmin, tmax, tray), new_form(tmin, tmax, tray)
    bad = np.flatnonzero((old != new) & tame)
    assert len(bad) == 0, "first: tmin %r tmax %r tray %r" % (tmin[bad[0]], tmax[bad[0]], tray[bad[0]])
    assert tame.sum() > 9 * 10 ** 6 and old[tame].sum() > 10 ** 5 and (~old[tame]).sum() > 10 ** 6


def test_the_excluded_tray_does_differ():
    """tray = denorm_min (bit pattern 1): its predecessor is +0, so a box with tmin <= 0 < tmax is refused where the conjunction accepts it — the guard is needed"""
    tray = f32([1, 1, 1])
    tmin, tmax = np.array([0.0, -1.0, -0.0], np.float32), np.array([1.0, 2.0, DMIN], np.float32)
    assert not tray_tame(tray).any()
    assert old_form(tmin, tmax, tray).all() and not new_form(tmin, tmax, tray).any()
    # and a zero tray has no predecessor of this form at all: bits - 1 is a NaN pattern
    assert np.isnan((f32([0]).view(np.uint32) - np.uint32(1)).view(np.float32)[0])


def test_library_exports_the_probe(crt):
    L = C.CDLL(crt.build())
    assert hasattr(L, "crt_debug_arith_forms")
