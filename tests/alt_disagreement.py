"""Rays of assets/scenes/tlas_scene.xml on which the two-level KD-tree / grid (TLASKDTree over BLASKDTree, TLASGrid over BLASGrid) does not return the TLAS-BVH's
nearest hit: the committed set tests/golden/alt_disagreement_rays.npz (written by tests/golden/make_alt_disagreement_rays.py with the CPU oracle alone) and the
comparison that defines it.  These are the rays that run what differs from the BVH path: BLASKDTree's rule-1 early return, the two `double` comparisons that skip
a child, a hit a float step outside the TLAS box that the BVH has culled.  Not collected by pytest (no test_ prefix)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "alt_disagreement_rays.npz")
HIT_FIELDS = ("t", "u", "v", "objIdx", "triIdx")
CLASSES = ("primary", "surface", "inside")                                # how a path produces the ray: from the camera, kEPS off a surface, inside the dielectric
MIN_RAYS, MIN_PER_SIGN = 100, 20


def load(kind):
    """O, D [n, 3] float32, inside [n] int32, seeds [n] uint32 (never 0), cls [n] uint8 (index into CLASSES) of kind "kd" / "grid" """
    z = np.load(FIXTURE)
    return tuple(z["%s_%s" % (kind, f)] for f in ("O", "D", "inside", "seeds", "cls"))


def scene_pair(orc, xml, assets, kind):
    """(the oracle's TLAS-BVH scene, the same scene walked through the two-level structure `kind`)"""
    b, _ = orc.load_scene(xml, 1, assets)
    a, _ = orc.load_scene(xml, 1, assets)
    orc.set_blas_accel(a, orc.blas_accels(a, kind))
    return b, a


def differ(bvh_hits, alt_hits):
    """(mask of rays whose records differ in any of t, u, v, objIdx, triIdx as bits; mask `structure loses the BVH's hit` (t larger); mask `finds a hit the BVH culled` (t smaller))"""
    d = np.zeros(len(bvh_hits), bool)
    for f in HIT_FIELDS:
        d |= bvh_hits[f].view(np.uint32) != alt_hits[f].view(np.uint32)
    return d, d & (alt_hits["t"] > bvh_hits["t"]), d & (alt_hits["t"] < bvh_hits["t"])


def check(kind, O, D, inside, seeds, cls, bvh_hits, alt_hits):
    """the conditions the committed set must meet; returns the counts {name: n}"""
    d, lost, found = differ(bvh_hits, alt_hits)
    assert d.all(), (kind, "rays that no longer disagree", np.flatnonzero(~d)[:8].tolist())
    assert len(O) >= MIN_RAYS and (D != 0).all() and np.isfinite(O).all() and np.isfinite(D).all() and (seeds != 0).all()
    assert set(np.unique(inside)) <= {0, 1} and np.array_equal(inside != 0, cls == CLASSES.index("inside"))
    counts = dict(rays=len(O), lost=int(lost.sum()), found=int(found.sum()), same_t=int((d & ~lost & ~found).sum()))
    counts.update({c: int((cls == i).sum()) for i, c in enumerate(CLASSES)})
    assert all(counts[c] >= 10 for c in CLASSES), counts                  # every way a path produces a ray is present
    if kind == "kd":
        assert counts["lost"] >= MIN_PER_SIGN and counts["found"] >= MIN_PER_SIGN, counts
    return counts
