#!/usr/bin/env python3
"""Generates tests/golden/alt_disagreement_rays.npz with the CPU oracle alone (no reference tree, no GPU): rays of assets/scenes/tlas_scene.xml whose record through
the two-level KD-tree / grid (orc.set_blas_accel) differs from the TLAS-BVH record in any of t, u, v, objIdx, triIdx.  tests/alt_disagreement.py states the
conditions; tests/test_tlas_alt_cpu.py re-derives them from the oracle on every run, so the set cannot go stale silently.

Candidates are drawn the way paths produce rays, from the default camera at 1024 x 640:
  primary   GetPrimaryRay through random sub-pixel positions, and through the positions that project floor points under / around each instance (where instance
            geometry touches the floor, the BVH's TLAS box test culls a hit a float step before the floor's that the other structures still find);
  surface   from the hit point of such a ray, kEPS along a random direction (what a diffuse bounce, a reflection or a shadow ray starts from);
  inside    from where a ray enters the dielectric instance (the torii gate), kEPS along a direction near the ray's, with inside = 1.
Random search is enough: the rate is about 5 per 2^20 for uniform primary rays but about 4 per 1000 for rays that leave the torii gate's surface.
Per kind, class and sign (loses the BVH's hit / finds a hit the BVH culled) at most QUOTA rays are kept."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "oracle")); sys.path.insert(0, os.path.join(REPO, "tests"))
import alt_disagreement as ad      # noqa: E402
import orc                         # noqa: E402

ASSETS = os.path.join(REPO, "assets")
XML = os.path.join(ASSETS, "scenes", "tlas_scene.xml")
W, H = 1024, 640
KEPS = np.float32(0.001)
QUOTA = {"kd": 30, "grid": 60}                                            # per (class, sign): lost / found / same t (the grid only ever finds culled hits)
ROUNDS, CHUNK = 24, 1 << 19
DIELECTRIC_OBJ = 3                                                         # objIdx of the torii gate (material 1: refractivity 1)


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def pixels_of(points, aspect):
    """screen positions whose default-camera primary ray (camera at (0, 0, -2), screen plane z = 0, template/camera.h:14-30) passes through `points`"""
    s = 2.0 / (points[:, 2] + 2.0)
    px, py = points[:, 0] * s, points[:, 1] * s
    xy = np.stack([(px + aspect) / (2 * aspect) * W, (1 - py) / 2 * H], 1)
    return xy[(xy[:, 0] >= 0) & (xy[:, 0] < W) & (xy[:, 1] >= 0) & (xy[:, 1] < H)].astype(np.float32)


def candidates(b, rng):
    """one round: (O, D, inside, cls) of all three classes"""
    xy = [np.stack([rng.uniform(0, W, CHUNK // 4), rng.uniform(0, H, CHUNK // 4)], 1).astype(np.float32)]
    for i in range(b.bvh_count()):
        _, _, lo, hi = b.blas_transform(i)
        k = CHUNK // 4
        y = np.where(rng.random(k) < 0.8, -1.0, rng.uniform(-1.0, hi[1], k))          # mostly on the floor plane y = -1, the rest anywhere in the instance's bounds
        pts = np.stack([rng.uniform(lo[0] - 0.05, hi[0] + 0.05, k), y, rng.uniform(lo[2] - 0.05, hi[2] + 0.05, k)], 1)
        xy.append(pixels_of(pts, W / H))
    Op, Dp = b.primary_rays(np.concatenate(xy))
    h = b.find_nearest(Op, Dp)
    hit = h["objIdx"] >= 1
    I = (Op[hit] + h["t"][hit][:, None] * Dp[hit]).astype(np.float32)
    R = unit(rng.normal(size=(len(I), 3)))
    Os, Ds = (I + R * KEPS).astype(np.float32), R
    ent = h["objIdx"] == DIELECTRIC_OBJ
    Ie = (Op[ent] + h["t"][ent][:, None] * Dp[ent]).astype(np.float32)
    reps = 8                                                               # the gate covers few pixels: several directions per entry point
    Ie = np.repeat(Ie, reps, 0); De = np.repeat(Dp[ent], reps, 0)
    T = unit(De + rng.normal(scale=0.5, size=De.shape).astype(np.float32))
    Oi, Di = (Ie + T * KEPS).astype(np.float32), T
    O = np.concatenate([Op, Os, Oi]); D = np.concatenate([Dp, Ds, Di])
    cls = np.concatenate([np.full(len(Op), 0, np.uint8), np.full(len(Os), 1, np.uint8), np.full(len(Oi), 2, np.uint8)])
    ok = (D != 0).all(axis=1) & np.isfinite(D).all(axis=1)
    return O[ok], D[ok], (cls[ok] == 2).astype(np.int32), cls[ok]


def main():
    out = {}
    for kind in ("kd", "grid"):
        b, a = ad.scene_pair(orc, XML, ASSETS, kind)
        b.renderer_init(W, H)
        rng = np.random.default_rng(20240 + len(kind))
        kept = {(c, s): [] for c in range(3) for s in range(3)}
        seen = tested = 0
        for _ in range(ROUNDS):
            O, D, inside, cls = candidates(b, rng)
            hb, ha = b.find_nearest(O, D, inside), a.find_nearest(O, D, inside)
            d, lost, found = ad.differ(hb, ha)
            sign = np.where(lost, 0, np.where(found, 1, 2))
            tested += len(O); seen += int(d.sum())
            for i in np.flatnonzero(d):
                kept[(int(cls[i]), int(sign[i]))].append((O[i], D[i], inside[i], cls[i]))
            if all(len(v) >= QUOTA[kind] for (c, s), v in kept.items() if s == 1 or (s == 0 and kind == "kd")):
                break
        pick = np.random.default_rng(5)                                    # a random QUOTA of each slot, not the first ones found
        kept = {k: [v[i] for i in sorted(pick.permutation(len(v))[:QUOTA[kind]])] for k, v in kept.items()}
        rows = [r for v in kept.values() for r in v]
        perm = np.random.default_rng(7).permutation(len(rows))
        O = np.array([rows[i][0] for i in perm], np.float32); D = np.array([rows[i][1] for i in perm], np.float32)
        inside = np.array([rows[i][2] for i in perm], np.int32); cls = np.array([rows[i][3] for i in perm], np.uint8)
        seeds = (np.random.default_rng(11).integers(1, 1 << 32, len(O), dtype=np.uint64)).astype(np.uint32)
        counts = ad.check(kind, O, D, inside, seeds, cls, b.find_nearest(O, D, inside), a.find_nearest(O, D, inside))
        print("%s: %d candidates, %d disagree (%.1f per 2^20); kept %s" % (kind, tested, seen, seen / tested * (1 << 20), counts))
        print("   per class and sign (lost, found, same t): %s" % {ad.CLASSES[c]: [len(kept[(c, s)]) for s in range(3)] for c in range(3)})
        for f, v in (("O", O), ("D", D), ("inside", inside), ("seeds", seeds), ("cls", cls)):
            out["%s_%s" % (kind, f)] = v
    np.savez(ad.FIXTURE, **out)
    print("wrote %s (%d bytes)" % (os.path.relpath(ad.FIXTURE, REPO), os.path.getsize(ad.FIXTURE)))


if __name__ == "__main__":
    sys.exit(main())
