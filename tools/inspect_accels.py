#!/usr/bin/env python3
"""The Whitted renderer's console report ("2. WhittedStyle/renderer.cpp":164-178), side by side for every accelerator a scene can be traced through: the BVH,
the KD-tree and the grid of a FileScene; the two-level BVH, KD-tree and grid of a TLAS scene (--tlas).  One line each: primary rays with traversed > 0, total /
average / peak traversal steps, total / average / peak triangle tests of one Tick.  --dump DIR also writes the two heat maps of each ("Inspect traversal" /
"Inspect intersection", second Tick: every pixel scaled by the frame's peak) and the per-pixel counts as .npy.  Needs a GPU.
    python tools/inspect_accels.py assets/scenes/bunny_scene.xml [--tlas] [--size 1280x720] [--camera px,py,pz,tx,ty,tz] [--dump DIR]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from query_latency import ASSETS, load_crt   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("xml")
    ap.add_argument("--tlas", action="store_true", help="load the scene as a TLASFileScene")
    ap.add_argument("--size", default="1280x720")
    ap.add_argument("--camera", default=None)
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    crt = load_crt()
    if crt.device_count() < 1:
        sys.exit("inspect_accels: no GPU")
    kind = crt.SCENE_TLAS if a.tlas else crt.SCENE_FILE
    hs = crt.HostScene(a.xml, kind, ASSETS)
    ctx = crt.Context(W, H)
    hs.upload(ctx)
    if a.camera:
        c = [float(v) for v in a.camera.split(",")]
        ctx.set_camera_state(c[:3], c[3:])
    for code in (crt.ACCEL_KDTREE, crt.ACCEL_GRID):
        hs.build_alt(code); hs.upload_alt(ctx, code)
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    print("%-12s %9s %12s %9s %6s %12s %9s %6s" % ("accelerator", "hit rays", "total trav", "avg trav", "peak", "total tests", "avg tests", "peak"))
    for name, code in (("tlas-bvh" if a.tlas else "bvh", 0), ("tlas-kdtree" if a.tlas else "kdtree", crt.ACCEL_KDTREE), ("tlas-grid" if a.tlas else "grid", crt.ACCEL_GRID)):
        ctx.set_render_accel(code)
        _, m, tr, te = ctx.whitted_tick_inspect(crt.INSPECT_NONE, counts=True)
        hits = max(m["rayHitCount"], 1)
        print("%-12s %9d %12d %9.2f %6d %12d %9.2f %6d" % (name, m["rayHitCount"], m["totalTraversal"], np.float32(m["totalTraversal"]) / np.float32(hits), m["peakTraversal"],
                                                          m["totalTests"], np.float32(m["totalTests"]) / np.float32(hits), m["peakTests"]))
        if a.dump:
            for mode, tag in ((crt.INSPECT_TRAVERSAL, "traversal"), (crt.INSPECT_TESTS, "tests")):
                ctx.whitted_tick_inspect(mode, m["peakTraversal"], m["peakTests"])
                np.save(os.path.join(a.dump, "%s_%s_heat.npy" % (name, tag)), ctx.accumulator()[..., :3])
            np.save(os.path.join(a.dump, "%s_traversed.npy" % name), tr); np.save(os.path.join(a.dump, "%s_tested.npy" % name), te)
    ctx.close(); hs.close()


if __name__ == "__main__":
    main()
