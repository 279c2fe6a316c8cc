#!/usr/bin/env python3
"""Cost of the Whitted renderer's traversal inspection and metrics (crt_whitted_tick_inspect) against what exists without it, at 1280 x 720:
bunny_scene.xml through the BVH, the KD-tree and the grid, and tlas_scene.xml through the two-level BVH.  Per configuration, in ONE process, every variant warmed
up and the variants alternated call by call (so drift hits all of them alike), each figure the median of --reps calls timed by a host clock around the
synchronous call (screen pixels read back in every variant, as crt_whitted_tick's callers do):
    whitted_tick        crt_whitted_tick                                                        (the baseline of modes 1 / 2, and of mode 0 "reported only")
    tick_plus_query     crt_whitted_tick, then crt_find_nearest_device over the same W*H primary rays already on the device, then the stream's completion:
                        what a caller can compose today to get the counts next to the shaded image  (the baseline of mode 0)
    inspect_0 / _1 / _2 crt_whitted_tick_inspect with screen pixels and metrics
With a library that lacks crt_whitted_tick_inspect (CRT_LIB_PATH pointing at a build of the parent commit) only the first two are measured: that run gives
the baselines and their run-to-run spread (min, max and quartiles are kept next to every median).  Writes profiles/whitted_inspect.json (or --out).
    python tools/whitted_inspect_bench.py [--reps 25] [--out profiles/whitted_inspect.json] [--label new]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from query_latency import REPO, ASSETS, load_crt, unit   # noqa: E402


def primary_rays(crt, W, H):
    """the default Camera's primary rays of the pixel grid (camera.h:14-30), row-major, as crt_ray records"""
    aspect = np.float32(W) / np.float32(H)
    cam = np.array([0, 0, -2], np.float32); tl = np.array([-aspect, 1, 0], np.float32); tr = np.array([aspect, 1, 0], np.float32); bl = np.array([-aspect, -1, 0], np.float32)
    ys, xs = np.mgrid[0:H, 0:W]
    u = (xs.ravel().astype(np.float32) * np.float32(1.0 / W))[:, None]; v = (ys.ravel().astype(np.float32) * np.float32(1.0 / H))[:, None]
    P = tl + u * (tr - tl) + v * (bl - tl)
    r = np.zeros(W * H, crt.RAY_DTYPE)
    r["O"] = cam; r["D"] = unit(P - cam)
    return r


def stats(ms):
    a = np.sort(np.asarray(ms))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), q1_ms=float(np.percentile(a, 25)), q3_ms=float(np.percentile(a, 75)), calls=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "whitted_inspect.json"))
    ap.add_argument("--label", default="new")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20 calls per figure")
    import torch
    if not torch.cuda.is_available():
        sys.exit("whitted_inspect_bench: no GPU")
    crt = load_crt()
    L = crt.lib()
    have = hasattr(L, "crt_whitted_tick_inspect")
    W, H = 1280, 720
    px = np.empty((H, W), np.uint32)
    res = dict(label=a.label, library=os.path.basename(crt.LIB_PATH), has_inspect=have, width=W, height=H, reps=a.reps, configs={})
    rays = torch.from_numpy(primary_rays(crt, W, H).view(np.float32).reshape(-1, 7).copy()).to(torch.device("cuda", 0))
    for name, xml, kind, accel in (("bunny_bvh", "bunny_scene.xml", 0, 0), ("bunny_kd", "bunny_scene.xml", 0, 1), ("bunny_grid", "bunny_scene.xml", 0, 2), ("tlas_bvh", "tlas_scene.xml", 1, 0)):
        hs = crt.HostScene(os.path.join(ASSETS, "scenes", xml), kind, ASSETS)
        ctx = crt.Context(W, H)
        hs.upload(ctx)
        if accel:
            hs.build_alt(accel); hs.upload_alt(ctx, accel); ctx.set_render_accel(accel)

        def tick():
            ctx._ck(L.crt_whitted_tick(ctx.h, px.ctypes.data_as(C.c_void_p)))

        def tick_plus_query():
            tick()
            ctx.find_nearest_device(rays, accel=accel)
            torch.cuda.synchronize()

        variants = [("whitted_tick", tick), ("tick_plus_query", tick_plus_query)]
        if have:
            m = crt.WhittedMetricsS()
            for mode in (0, 1, 2):
                variants.append(("inspect_%d" % mode, lambda mode=mode: ctx._ck(L.crt_whitted_tick_inspect(ctx.h, mode, 0, 0, px.ctypes.data_as(C.c_void_p), None, None, C.byref(m)))))
        for _, fn in variants:                     # every shape warmed up (first-use allocations, code objects)
            for _ in range(3):
                fn()
        ms = {n: [] for n, _ in variants}
        for _ in range(a.reps):                    # alternated
            for n, fn in variants:
                t0 = time.perf_counter(); fn(); ms[n].append((time.perf_counter() - t0) * 1e3)
        res["configs"][name] = {n: stats(v) for n, v in ms.items()}
        print(name, {n: round(s["median_ms"], 3) for n, s in res["configs"][name].items()}, flush=True)
        ctx.close(); hs.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
