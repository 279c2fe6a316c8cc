#!/usr/bin/env python3
"""TLASFileScene's three accelerator variants on tlas_scene.xml (TLAS_USE_BVH, TLAS_USE_KDTree, TLAS_USE_Grid: crt_upload_blas_accel) on the same rays:
    find_nearest   crt_find_nearest_device per 2^20 rays (camera rays of the default Camera plus random bounces off their hits): wall ms from the call to the
                   stream's completion, and the GPU time between torch (HIP) events around the call
    is_occluded    crt_is_occluded_device on the same rays, t = distance to the light centre: the same two figures
    render         one crt_render of 64 frames x 1 pass at 1280 x 720 through each (crt_set_render_accel), wall ms to crt_sync
Also how many records of the KD-tree / grid differ from the TLAS-BVH record (t, u, v, objIdx, triIdx) on these rays.
Medians over --reps repetitions after two warm-ups (the render: --render-reps).  Writes profiles/query_tlas_alt.json (or --out).
    python tools/query_tlas_alt.py [--reps 10] [--render-reps 3] [--out profiles/query_tlas_alt.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from query_latency import REPO, ASSETS, load_crt, unit   # noqa: E402


def rays(crt, ctx, n, rng):
    """n / 2 camera rays of the default camera, n / 2 uniformly random directions from their mesh / floor hits (BVH path)"""
    h = n // 2
    O1 = np.tile(np.array([0.0, 0.0, -2.0], np.float32), (h, 1))
    P = np.stack([rng.uniform(-2.5, 2.5, h), rng.uniform(-1.2, 1.0, h), np.full(h, 2.0)], 1).astype(np.float32)
    D1 = unit(P - O1)
    hb = ctx.find_nearest(O1, D1)
    ok = hb["objIdx"] >= 1
    I = O1 + np.where(ok, hb["t"], 1.0)[:, None] * D1
    R = unit(rng.normal(size=(h, 3)))
    O2 = (I + R * np.float32(0.001)).astype(np.float32)
    return np.concatenate([O1, O2]), np.concatenate([D1, R])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--render-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "query_tlas_alt.json"))
    a = ap.parse_args()
    import torch
    crt = load_crt()
    xml = os.path.join(ASSETS, "scenes", "tlas_scene.xml")
    hs = crt.HostScene(xml, 1, ASSETS)
    t0 = time.perf_counter(); hs.build_alt(crt.ACCEL_KDTREE); t1 = time.perf_counter(); hs.build_alt(crt.ACCEL_GRID); t2 = time.perf_counter()
    ctx = crt.Context(64, 64)
    hs.upload(ctx)
    t3 = time.perf_counter(); hs.upload_alt(ctx, crt.ACCEL_KDTREE); t4 = time.perf_counter(); hs.upload_alt(ctx, crt.ACCEL_GRID); t5 = time.perf_counter()
    n = 1 << 20
    O, D = rays(crt, ctx, n, np.random.default_rng(7))
    light = np.array([0.0, 3.0, 1.5], np.float32)
    t = np.linalg.norm(light - O, axis=1).astype(np.float32)
    r = np.zeros(n, crt.RAY_DTYPE); r["O"], r["D"] = O, D
    s = np.zeros(n, crt.SHADOW_RAY_DTYPE); s["O"], s["D"], s["t"] = O, D, t
    dev = torch.device("cuda", 0)
    rr = torch.from_numpy(r.view(np.float32).reshape(-1, 7).copy()).to(dev)
    sr = torch.from_numpy(s.view(np.float32).reshape(-1, 7).copy()).to(dev)
    res = dict(scene="tlas_scene.xml", rays=n, form="persistent waves, one step of each kind per trip (tlas_alt.hip)", reps=a.reps, host_build_ms=dict(kd=(t1 - t0) * 1e3, grid=(t2 - t1) * 1e3),
               upload_ms=dict(kd=(t4 - t3) * 1e3, grid=(t5 - t4) * 1e3), queries={}, render_1280x720_64spp_ms={})

    def timed(fn):
        wall, gpu = [], []
        for k in range(a.reps + 2):
            st = torch.cuda.current_stream(); e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            w0 = time.perf_counter(); e0.record(st); fn(); e1.record(st); st.synchronize(); w1 = time.perf_counter()
            if k >= 2:
                wall.append((w1 - w0) * 1e3); gpu.append(e0.elapsed_time(e1))
        return dict(wall_ms=float(np.median(wall)), gpu_ms=float(np.median(gpu)))

    ref = None
    for name, accel in (("bvh", 0), ("kd", crt.ACCEL_KDTREE), ("grid", crt.ACCEL_GRID)):
        q = dict(find_nearest=timed(lambda: ctx.find_nearest_device(rr, accel=accel)), is_occluded=timed(lambda: ctx.is_occluded_device(sr, accel=accel)))
        rec = ctx.find_nearest_device(rr, accel=accel)[:, :5].contiguous().view(torch.int32).cpu().numpy()   # t, u, v, objIdx, triIdx as bits
        obj = rec[:, 3]
        q["mesh_hits"] = int((obj >= 2).sum())
        if ref is None:
            ref = rec
        q["objIdx_differs_from_bvh"] = int((obj != ref[:, 3]).sum())
        q["hit_differs_from_bvh"] = int((rec != ref).any(axis=1).sum())       # some of t, u, v, objIdx, triIdx not bit-equal to the TLAS-BVH record
        q["hit_differs_with_zero_direction_component"] = int(((rec != ref).any(axis=1) & (D == 0).any(axis=1)).sum())
        res["queries"][name] = q
        print(name, q, flush=True)
    ctx.close()
    W, H = 1280, 720
    rc = crt.Context(W, H)
    hs.upload(rc); hs.upload_alt(rc, crt.ACCEL_KDTREE); hs.upload_alt(rc, crt.ACCEL_GRID)
    for name, accel in (("bvh", 0), ("kd", crt.ACCEL_KDTREE), ("grid", crt.ACCEL_GRID)):
        rc.set_render_accel(accel)
        ms = []
        for k in range(a.render_reps + 1):
            rc.clear(); rc.sync()
            w0 = time.perf_counter(); rc.render(1, 64, 1); rc.sync(); w1 = time.perf_counter()
            if k >= 1:
                ms.append((w1 - w0) * 1e3)
        res["render_1280x720_64spp_ms"][name] = float(np.median(ms))
        print(name, "render", res["render_1280x720_64spp_ms"][name], flush=True)
    rc.close(); hs.close()
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
