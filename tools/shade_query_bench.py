#!/usr/bin/env python3
"""GPU time of the shading queries (crt_get_hit_info_device, crt_get_sky_color_device) beside crt_find_nearest_device on the same rays, in one process:
the 2^20-ray set of tools/query_latency.py on bunny_scene.xml (FileScene) and that of tools/query_tlas_alt.py on tlas_scene.xml (two-level).

A timed window is a run of back-to-back calls of one entry on a non-default torch stream between two HIP events on that stream (outputs preallocated, the C
entries called directly: no allocation inside a window; beyond 64 calls in flight the library waits for the oldest, which keeps the GPU's queue full).  The
number of calls per window is chosen per entry from a first window so that a window lasts about --window-ms (at least 16 calls): a 26 us gather is timed over
hundreds of calls, not over a fraction of a millisecond.  Per entry the median of --windows windows after two warm-up windows, the entries alternated window by
window.  Figures per call:
    gpu_ms            window time / calls
    bytes             the algorithmic bytes of the call: per record 56 B in (crt_ray + crt_hit) and 48 B out, per mesh record 64 B ShadeTri + 32 B Material
                      (+ 48 B of Instance::T in a two-level scene), one 4-byte texel per record that samples a texture (floor, textured mesh, the sky of a miss);
                      the sky query: 28 B in, 12 B out, one texel
    GBps              bytes / gpu_ms
    stream_floor_ms   104 B (hit info) / 40 B (sky) per record at 6.1 TB/s, the rate the accumulate kernel reaches on this chip; floor_ratio = gpu_ms / that
What to read them against: a gather that takes longer than the walk that produced its input (find_nearest on the same rays) has a defect.
Writes profiles/shade_query.json (or --out).
    python tools/shade_query_bench.py [--windows 10] [--window-ms 10] [--out profiles/shade_query.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from query_latency import REPO, ASSETS, load_crt, make_rays   # noqa: E402
from query_tlas_alt import rays as tlas_rays                  # noqa: E402

STREAM_RATE = 6.1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=10.0)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shade_query.json"))
    a = ap.parse_args()
    import torch
    crt = load_crt()
    dev = torch.device("cuda", 0)
    res = dict(n=a.n, windows=a.windows, window_ms_target=a.window_ms, device=torch.cuda.get_device_name(0), stream_rate_Bps=STREAM_RATE, scenes={})
    for name, xml, kind in (("bunny", "bunny_scene.xml", crt.SCENE_FILE), ("tlas", "tlas_scene.xml", crt.SCENE_TLAS)):
        hs = crt.HostScene(os.path.join(ASSETS, "scenes", xml), kind, ASSETS)
        ctx = crt.Context(64, 64)
        hs.upload(ctx)
        O, D = make_rays(crt, ctx, hs, a.n) if name == "bunny" else tlas_rays(crt, ctx, a.n, np.random.default_rng(7))
        n = len(O)
        r = np.zeros(n, crt.RAY_DTYPE); r["O"], r["D"] = O, D
        rays = torch.from_numpy(r.view(np.float32).reshape(-1, 7).copy()).to(dev)
        st = torch.cuda.Stream()
        hits = ctx.find_nearest_device(rays, stream=st)
        info = torch.empty((n, 12), dtype=torch.float32, device=dev)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        h = crt.hit_fields(hits)
        obj = h["objIdx"].cpu().numpy()
        mats = crt.hit_info_fields(ctx.get_hit_info_device(rays, hits, stream=st))["material"].cpu().numpy()
        textured_mesh = 0
        if name == "tlas":                                                # tlas_scene.xml: material 0 (the wok's, record value 2) is the textured one
            textured_mesh = int((mats == 2).sum())
        mesh, floor, miss = int((obj >= 2).sum()), int((obj == 1).sum()), int((obj == -1).sum())
        hit_bytes = n * (56 + 48) + mesh * (64 + 32 + (48 if kind == crt.SCENE_TLAS else 0)) + 4 * (floor + miss + textured_mesh)
        sky_bytes = n * (28 + 12 + 4)
        p = lambda t: C.c_void_p(t.data_ptr())
        sp, nn = C.c_void_p(st.cuda_stream), C.c_size_t(n)
        entries = {
            "find_nearest": lambda: ctx._ck(ctx.L.crt_find_nearest_device(ctx.h, 0, p(rays), p(hits), nn, sp)),
            "get_hit_info": lambda: ctx._ck(ctx.L.crt_get_hit_info_device(ctx.h, p(rays), p(hits), p(info), nn, sp)),
            "get_sky_color": lambda: ctx._ck(ctx.L.crt_get_sky_color_device(ctx.h, p(rays), p(rgb), nn, sp)),
        }

        def window(fn, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(calls):
                fn()
            e1.record(st)
            st.synchronize()
            return e0.elapsed_time(e1) / calls

        calls = {k: int(min(2048, max(16, np.ceil(a.window_ms / window(fn, 16))))) for k, fn in entries.items()}
        times = {k: [] for k in entries}
        for w in range(a.windows + 2):
            for k, fn in entries.items():
                t = window(fn, calls[k])
                if w >= 2:
                    times[k].append(t)
        out = dict(records=dict(mesh=mesh, floor=floor, miss=miss, light=int((obj == 0).sum())))
        for k, ts in times.items():
            ms = float(np.median(ts))
            e = dict(gpu_ms=ms, calls_per_window=calls[k], window_ms=ms * calls[k], min_ms=float(np.min(ts)), max_ms=float(np.max(ts)))
            if k != "find_nearest":
                b = hit_bytes if k == "get_hit_info" else sky_bytes
                floor_ms = n * (104 if k == "get_hit_info" else 40) / STREAM_RATE * 1e3
                e.update(bytes=int(b), GBps=b / (ms * 1e-3) / 1e9, stream_floor_ms=floor_ms, floor_ratio=ms / floor_ms)
            out[k] = e
        out["hit_info_over_find_nearest"] = out["get_hit_info"]["gpu_ms"] / out["find_nearest"]["gpu_ms"]
        res["scenes"][name] = out
        print(name, json.dumps(out), flush=True)
        ctx.close(); hs.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
