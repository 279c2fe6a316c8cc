#!/usr/bin/env python3
"""Cost of rebuilding the KD-tree for moved vertices that live on the GPU, two ways, on the bunny FileScene and on every BLAS of tlas_scene.xml (the scenes and the
method of tools/grid_device_cost.py):
  (a) host route (what the library had before crt_build_kdtree_device): positions -> host copy -> crt_host_scene_bvh_move_and_refit -> crt_host_scene_build_alt(KDTREE)
      -> crt_host_scene_upload_alt(KDTREE) (which drains the context), wall time
  (b) device route: crt_build_kdtree_device on a stream, then a synchronise, wall time; beside it `stream_ms`, the span of HIP events the library records on the
      stream around the build (first launch to last: it includes the host round trips in between), `waits` and `wait_ms`, the number of the call's host waits (one
      per level) and their wall time together (crt_debug_kdtree_build_ms)
The two routes alternate step by step on contexts of their own; medians over the timed steps after a warm-up.  A two-level scene has NO host route once a BLAS has
deformed: crt_upload_blas_accel requires the tree's root box to equal the BVH's root box, and after Refit that box is not the true bounds (the reference skips node 1),
so the upload is refused; the tool reports the device route alone there (`host_route_ms` null), which rebuilds one BLAS and carries the others over.
Usage: python tools/kdtree_device_cost.py [--steps 50] [--warmup 5] [--out profiles/kdtree_device.json]"""
import argparse, ctypes, importlib.util, json, os, sys, time
os.environ.setdefault("CRT_ENABLE_DEBUG_HOOKS", "1")      # the library reads its diagnostic environment switches only for processes that opt in
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("cpu_ray_tracer_amd", os.path.join(REPO, "cpu-ray-tracer_amd", "__init__.py"))
crt = importlib.util.module_from_spec(spec); spec.loader.exec_module(crt)
A = os.path.join(REPO, "assets")
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50); ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kdtree_device.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
med = lambda v: float(sorted(v)[len(v) // 2])
KD = crt.ACCEL_KDTREE


def positions(b):
    t = b["tris"]
    return np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1).astype(np.float32)


def measure(xml, kind, bvh):
    path = os.path.join(A, "scenes", xml)
    ha, hb = crt.HostScene(path, kind, A), crt.HostScene(path, kind, A)
    ca, cb = crt.Context(256, 160), crt.Context(256, 160)
    for h, c in ((ha, ca), (hb, cb)):
        h.build_alt(KD); h.upload(c); h.upload_alt(c, KD)
    p0 = positions(hb.bvh(bvh))
    frames = [torch.from_numpy((p0.astype(np.float64) + 0.02 * (k + 1) * np.sin(3.0 * p0[..., [1, 2, 0]].astype(np.float64))).astype(np.float32)).to(dev) for k in range(4)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    host, device, stream_ms, wait_ms = [], [], [], []
    ms = ctypes.c_float(); wms = ctypes.c_double(); waits = ctypes.c_uint32(); levels = ctypes.c_uint32()
    for f in range(args.warmup + args.steps):
        t = frames[f % 4]
        t0 = time.perf_counter()
        if kind == 0:
            ha.move_and_refit(bvh, t.cpu().numpy()); ha.build_alt(KD); ha.upload_alt(ca, KD); ca.sync()
        t1 = time.perf_counter()
        cb.build_kdtree_device(bvh, t, stream=st); st.synchronize()
        t2 = time.perf_counter()
        cb._ck(cb.L.crt_debug_kdtree_build_ms(cb.h, ctypes.byref(ms), ctypes.byref(wms), ctypes.byref(waits), ctypes.byref(levels)))
        if f >= args.warmup:
            host.append((t1 - t0) * 1e3); device.append((t2 - t1) * 1e3); stream_ms.append(ms.value); wait_ms.append(wms.value)
    g = cb.get_kdtree(bvh)                                                  # (of the last frame)
    pct = lambda v: [float(np.percentile(v, 10)), float(np.percentile(v, 90))]
    return dict(scene=xml, bvh=bvh, triangles=int(len(p0)), nodes=int(len(g["nodes"])), references=int(len(g["refs"])), levels=int(levels.value), waits=int(waits.value), steps=args.steps, warmup=args.warmup,
                host_route_ms=med(host) if kind == 0 else None, device_route_ms=med(device), stream_ms=med(stream_ms), wait_ms=med(wait_ms),
                host_route_ms_p10_p90=pct(host) if kind == 0 else None, device_route_ms_p10_p90=pct(device), stream_ms_p10_p90=pct(stream_ms), wait_ms_p10_p90=pct(wait_ms))


results = [measure("bunny_scene.xml", 0, 0)]
n = crt.HostScene(os.path.join(A, "scenes", "tlas_scene.xml"), 1, A).bvh_count()
results += [measure("tlas_scene.xml", 1, i) for i in range(n)]
out = dict(tool="tools/kdtree_device_cost.py", device=torch.cuda.get_device_name(0), results=results)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
for r in results:
    print("%s BVH %d (%d triangles, %d nodes, %d references, %d levels): host route %s ms | device route %.3f ms (on the stream %.3f ms, %d host waits %.3f ms)"
          % (r["scene"], r["bvh"], r["triangles"], r["nodes"], r["references"], r["levels"], "%.3f" % r["host_route_ms"] if r["host_route_ms"] is not None else "none",
             r["device_route_ms"], r["stream_ms"], r["waits"], r["wait_ms"]))
