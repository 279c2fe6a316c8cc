#!/usr/bin/env python3
"""Cost of rebuilding the binned-SAH BVH for moved vertices that live on the GPU, two ways, on the wobbled bunny FileScene and on one BLAS of bunny14_scene.xml loaded as
a two-level scene (the method of tools/kdtree_device_cost.py):
  (a) host route (what the library had before crt_build_bvh_device), its three parts timed one by one: `copy_ms` positions -> host, `host_build_ms`
      crt_host_bvh_build over them, `upload_ms` crt_host_scene_upload of the rebuilt scene (which waits for every reader and sends the textures again) + a synchronise
  (b) device route: crt_build_bvh_device on a stream, then a synchronise, wall time; beside it `stream_ms`, the span of HIP events the library records on the stream
      from the first launch to the last kernel (it includes the per-level host round trips in between), `waits` / `wait_ms`, the number of those host waits and their
      wall time together, and `read_back_ms`, the wall time of reading the new pair and leaf sections back into the host mirror (crt_debug_bvh_build_ms)
The two routes alternate step by step on contexts of their own; medians over the timed steps after a warm-up, with the 10th / 90th percentiles.  Also, per scene:
crt_whitted_tick_inspect's average traversal steps per primary ray that hit, after crt_refit_device alone and after the rebuild, for the same deformation.
Usage: python tools/bvh_device_cost.py [--steps 30] [--warmup 3] [--out profiles/bvh_device.json]"""
import argparse, ctypes, importlib.util, json, os, sys, time
os.environ.setdefault("CRT_ENABLE_DEBUG_HOOKS", "1")      # the library reads its diagnostic environment switches only for processes that opt in
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("cpu_ray_tracer_amd", os.path.join(REPO, "cpu-ray-tracer_amd", "__init__.py"))
crt = importlib.util.module_from_spec(spec); spec.loader.exec_module(crt)
A = os.path.join(REPO, "assets")
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30); ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bvh_device.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
med = lambda v: float(sorted(v)[len(v) // 2])
pct = lambda v: [float(np.percentile(v, 10)), float(np.percentile(v, 90))]


def positions(b):
    t = b["tris"]
    return np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1).astype(np.float32)


def wobble(p, amount):
    return (p.astype(np.float64) + amount * np.sin(3.0 * p[..., [1, 2, 0]].astype(np.float64))).astype(np.float32)


def steps_per_hit(ctx):
    _, m = ctx.whitted_tick_inspect(crt.INSPECT_TRAVERSAL)
    return m["totalTraversal"] / max(m["rayHitCount"], 1), m


def measure(xml, kind, bvh):
    path = os.path.join(A, "scenes", xml)
    ha, hb = crt.HostScene(path, kind, A), crt.HostScene(path, kind, A)
    ca, cb = crt.Context(256, 160), crt.Context(256, 160)
    ha.upload(ca); hb.upload(cb)
    p0 = positions(hb.bvh(bvh))
    frames = [torch.from_numpy(wobble(p0, 0.15 * (k + 1) / 4)).to(dev) for k in range(4)]        # the last one is the tests' wobble
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    cols = {k: [] for k in ("copy_ms", "host_build_ms", "upload_ms", "host_route_ms", "device_route_ms", "stream_ms", "wait_ms", "read_back_ms")}
    ms = ctypes.c_float(); wms = ctypes.c_double(); rms = ctypes.c_double(); waits = ctypes.c_uint32(); levels = ctypes.c_uint32()
    for f in range(args.warmup + args.steps):
        t = frames[f % 4]
        t0 = time.perf_counter()
        p = t.cpu().numpy()
        t1 = time.perf_counter()
        crt.host_bvh_build(p)
        t2 = time.perf_counter()
        ha.move_and_rebuild(bvh, p)                                        # (the scene's own arrays for the upload: the same build again, not counted)
        t3 = time.perf_counter()
        ha.upload(ca); ca.sync()
        t4 = time.perf_counter()
        cb.build_bvh_device(bvh, t, stream=st, root_box=False); st.synchronize()
        t5 = time.perf_counter()
        cb._ck(cb.L.crt_debug_bvh_build_ms(cb.h, ctypes.byref(ms), ctypes.byref(wms), ctypes.byref(waits), ctypes.byref(levels), ctypes.byref(rms)))
        if f >= args.warmup:
            row = dict(copy_ms=(t1 - t0) * 1e3, host_build_ms=(t2 - t1) * 1e3, upload_ms=(t4 - t3) * 1e3, device_route_ms=(t5 - t4) * 1e3, stream_ms=ms.value, wait_ms=wms.value,
                       read_back_ms=rms.value)
            row["host_route_ms"] = row["copy_ms"] + row["host_build_ms"] + row["upload_ms"]
            for k, v in row.items():
                cols[k].append(v)
    g = cb.get_bvh(bvh)                                                     # (of the last frame)
    # traversal steps for the tests' deformation: refit alone against the rebuild, on a fresh context each
    last = frames[3]
    hc = crt.HostScene(path, kind, A); cc = crt.Context(256, 160); hc.upload(cc)
    if kind == 1:
        T = torch.from_numpy(np.stack([hc.blas_transform(i)[0] for i in range(hc.bvh_count())])).to(dev)
    rest, _ = steps_per_hit(cc)
    cc.refit_device(bvh, last)
    if kind == 1:
        cc.update_transforms_device(T)
    refit, m_refit = steps_per_hit(cc)
    cc.build_bvh_device(bvh, last)
    if kind == 1:
        cc.update_transforms_device(T)
    rebuilt, m_rebuilt = steps_per_hit(cc)
    r = dict(scene=xml, kind=kind, bvh=bvh, triangles=int(len(p0)), nodesUsed=g["nodesUsed"], height=g["height"], levels=int(levels.value), waits=int(waits.value), steps=args.steps,
             warmup=args.warmup, traversal_steps_per_hit=dict(rest_pose=rest, refit_only=refit, rebuilt=rebuilt, hits_refit=m_refit["rayHitCount"], hits_rebuilt=m_rebuilt["rayHitCount"]))
    for k, v in cols.items():
        r[k] = med(v); r[k + "_p10_p90"] = pct(v)
    return r


results = [measure("bunny_scene.xml", 0, 0), measure("bunny14_scene.xml", 1, 0)]
out = dict(tool="tools/bvh_device_cost.py", device=torch.cuda.get_device_name(0), results=results)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
for r in results:
    tr = r["traversal_steps_per_hit"]
    print("%s BVH %d (%d triangles, %d nodes, %d levels): host route %.3f ms (copy %.3f, build %.3f, upload %.3f) | device route %.3f ms (on the stream %.3f ms, %d host waits %.3f ms, "
          "read-back %.3f ms) | traversal steps per hit: rest %.2f, refit only %.2f, rebuilt %.2f"
          % (r["scene"], r["bvh"], r["triangles"], r["nodesUsed"], r["levels"], r["host_route_ms"], r["copy_ms"], r["host_build_ms"], r["upload_ms"], r["device_route_ms"], r["stream_ms"],
             r["waits"], r["wait_ms"], r["read_back_ms"], tr["rest_pose"], tr["refit_only"], tr["rebuilt"]))
