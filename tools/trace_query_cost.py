#!/usr/bin/env python3
"""Cost of crt_trace_device: the W x H primary rays of the context's camera (integer pixel positions) through the Whitted Renderer::Trace as a ray query, once in
row-major order and once in a fixed shuffled order, beside crt_whitted_tick at the same resolution — whitted_kernel, one thread per pixel, whose per-ray body is the
same trace_body.h.  Scenes: tlas_scene.xml (a dielectric and a half mirror: trees of very different sizes) and bunny_scene.xml (all diffuse: every tree is one
FindNearest and at most one shadow walk).  The query's time is the span of events on the stream around the bare crt_trace_device call (cursor memset +
trace_query_kernel), and a host clock around call + stream synchronise; the Tick's is a host clock around crt_whitted_tick without a pixel read-back (launch +
synchronise), so compare it with the query's host figure.  Medians of the timed launches after a warm-up.  The row-major result is checked against the Tick's
accumulator bit for bit.  Usage: python tools/trace_query_cost.py [--reps 30] [--warmup 5] [--width 1280 --height 720] [--out profiles/trace_query.json]"""
import argparse, ctypes as C, importlib.util, json, os, sys, time
os.environ.setdefault("CRT_ENABLE_DEBUG_HOOKS", "1")      # the library reads its diagnostic environment switches only for processes that opt in
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("cpu_ray_tracer_amd", os.path.join(REPO, "cpu-ray-tracer_amd", "__init__.py"))
crt = importlib.util.module_from_spec(spec); spec.loader.exec_module(crt)
sys.path.insert(0, os.path.join(REPO, "oracle"))
import orc                                                  # Camera::GetPrimaryRay for the ray set (CPU)
A = os.path.join(REPO, "assets")
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30); ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--width", type=int, default=1280); ap.add_argument("--height", type=int, default=720)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trace_query.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
W, H = args.width, args.height
n = W * H
# trace_query_kernel as the compiler reports it for gfx950 (-Rpass-analysis=kernel-resource-usage): <0, AltAccelDev> serves both scenes here
KERNEL = dict(name="trace_query_kernel<0, AltAccelDev>", vgprs=115, sgprs=106, scratch_bytes_per_lane=624, block_threads=256)
med = lambda v: float(sorted(v)[len(v) // 2])              # noqa: E731
cus = torch.cuda.get_device_properties(0).multi_processor_count
orc.build()
out = dict(tool="tools/trace_query_cost.py", device=torch.cuda.get_device_name(0), width=W, height=H, rays=n, reps=args.reps, warmup=args.warmup, compute_units=cus,
           kernel=KERNEL, scenes={})
for name, kind in (("tlas_scene.xml", 1), ("bunny_scene.xml", 0)):
    xml = os.path.join(A, "scenes", name)
    hs = crt.HostScene(xml, kind, A); ctx = crt.Context(W, H); hs.upload(ctx)
    o, _ = orc.load_scene(xml, kind, A); o.renderer_init(W, H)
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2).astype(np.float32)
    O, D = o.primary_rays(xy)
    rec = np.zeros(n, crt.RAY_DTYPE); rec["O"], rec["D"] = O, D
    perm = np.random.default_rng(1).permutation(n)
    orders = {"row_major": torch.from_numpy(rec.view(np.float32).reshape(-1, 7).copy()).to(dev),
              "shuffled": torch.from_numpy(rec[perm].view(np.float32).reshape(-1, 7).copy()).to(dev)}
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    # the yardstick: crt_whitted_tick (whitted_kernel<0>, one thread per pixel, 64 per block), no pixel read-back
    tick = []
    for k in range(args.warmup + args.reps):
        ctx.sync()
        t0 = time.perf_counter(); ctx._ck(ctx.L.crt_whitted_tick(ctx.h, None)); t1 = time.perf_counter()
        if k >= args.warmup:
            tick.append((t1 - t0) * 1e3)
    acc = ctx.accumulator().reshape(-1, 4)[:, :3]
    ctx.reset_counters(); ctx._ck(ctx.L.crt_whitted_tick(ctx.h, None)); tick_rays = ctx.counters()["rays"]
    res = dict(whitted_tick=dict(host_ms=med(tick), host_ms_p10_p90=[float(np.percentile(tick, 10)), float(np.percentile(tick, 90))], blocks=(n + 63) // 64, block_threads=64,
                                 find_nearest_and_shadow_rays=tick_rays))
    resident = ctx.trace_resident_lanes(0)
    for oname, rays in orders.items():
        ev, host = [], []
        with torch.cuda.stream(st):
            for k in range(args.warmup + args.reps):
                st.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(st)
                ctx._ck(ctx.L.crt_trace_device(ctx.h, 0, C.c_void_p(rays.data_ptr()), C.c_void_p(rgb.data_ptr()), None, None, C.c_size_t(n), C.c_void_p(st.cuda_stream)))
                e1.record(st); e1.synchronize()
                t1 = time.perf_counter()
                if k >= args.warmup:
                    ev.append(e0.elapsed_time(e1)); host.append((t1 - t0) * 1e3)
        got = rgb.cpu().numpy()
        want = acc if oname == "row_major" else acc[perm]
        same = bool(np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)))
        assert same, "trace_device differs from crt_whitted_tick's accumulator (%s, %s)" % (name, oname)
        ctx.reset_counters(); st.synchronize()
        with torch.cuda.stream(st):
            ctx._ck(ctx.L.crt_trace_device(ctx.h, 0, C.c_void_p(rays.data_ptr()), C.c_void_p(rgb.data_ptr()), None, None, C.c_size_t(n), C.c_void_p(st.cuda_stream)))
        st.synchronize()
        res[oname] = dict(event_ms=med(ev), event_ms_p10_p90=[float(np.percentile(ev, 10)), float(np.percentile(ev, 90))], host_ms=med(host), rays_per_s=n / (med(ev) * 1e-3),
                          find_nearest_and_shadow_rays=ctx.counters()["rays"], equals_whitted_tick=same, host_ms_over_whitted_tick=med(host) / med(tick))
    res["trace_query"] = dict(resident_lanes=resident, grid_blocks=min((n + 255) // 256, resident // 256), waves_per_simd=resident / 64 / (4 * cus))
    out["scenes"][name] = res
    print("%s %dx%d: whitted_tick %.3f ms host | trace_device row-major %.3f ms (events) %.3f ms host, shuffled %.3f ms (events) %.3f ms host | grid %d blocks of 256, %.1f waves/SIMD"
          % (name, W, H, med(tick), res["row_major"]["event_ms"], res["row_major"]["host_ms"], res["shuffled"]["event_ms"], res["shuffled"]["host_ms"],
             res["trace_query"]["grid_blocks"], res["trace_query"]["waves_per_simd"]))
    ctx.close(); hs.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
