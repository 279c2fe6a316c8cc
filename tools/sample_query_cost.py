#!/usr/bin/env python3
"""Cost of crt_sample_device: 2^20 primary rays of bench.py's bunny camera (1280x720, jittered pixel positions, seeds 1 + i) through Renderer::Sample as a ray query,
beside crt_render's time for ONE 1280x720 frame (921 600 paths through render_tiles_kernel).  The query's time is the span of events on the stream around the bare
crt_sample_device call (cursor memset + sample_query_kernel<BvhWorld<0>>), the seeds restored before each launch; median of the timed launches after a warm-up.
The frame's time is a host clock around clear + crt_render(1, 1, 1) + sync, and the library's own event figure for the render kernel.  Rays per path come from
crt_counters.  Usage: python tools/sample_query_cost.py [--reps 30] [--warmup 5] [--out profiles/sample_query.json]"""
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
ap.add_argument("--reps", type=int, default=30); ap.add_argument("--warmup", type=int, default=5); ap.add_argument("--rays", type=int, default=1 << 20)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sample_query.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
W, H, n = 1280, 720, args.rays
# sample_query_kernel<BvhWorld<0>> as the compiler reports it for gfx950 (-Rpass-analysis=kernel-resource-usage)
KERNEL = dict(name="sample_query_kernel<BvhWorld<0>>", vgprs=76, sgprs=106, scratch_bytes_per_lane=0, block_threads=256)

xml = os.path.join(A, "scenes", "bunny_scene.xml")
hs = crt.HostScene(xml, 0, A); ctx = crt.Context(W, H); hs.upload(ctx)
orc.build(); o, _ = orc.load_scene(xml, 0, A); o.renderer_init(W, H)
rng = np.random.default_rng(1)
O, D = o.primary_rays(np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1).astype(np.float32))
rec = np.zeros(n, crt.RAY_DTYPE); rec["O"], rec["D"] = O, D
rays = torch.from_numpy(rec.view(np.float32).reshape(-1, 7).copy()).to(dev)
seeds0 = torch.arange(1, n + 1, dtype=torch.int32, device=dev); seeds = seeds0.clone()
rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
st = torch.cuda.Stream(device=dev)
torch.cuda.synchronize()


def launch():
    ctx._ck(ctx.L.crt_sample_device(ctx.h, 0, C.c_void_p(rays.data_ptr()), C.c_void_p(seeds.data_ptr()), C.c_void_p(rgb.data_ptr()), C.c_size_t(n), C.c_void_p(st.cuda_stream)))


ms = []
with torch.cuda.stream(st):
    for k in range(args.warmup + args.reps):
        seeds.copy_(seeds0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); launch(); e1.record(st); e1.synchronize()
        if k >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    seeds.copy_(seeds0)
    st.synchronize(); ctx.reset_counters(); launch(); st.synchronize()
cnt = ctx.counters()
assert torch.isfinite(rgb).all().item()
frame, kern = [], []
for k in range(args.warmup + args.reps):
    ctx.clear(); ctx.sync(); ctx.timing()
    t0 = time.perf_counter(); ctx.render(1 + k, 1, 1); ctx.sync(); t1 = time.perf_counter()
    if k >= args.warmup:
        frame.append((t1 - t0) * 1e3); kern.append(ctx.timing()["render_kernel_ms"])
med = lambda v: float(sorted(v)[len(v) // 2])
resident = ctx.sample_resident_lanes(0)
cus = torch.cuda.get_device_properties(0).multi_processor_count
q = med(ms)
out = dict(tool="tools/sample_query_cost.py", device=torch.cuda.get_device_name(0), scene="bunny_scene.xml", rays=n, reps=args.reps, warmup=args.warmup,
           sample_query=dict(ms=q, ms_p10_p90=[float(np.percentile(ms, 10)), float(np.percentile(ms, 90))], paths_per_s=n / (q * 1e-3), rays_per_path=cnt["rays"] / n,
                             rays_per_s=cnt["rays"] / (q * 1e-3), resident_lanes=resident, grid_blocks=min((n + 255) // 256, resident // 256), compute_units=cus,
                             waves_per_simd=resident / 64 / (4 * cus), kernel=KERNEL, lds_bytes_per_block="(stack depth + 15) * 1024: traversal stack + 15 factor columns, 4 wavefronts"),
           render_one_frame=dict(paths=W * H, host_ms=med(frame), render_kernel_ms=med(kern), paths_per_s=W * H / (med(frame) * 1e-3)))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
print("sample_device: %d paths in %.3f ms (%.1f M paths/s, %.2f rays/path), grid %d blocks of 256, %.1f waves/SIMD | crt_render one %dx%d frame: %.3f ms host, %.3f ms kernel"
      % (n, q, n / q / 1e3, cnt["rays"] / n, out["sample_query"]["grid_blocks"], out["sample_query"]["waves_per_simd"], W, H, med(frame), med(kern)))
