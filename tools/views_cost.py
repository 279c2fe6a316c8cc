#!/usr/bin/env python3
"""Cost of crt_render_views_device beside the loop over the existing entries it replaces, 1280x720, one MI355X, bunny_scene.xml and tlas_scene.xml, cameras on a
circle round the mesh:
  (a) 64 views x 1 frame through the entry: one job of 64 view-frames, a camera per lane;
  (b) the same 64 frames as the loop crt_set_camera, crt_clear, crt_render(1, 1, 1), crt_sync per view — the existing entries, which this entry does not change;
  (c) 16 views x 64 frames both ways;
  (d), (e) the same 1 024 view-frames as 8 views x 128 frames and 4 views x 256 frames both ways: from two windows per view on, the loop's renders are jobs of the
      pool kernel — where a caller should go back to looping crt_render.
Per figure: the median, p10 and p90 of `reps` repetitions after `warmup`, of the wall time (a host clock round the calls, ending in a synchronise) and of the device
time (the entry: HIP events on its stream round the call, i.e. render + per-view accumulate kernels; the loop: the library's own event figures of its render and
accumulate kernels, crt_get_timing).  The loop and the entry alternate inside one repetition.  The outputs of both are compared bit for bit once per shape.
Usage: python tools/views_cost.py [--reps 10] [--warmup 2] [--out profiles/render_views.json]"""
import argparse, importlib.util, json, math, os, sys, time
os.environ.setdefault("CRT_ENABLE_DEBUG_HOOKS", "1")      # the library reads its diagnostic environment switches only for processes that opt in
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("cpu_ray_tracer_amd", os.path.join(REPO, "cpu-ray-tracer_amd", "__init__.py"))
crt = importlib.util.module_from_spec(spec); spec.loader.exec_module(crt)
A = os.path.join(REPO, "assets")
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--width", type=int, default=1280); ap.add_argument("--height", type=int, default=720)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_views.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
W, H = args.width, args.height
# the kernels as the compiler reports them for gfx950 (-Rpass-analysis=kernel-resource-usage)
KERNELS = {"render_views_kernel<BvhWorld<0>>": dict(vgprs=92, sgprs=106, scratch_bytes_per_lane=0), "render_views_kernel<BvhWorld<1>>": dict(vgprs=92, sgprs=106, scratch_bytes_per_lane=0),
           "views_accumulate_kernel": dict(vgprs=17, sgprs=33, scratch_bytes_per_lane=0)}
SCENES = [("bunny_scene.xml", 0, (0.0, -0.2, 2.0), 4.0), ("tlas_scene.xml", 1, (0.0, -0.3, 3.3), 5.3)]
SHAPES = [("a_b_64_views_x_1_frame", 64, 1), ("c_16_views_x_64_frames", 16, 64), ("d_8_views_x_128_frames", 8, 128), ("e_4_views_x_256_frames", 4, 256)]


def circle(n, centre, radius):
    return [((centre[0] + radius * math.cos(2 * math.pi * k / n), centre[1] + 0.6, centre[2] + radius * math.sin(2 * math.pi * k / n)), centre) for k in range(n)]


def stats(v):
    return dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), n=len(v))


result = dict(tool="tools/views_cost.py", device=torch.cuda.get_device_name(0), width=W, height=H, reps=args.reps, warmup=args.warmup, kernels=KERNELS, scenes={})
for xml, kind, centre, radius in SCENES:
    hs = crt.HostScene(os.path.join(A, "scenes", xml), kind, A); ctx = crt.Context(W, H); hs.upload(ctx)
    st = torch.cuda.Stream(device=dev)
    per_scene = {}
    for name, K, frames in SHAPES:
        pairs = circle(K, centre, radius)
        cams = torch.from_numpy(crt.camera_records(W, H, pairs)).to(dev)
        out = torch.zeros((K, H, W, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ent_wall, ent_dev, loop_wall, loop_dev = [], [], [], []
        for rep in range(args.warmup + args.reps):
            # the entry
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(st); ctx.render_views_device(cams, out, 1, frames, stream=st); e1.record(st); st.synchronize()
            t1 = time.perf_counter()
            # the loop
            ctx.sync(); ctx.timing()
            t2 = time.perf_counter()
            for pos, target in pairs:
                ctx.set_camera_state(pos, target); ctx.clear(); ctx.render(1, frames, 1); ctx.sync()
            t3 = time.perf_counter()
            tm = ctx.timing()
            if rep >= args.warmup:
                ent_wall.append((t1 - t0) * 1e3); ent_dev.append(e0.elapsed_time(e1))
                loop_wall.append((t3 - t2) * 1e3); loop_dev.append(tm["render_kernel_ms"] + tm["resolve_kernel_ms"])
        # the last view of the loop is still in the accumulator
        same = bool(np.array_equal(ctx.accumulator().view(np.uint32), out[K - 1].cpu().numpy().view(np.uint32)))
        assert same, (xml, name, "the entry's last view differs from the loop's")
        ew, lw = stats(ent_wall), stats(loop_wall)
        per_scene[name] = dict(views=K, frames=frames, view_frames=K * frames, entry=dict(wall_ms=ew, device_ms=stats(ent_dev)), loop=dict(wall_ms=lw, device_ms=stats(loop_dev)),
                               loop_over_entry_wall=lw["median"] / ew["median"], last_view_bit_equal=same)
        print("%s %s: entry %.2f ms wall / %.2f ms device, loop %.2f ms wall / %.2f ms device, loop / entry = %.2f"
              % (xml, name, ew["median"], float(np.median(ent_dev)), lw["median"], float(np.median(loop_dev)), lw["median"] / ew["median"]), flush=True)
        del out, cams
    result["scenes"][xml] = per_scene
    ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", args.out)
