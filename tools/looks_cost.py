#!/usr/bin/env python3
"""Cost of crt_render_looks_device beside the two loops it replaces, one MI355X, 1280x720, bunny_scene.xml and tlas_scene.xml, cameras on a circle round the meshes,
every look a step of a material sweep with the light quad moving along x (reflectivity of material 0 from 0 to 1, the light from -1.5 to +1.5 of its place).
For looks x frames = 64 x 1, 16 x 64 and 4 x 256, one view per look:
  (a) job           crt_render_looks_device: one build launch, one job of looks x frames view-frames, a look and a camera per lane;
  (b) update loop   crt_update_look, crt_set_camera, crt_clear, crt_render(1, frames, 1), crt_sync per look (on a second context);
  (c) upload loop   the host scene takes the look over, crt_upload_scene, then the same render per look (on a third context): what a look cost before crt_update_look;
  (d) job, L = 1    the job with ONE look, the live one, for all the cameras — against
  (e) views         crt_render_views_device with the same cameras: (d) - (e) is what lane-local looks cost (the table reads, the general light quad test).
Per figure: the median, p10 and p90 of the wall time (a host clock round the calls, ending in a synchronise) of `reps` repetitions after `warmup`; the ways
alternate inside one repetition, so drift of the machine reaches all of them alike.  The job's last view is compared bit for bit with the update loop's once per shape.
Usage: python tools/looks_cost.py [--reps 5] [--warmup 1] [--out profiles/render_looks.json]"""
import argparse, importlib.util, json, math, os, sys, time
os.environ.setdefault("CRT_ENABLE_DEBUG_HOOKS", "1")      # the library reads its diagnostic environment switches only for processes that opt in
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("cpu_ray_tracer_amd", os.path.join(REPO, "cpu-ray-tracer_amd", "__init__.py"))
crt = importlib.util.module_from_spec(spec); sys.modules["cpu_ray_tracer_amd"] = crt; spec.loader.exec_module(crt)
A = os.path.join(REPO, "assets")
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--width", type=int, default=1280); ap.add_argument("--height", type=int, default=720)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_looks.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
W, H = args.width, args.height
SCENES = [("bunny_scene.xml", 0, (0.0, -0.2, 2.0), 4.0), ("tlas_scene.xml", 1, (0.0, -0.3, 3.3), 5.3)]
SHAPES = [(64, 1), (16, 64), (4, 256)]
# the kernels' resource figures as DESIGN.md section 6 records them from the compiler's kernel metadata: COPIED here, not derived from a compile — the JSON says so
KERNELS = {"render_looks_kernel<0>": dict(vgprs=96, sgprs=75, scratch_bytes_per_lane=0, waves_per_simd=5), "render_looks_kernel<1>": dict(vgprs=107, sgprs=80, scratch_bytes_per_lane=0, waves_per_simd=4),
           "look_build_kernel": dict(vgprs=32, sgprs=24, scratch_bytes_per_lane=0, lds_bytes=0)}


def circle(n, centre, radius):
    return [((centre[0] + radius * math.cos(2 * math.pi * k / n), centre[1] + 0.6, centre[2] + radius * math.sin(2 * math.pi * k / n)), centre) for k in range(n)]


def stats(v):
    return dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), n=len(v))


def sweep(base, count):
    """`count` looks round `base`: material 0's reflectivity from 0 to 1, the light quad from -1.5 to +1.5 along x (T and invT: a pure translation)"""
    out = []
    for k in range(count):
        s = k / max(count - 1, 1)
        look = dict(base); m = list(base["materials"]); m[0] = (s, m[0][1] * (1.0 - s), m[0][2], m[0][3]); look["materials"] = m
        T = np.asarray(base["light_T"], np.float32).reshape(4, 4).copy(); T[0, 3] += np.float32(3.0 * s - 1.5)
        inv = np.eye(4, dtype=np.float32); inv[:3, 3] = -T[:3, 3]
        look["light_T"], look["light_invT"] = T.reshape(16), inv.reshape(16)
        out.append(look)
    return crt.look_records(out)


def timed(fn, sync):
    t0 = time.perf_counter(); fn(); sync()
    return (time.perf_counter() - t0) * 1e3


result = dict(tool="tools/looks_cost.py", device=torch.cuda.get_device_name(0), width=W, height=H, reps=args.reps, warmup=args.warmup, kernels=KERNELS,
              kernels_source="constants in tools/looks_cost.py, copied from DESIGN.md section 6; not derived from the build that was measured", scenes={})
st = torch.cuda.Stream(device=dev)
for xml, kind, centre, radius in SCENES:
    path = os.path.join(A, "scenes", xml)
    hs, hs_up = crt.HostScene(path, kind, A), crt.HostScene(path, kind, A)
    ctx, ref, up = crt.Context(W, H), crt.Context(W, H), crt.Context(W, H)
    hs.upload(ctx); hs.upload(ref); hs.upload(up)
    base_rec = hs.look(); base = crt.look_dicts(base_rec)[0]
    result["scenes"][xml] = {}
    for L, frames in SHAPES:
        pairs = circle(L, centre, radius)
        rec_h = sweep(base, L)
        cams = torch.from_numpy(crt.camera_records(W, H, pairs)).to(dev)
        looks = torch.from_numpy(rec_h.view(np.int32)).to(dev); live = torch.from_numpy(base_rec.view(np.int32).reshape(1, -1)).to(dev)
        zeros = torch.zeros((L,), dtype=torch.int32, device=dev)
        out = torch.zeros((L, H, W, 4), dtype=torch.float32, device=dev); out_v = torch.zeros((L, H, W, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        wall = dict(job=[], update_loop=[], upload_loop=[], job_one_look=[], views=[])

        def update_loop():
            for l, (pos, target) in enumerate(pairs):
                ref.update_look(rec_h[l]); ref.set_camera_state(pos, target); ref.clear(); ref.render(1, frames, 1); ref.sync()

        def upload_loop():
            for l, (pos, target) in enumerate(pairs):
                hs_up.set_look(rec_h[l]); hs_up.upload(up); up.set_camera_state(pos, target); up.clear(); up.render(1, frames, 1); up.sync()
        for rep in range(args.warmup + args.reps):
            j = timed(lambda: ctx.render_looks_device(cams, looks, out, 1, frames, stream=st), st.synchronize)
            u = timed(update_loop, ref.sync)
            f = timed(upload_loop, up.sync)
            o = timed(lambda: ctx.render_looks_device(cams, live, out_v, 1, frames, view_look=zeros, stream=st), st.synchronize)
            one = out_v[L - 1].clone()
            v = timed(lambda: ctx.render_views_device(cams, out_v, 1, frames, stream=st), st.synchronize)
            if rep >= args.warmup:
                for k, x in zip(("job", "update_loop", "upload_loop", "job_one_look", "views"), (j, u, f, o, v)):
                    wall[k].append(x)
        last = out[L - 1].cpu().numpy().view(np.uint32)
        same = bool(np.array_equal(ref.accumulator().view(np.uint32), last)) and bool(np.array_equal(up.accumulator().view(np.uint32), last))
        assert same, (xml, L, frames, "the job's last view differs from a loop's")
        assert torch.equal(one, out_v[L - 1]), (xml, L, frames, "the one-look job differs from crt_render_views")
        s = {k: stats(v) for k, v in wall.items()}
        d = s["job_one_look"]["median"] - s["views"]["median"]
        spread = max(s["views"]["p90"] - s["views"]["p10"], s["job_one_look"]["p90"] - s["job_one_look"]["p10"])
        result["scenes"][xml]["%d_looks_x_%d_frames" % (L, frames)] = dict(
            looks=L, frames=frames, view_frames=L * frames, wall_ms=s, update_loop_over_job=s["update_loop"]["median"] / s["job"]["median"],
            upload_loop_over_job=s["upload_loop"]["median"] / s["job"]["median"], one_look_minus_views_ms=d, one_look_over_views=s["job_one_look"]["median"] / s["views"]["median"],
            run_to_run_spread_ms=spread, one_look_slower_than_spread=bool(d > spread), last_view_bit_equal=same)
        print("%s %d looks x %d frames: job %.1f ms, update loop %.1f ms (x%.2f), upload loop %.1f ms (x%.2f); one live look %.1f ms vs crt_render_views %.1f ms (spread %.1f ms)"
              % (xml, L, frames, s["job"]["median"], s["update_loop"]["median"], s["update_loop"]["median"] / s["job"]["median"], s["upload_loop"]["median"],
                 s["upload_loop"]["median"] / s["job"]["median"], s["job_one_look"]["median"], s["views"]["median"], spread), flush=True)
        del out, out_v, cams, looks
    ctx.close(); ref.close(); up.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", args.out)
