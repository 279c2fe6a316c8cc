#!/usr/bin/env python3
"""Cost of crt_render_poses_device beside the loop over the existing entries it replaces, one MI355X, 1280x720, tlas_scene.xml, cameras on a circle round the
meshes, every pose the scene's three instances shifted and turned by amounts of its own:
  (a) 64 poses x 1 frame through the entry: one build launch of 64 workgroups, one job of 64 view-frames, a pose and a camera per lane;
  (b) the same as the loop crt_update_transforms_device, crt_set_camera, crt_clear, crt_render(1, 1, 1), crt_sync per pose (on a second context);
  (c) crt_render_views_device with the same cameras over the static scene: the difference to (a) is the price of the builds and of a TLAS per lane;
  (d) - (f) 16 poses x 64 frames the same three ways;
and the batched build by itself, scenes ring40 and rand256 of tests/tlas_device_inputs.py on a 16 x 16 image (one tile), ONE view of pose 0 among 64 poses, so the
render is one lane of one wavefront and the same one in (g) and (h):
  (g) the entry with 64 poses, 1 view x 1 frame; (h) crt_render_views_device with that camera over the scene at pose 0 (the part of (g) that is not the builds and
  their read-back); (i) 64 crt_update_transforms_device calls.
Per figure: the median, p10 and p90 of the wall time (a host clock round the calls, ending in a synchronise) of `reps` repetitions after `warmup`; the ways
alternate inside one repetition.  The entry's last view is compared bit for bit with the loop's once per shape.
Usage: python tools/poses_cost.py [--reps 10] [--warmup 2] [--out profiles/render_poses.json]"""
import argparse, importlib.util, json, math, os, sys, tempfile, time
os.environ.setdefault("CRT_ENABLE_DEBUG_HOOKS", "1")      # the library reads its diagnostic environment switches only for processes that opt in
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("cpu_ray_tracer_amd", os.path.join(REPO, "cpu-ray-tracer_amd", "__init__.py"))
crt = importlib.util.module_from_spec(spec); sys.modules["cpu_ray_tracer_amd"] = crt; spec.loader.exec_module(crt)
sys.path.insert(0, os.path.join(REPO, "tests"))
import tlas_device_inputs as inp                          # the ring40 / rand256 scenes and transforms
from pathlib import Path
A = os.path.join(REPO, "assets")
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--width", type=int, default=1280); ap.add_argument("--height", type=int, default=720)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_poses.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
W, H = args.width, args.height
# the kernels' resource figures as DESIGN.md section 6 records them from a -Rpass-analysis=kernel-resource-usage build: COPIED here, not derived from a compile — the JSON says so
KERNELS = {"render_poses_kernel": dict(vgprs=92, sgprs=104, scratch_bytes_per_lane=0, waves_per_simd=5), "render_views_kernel<BvhWorld<1>>": dict(vgprs=92, sgprs=106, scratch_bytes_per_lane=0, waves_per_simd=5),
           "tlas_build_poses_kernel": dict(vgprs=62, sgprs=50, scratch_bytes_per_lane=0, lds_bytes=17408), "tlas_build_kernel": dict(vgprs=62, sgprs=43, scratch_bytes_per_lane=0, lds_bytes=17408)}


def circle(n, centre, radius):
    return [((centre[0] + radius * math.cos(2 * math.pi * k / n), centre[1] + 0.6, centre[2] + radius * math.sin(2 * math.pi * k / n)), centre) for k in range(n)]


def stats(v):
    return dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), n=len(v))


def perturbed(base, count, spread):
    """[count, N, 16]: pose p shifts instance i by up to `spread` and turns it about y where it stands"""
    out = np.repeat(base[None].astype(np.float32), count, axis=0)
    for p in range(count):
        for i in range(base.shape[0]):
            a = 0.7 * p + 1.3 * i
            turn = inp.rigid((0.0, 0.0, 0.0), (0.0, 0.05 * p + 0.03 * i, 0.0))
            out[p, i, :3, :3] = (turn[:3, :3].astype(np.float64) @ base[i, :3, :3].astype(np.float64)).astype(np.float32)
            out[p, i, :3, 3] = base[i, :3, 3] + np.array([spread * math.sin(a), 0.3 * spread * math.cos(1.7 * a), spread * math.cos(a)], np.float32)
    return np.ascontiguousarray(out.reshape(count, base.shape[0], 16))


def timed(fn, sync):
    t0 = time.perf_counter(); fn(); sync()
    return (time.perf_counter() - t0) * 1e3


result = dict(tool="tools/poses_cost.py", device=torch.cuda.get_device_name(0), width=W, height=H, reps=args.reps, warmup=args.warmup, kernels=KERNELS,
              kernels_source="constants in tools/poses_cost.py, copied from DESIGN.md section 6; not derived from the build that was measured", render={}, build={})
st = torch.cuda.Stream(device=dev)

# ---- (a) - (f): tlas_scene.xml at full size ----
xml = os.path.join(A, "scenes", "tlas_scene.xml")
hs = crt.HostScene(xml, 1, A); ctx = crt.Context(W, H); ref = crt.Context(W, H); hs.upload(ctx); hs.upload(ref)
base = np.stack([hs.blas_transform(i)[0].reshape(4, 4) for i in range(hs.bvh_count())]).astype(np.float32)
for name, K, frames in (("64_poses_x_1_frame", 64, 1), ("16_poses_x_64_frames", 16, 64)):
    pairs = circle(K, (0.0, -0.3, 3.3), 5.3)
    T_h = perturbed(base, K, 0.3)
    cams = torch.from_numpy(crt.camera_records(W, H, pairs)).to(dev); T = torch.from_numpy(T_h).to(dev)
    T_each = [T[p].contiguous() for p in range(K)]
    out = torch.zeros((K, H, W, 4), dtype=torch.float32, device=dev); out_v = torch.zeros((K, H, W, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    wall = dict(entry=[], loop=[], views_static=[])

    def loop():
        for p, (pos, target) in enumerate(pairs):
            ref.update_transforms_device(T_each[p]); ref.set_camera_state(pos, target); ref.clear(); ref.render(1, frames, 1); ref.sync()
    for rep in range(args.warmup + args.reps):
        e = timed(lambda: ctx.render_poses_device(cams, T, out, 1, frames, stream=st), st.synchronize)
        l = timed(loop, ref.sync)
        v = timed(lambda: ctx.render_views_device(cams, out_v, 1, frames, stream=st), st.synchronize)
        if rep >= args.warmup:
            wall["entry"].append(e); wall["loop"].append(l); wall["views_static"].append(v)
    same = bool(np.array_equal(ref.accumulator().view(np.uint32), out[K - 1].cpu().numpy().view(np.uint32)))     # the loop's last view is still in its accumulator
    assert same, (name, "the entry's last view differs from the loop's")
    s = {k: stats(v) for k, v in wall.items()}
    result["render"][name] = dict(poses=K, frames=frames, view_frames=K * frames, wall_ms=s, loop_over_entry=s["loop"]["median"] / s["entry"]["median"],
                                  entry_over_views_static=s["entry"]["median"] / s["views_static"]["median"], last_view_bit_equal=same)
    print("tlas_scene.xml %s: entry %.2f ms, loop %.2f ms (loop / entry = %.2f), crt_render_views over the static scene %.2f ms"
          % (name, s["entry"]["median"], s["loop"]["median"], s["loop"]["median"] / s["entry"]["median"], s["views_static"]["median"]), flush=True)
    del out, out_v, cams, T, T_each
ctx.close(); ref.close()

# ---- (g) - (i): the batched build, one tile ----
tmp = Path(tempfile.mkdtemp(prefix="poses_cost_"))
for name in ("ring40", "rand256"):
    hs = crt.HostScene(inp.scene_xml(tmp, name), 1, A); ctx = crt.Context(16, 16); ref = crt.Context(16, 16); hs.upload(ctx); hs.upload(ref)
    P = 64
    T_h = perturbed(inp.transforms(name), P, 0.2)
    T = torch.from_numpy(T_h).to(dev); T_each = [T[p].contiguous() for p in range(P)]
    cams = torch.from_numpy(crt.camera_records(16, 16, [((0.0, 1.0, -3.0), (0.0, 0.5, 6.0))])).to(dev)
    vp = torch.zeros((1,), dtype=torch.int32, device=dev)
    out = torch.zeros((1, 16, 16, 4), dtype=torch.float32, device=dev); out_v = torch.zeros((1, 16, 16, 4), dtype=torch.float32, device=dev)
    ctx.update_transforms_device(T_each[0])                              # (h) renders what (g)'s one view renders
    torch.cuda.synchronize()
    wall = dict(entry_64_poses=[], views_1_camera=[], update_transforms_device_x64=[])

    def updates():
        for p in range(P):
            ref.update_transforms_device(T_each[p])
    for rep in range(args.warmup + args.reps):
        e = timed(lambda: ctx.render_poses_device(cams, T, out, 1, 1, view_pose=vp, stream=st), st.synchronize)
        v = timed(lambda: ctx.render_views_device(cams, out_v, 1, 1, stream=st), st.synchronize)
        u = timed(updates, ref.sync)
        if rep >= args.warmup:
            wall["entry_64_poses"].append(e); wall["views_1_camera"].append(v); wall["update_transforms_device_x64"].append(u)
    assert torch.equal(out, out_v), (name, "the entry's view of pose 0 differs from crt_render_views' of the scene at pose 0")
    s = {k: stats(v) for k, v in wall.items()}
    result["build"][name] = dict(instances=int(T_h.shape[1]), poses=P, wall_ms=s, build_part_ms=s["entry_64_poses"]["median"] - s["views_1_camera"]["median"],
                                 updates_over_build_part=s["update_transforms_device_x64"]["median"] / max(s["entry_64_poses"]["median"] - s["views_1_camera"]["median"], 1e-9))
    print("%s: entry (64 builds + a one-lane job) %.3f ms, the one-lane job alone %.3f ms, 64 crt_update_transforms_device %.3f ms"
          % (name, s["entry_64_poses"]["median"], s["views_1_camera"]["median"], s["update_transforms_device_x64"]["median"]), flush=True)
    ctx.close(); ref.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", args.out)
