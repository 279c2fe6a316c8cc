#!/usr/bin/env python3
"""Cost of crt_render_shapes_device beside the loop over the existing entries it replaces, one MI355X, 1280x720, cameras on a circle round the meshes, shape s the
uploaded vertices moved by p + a_s * (p.yzx * p.zxy) (tests/render_shapes_inputs.py deform_by), on bunny_scene.xml (a FileScene, BVH 0 deforms) and tlas_scene.xml
(its last BLAS deforms while every instance moves, tools/poses_cost.py `perturbed`):
  (a) 64 shapes x 1 frame through the entry: the leaf launch, the box launch of 64 workgroups (+ one TLAS build launch of 64), one job of 64 view-frames, a shape and a
      camera per lane;
  (b) the same as the loop crt_refit_device (+ crt_update_transforms_device), crt_set_camera, crt_clear, crt_render(1, 1, 1), crt_sync per shape (on a second context);
  (c) crt_render_views_device with the same cameras over the static scene: the difference to (a) is the price of the builds and of an image per lane;
  (d) - (f) 16 shapes x 64 frames, 8 x 128 and 4 x 256 the same three ways (from which frame count on the loop is the better call);
and the shape builds by themselves, the same two scenes on a 16 x 16 image (one tile), ONE view of shape 0 among 64 shapes, so the render is one lane of one wavefront
and the same one in (g) and (h):
  (g) the entry with 64 shapes, 1 view x 1 frame; (h) crt_render_views_device with that camera over the uploaded scene (the part of (g) that is not the builds and
  their read-back); (i) 64 crt_refit_device (+ crt_update_transforms_device) calls.
Per figure: the median, p10 and p90 of the wall time (a host clock round the calls, ending in a synchronise) of `reps` repetitions after `warmup`; the ways
alternate inside one repetition.  The entry's last view is compared bit for bit with the loop's once per shape count.
Usage: python tools/shapes_cost.py [--reps 8] [--warmup 2] [--out profiles/render_shapes.json]"""
import argparse, importlib.util, json, math, os, sys, time
os.environ.setdefault("CRT_ENABLE_DEBUG_HOOKS", "1")      # the library reads its diagnostic environment switches only for processes that opt in
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("cpu_ray_tracer_amd", os.path.join(REPO, "cpu-ray-tracer_amd", "__init__.py"))
crt = importlib.util.module_from_spec(spec); sys.modules["cpu_ray_tracer_amd"] = crt; spec.loader.exec_module(crt)
sys.path.insert(0, os.path.join(REPO, "tests"))
import tlas_device_inputs as inp                          # rigid()
A = os.path.join(REPO, "assets")
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=8); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--width", type=int, default=1280); ap.add_argument("--height", type=int, default=720)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_shapes.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
W, H = args.width, args.height
# the kernels' resource figures as DESIGN.md section 6 records them from a -Rpass-analysis=kernel-resource-usage build: COPIED here, not derived from a compile — the JSON says so
KERNELS = {"render_shapes_kernel<0>": dict(vgprs=78, sgprs=104, scratch_bytes_per_lane=0, waves_per_simd=6), "render_shapes_kernel<1>": dict(vgprs=93, sgprs=106, scratch_bytes_per_lane=0, waves_per_simd=5),
           "shape_leaf_kernel": dict(vgprs=24, sgprs=20, scratch_bytes_per_lane=0, lds_bytes=0), "shape_box_kernel": dict(vgprs=28, sgprs=62, scratch_bytes_per_lane=0, lds_bytes=0),
           "tlas_build_shapes_kernel": dict(vgprs=62, sgprs=51, scratch_bytes_per_lane=0, lds_bytes=17408)}
SCENES = (("bunny_scene.xml", 0, None, None), ("tlas_scene.xml", 1, (0.0, -0.3, 3.3), 5.3))      # file, kind, what the cameras look at, their distance (a FileScene: its mesh)


def circle(n, centre, radius):
    return [((centre[0] + radius * math.cos(2 * math.pi * k / n), centre[1] + 0.6, centre[2] + radius * math.sin(2 * math.pi * k / n)), centre) for k in range(n)]


def stats(v):
    return dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), n=len(v))


def perturbed(base, count, spread):
    """[count, N, 16]: pose p shifts instance i by up to `spread` and turns it about y where it stands (tools/poses_cost.py)"""
    out = np.repeat(base[None].astype(np.float32), count, axis=0)
    for p in range(count):
        for i in range(base.shape[0]):
            a = 0.7 * p + 1.3 * i
            turn = inp.rigid((0.0, 0.0, 0.0), (0.0, 0.05 * p + 0.03 * i, 0.0))
            out[p, i, :3, :3] = (turn[:3, :3].astype(np.float64) @ base[i, :3, :3].astype(np.float64)).astype(np.float32)
            out[p, i, :3, 3] = base[i, :3, 3] + np.array([spread * math.sin(a), 0.3 * spread * math.cos(1.7 * a), spread * math.cos(a)], np.float32)
    return np.ascontiguousarray(out.reshape(count, base.shape[0], 16))


def shapes_of(p0, count, step):
    p0 = np.asarray(p0, np.float32)
    return np.ascontiguousarray(np.stack([p0] + [(p0 + np.float32(step * s) * (p0[..., [1, 2, 0]] * p0[..., [2, 0, 1]])).astype(np.float32) for s in range(1, count)]))


def timed(fn, sync):
    t0 = time.perf_counter(); fn(); sync()
    return (time.perf_counter() - t0) * 1e3


global_view = {}


def load(xml, kind, w, h):
    hs = crt.HostScene(os.path.join(A, "scenes", xml), kind, A)
    ctx, ref = crt.Context(w, h), crt.Context(w, h)
    hs.upload(ctx); hs.upload(ref)
    bvh = hs.bvh_count() - 1 if kind == 1 else 0
    t = hs.bvh(bvh)["tris"]
    p0 = np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1).astype(np.float32)
    base = np.stack([hs.blas_transform(i)[0].reshape(4, 4) for i in range(hs.bvh_count())]).astype(np.float32) if kind == 1 else None
    if kind == 0:                                                            # a FileScene's vertices are in world space: the cameras circle the mesh itself
        lo, hi = p0.reshape(-1, 3).min(0).astype(np.float64), p0.reshape(-1, 3).max(0).astype(np.float64)
        global_view[xml] = (tuple(float(x) for x in (lo + hi) / 2), float(2.5 * (hi - lo).max()))
    return hs, ctx, ref, bvh, p0, base


result = dict(tool="tools/shapes_cost.py", device=torch.cuda.get_device_name(0), width=W, height=H, reps=args.reps, warmup=args.warmup, kernels=KERNELS,
              kernels_source="constants in tools/shapes_cost.py, copied from DESIGN.md section 6; not derived from the build that was measured", render={}, build={})
st = torch.cuda.Stream(device=dev)

# ---- (a) - (f): full size ----
for xml, kind, centre, radius in SCENES:
    hs, ctx, ref, bvh, p0, base = load(xml, kind, W, H)
    centre, radius = global_view.get(xml, (centre, radius))
    result["render"][xml] = dict(bvh=bvh, triangles=int(p0.shape[0]))
    for name, K, frames in (("64_shapes_x_1_frame", 64, 1), ("16_shapes_x_64_frames", 16, 64), ("8_shapes_x_128_frames", 8, 128), ("4_shapes_x_256_frames", 4, 256)):
        pairs = circle(K, centre, radius)
        pos = torch.from_numpy(shapes_of(p0, K, 0.4 / K)).to(dev)
        T = torch.from_numpy(perturbed(base, K, 0.3)).to(dev) if kind == 1 else None
        cams = torch.from_numpy(crt.camera_records(W, H, pairs)).to(dev)
        pos_each = [pos[s].contiguous() for s in range(K)]; T_each = [T[s].contiguous() for s in range(K)] if kind == 1 else None
        out = torch.zeros((K, H, W, 4), dtype=torch.float32, device=dev); out_v = torch.zeros((K, H, W, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        wall = dict(entry=[], loop=[], views_static=[])

        def loop():
            for s, (eye, target) in enumerate(pairs):
                ref.refit_device(bvh, pos_each[s], root_box=False)
                if kind == 1:
                    ref.update_transforms_device(T_each[s])
                ref.set_camera_state(eye, target); ref.clear(); ref.render(1, frames, 1); ref.sync()
        for rep in range(args.warmup + args.reps):
            e = timed(lambda: ctx.render_shapes_device(cams, bvh, pos, out, 1, frames, T=T, stream=st), st.synchronize)
            l = timed(loop, ref.sync)
            v = timed(lambda: ctx.render_views_device(cams, out_v, 1, frames, stream=st), st.synchronize)
            if rep >= args.warmup:
                wall["entry"].append(e); wall["loop"].append(l); wall["views_static"].append(v)
        same = bool(np.array_equal(ref.accumulator().view(np.uint32), out[K - 1].cpu().numpy().view(np.uint32)))     # the loop's last view is still in its accumulator
        assert same, (xml, name, "the entry's last view differs from the loop's")
        s = {k: stats(v) for k, v in wall.items()}
        result["render"][xml][name] = dict(shapes=K, frames=frames, view_frames=K * frames, wall_ms=s, loop_over_entry=s["loop"]["median"] / s["entry"]["median"],
                                           entry_over_views_static=s["entry"]["median"] / s["views_static"]["median"], last_view_bit_equal=same)
        print("%s %s: entry %.2f ms, loop %.2f ms (loop / entry = %.2f), crt_render_views over the static scene %.2f ms"
              % (xml, name, s["entry"]["median"], s["loop"]["median"], s["loop"]["median"] / s["entry"]["median"], s["views_static"]["median"]), flush=True)
        del out, out_v, cams, pos, pos_each, T, T_each
    ctx.close(); ref.close()

# ---- (g) - (i): the shape builds, one tile ----
for xml, kind, centre, radius in SCENES:
    hs, ctx, ref, bvh, p0, base = load(xml, kind, 16, 16)
    centre, radius = global_view.get(xml, (centre, radius))
    S = 64
    pos = torch.from_numpy(shapes_of(p0, S, 0.4 / S)).to(dev); pos_each = [pos[s].contiguous() for s in range(S)]
    T = torch.from_numpy(np.repeat(base.reshape(1, -1, 16), S, axis=0).copy()).to(dev) if kind == 1 else None      # the uploaded transforms for every shape: (h) renders what (g)'s one view renders
    T_each = [T[s].contiguous() for s in range(S)] if kind == 1 else None
    cams = torch.from_numpy(crt.camera_records(16, 16, circle(1, centre, radius))).to(dev)
    vs = torch.zeros((1,), dtype=torch.int32, device=dev)
    out = torch.zeros((1, 16, 16, 4), dtype=torch.float32, device=dev); out_v = torch.zeros((1, 16, 16, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    wall = dict(entry_64_shapes=[], views_1_camera=[], refit_device_x64=[])

    def refits():
        for s in range(S):
            ref.refit_device(bvh, pos_each[s], root_box=False)
            if kind == 1:
                ref.update_transforms_device(T_each[s])
    for rep in range(args.warmup + args.reps):
        e = timed(lambda: ctx.render_shapes_device(cams, bvh, pos, out, 1, 1, T=T, view_shape=vs, stream=st), st.synchronize)
        v = timed(lambda: ctx.render_views_device(cams, out_v, 1, 1, stream=st), st.synchronize)
        u = timed(refits, ref.sync)
        if rep >= args.warmup:
            wall["entry_64_shapes"].append(e); wall["views_1_camera"].append(v); wall["refit_device_x64"].append(u)
    assert torch.equal(out, out_v), (xml, "the entry's view of shape 0 differs from crt_render_views' of the uploaded scene")
    s = {k: stats(v) for k, v in wall.items()}
    part = s["entry_64_shapes"]["median"] - s["views_1_camera"]["median"]
    result["build"][xml] = dict(bvh=bvh, triangles=int(p0.shape[0]), shapes=S, loop_calls="crt_refit_device" + (" + crt_update_transforms_device" if kind == 1 else ""), wall_ms=s,
                                build_part_ms=part, refits_over_build_part=s["refit_device_x64"]["median"] / max(part, 1e-9))
    print("%s: entry (64 shape builds + a one-lane job) %.3f ms, the one-lane job alone %.3f ms, 64 x %s %.3f ms"
          % (xml, s["entry_64_shapes"]["median"], s["views_1_camera"]["median"], result["build"][xml]["loop_calls"], s["refit_device_x64"]["median"]), flush=True)
    ctx.close(); ref.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", args.out)
