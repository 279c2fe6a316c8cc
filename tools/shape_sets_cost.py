#!/usr/bin/env python3
"""Cost of crt_render_shape_sets_device beside what it replaces, one MI355X, tlas_scene.xml, cameras on a circle round the meshes, shape s of BLAS m the uploaded
vertices moved by p + a * (p.yzx * p.zxy) with a factor of its own per (shape, mesh), every instance moving per shape (tools/shapes_cost.py `perturbed`):
  render  1280x720, ALL THREE BLASes deforming: the entry against the loop over the existing entries — per shape crt_refit_device for every mesh (one host wait each),
          crt_update_transforms_device, crt_set_camera, crt_clear, crt_render(1, frames, 1), crt_sync, on a second context — at 64 shapes x 1 frame, 16 x 64, 4 x 256;
  lookup  the per-instance lookup's cost: the entry with M = 1 (BLAS 2) against crt_render_shapes_device for the same job, 64 x 1 and 16 x 64, each in a fresh child
          process, the processes alternating; with --parent-lib the crt_render_shapes_device side runs on that library (a build of the parent commit), else on this one;
  build   the builds alone, a 16x16 image (one tile), ONE view of shape 0 among 64 shapes: the entry, crt_render_views_device with that camera over the uploaded scene
          (the part of the entry that is not the builds and their read-back), and 64 x (3 crt_refit_device + crt_update_transforms_device).
Per figure: the median, min, max, p10 and p90 of the wall time (a host clock round the calls, ending in a synchronise) of `reps` repetitions after `warmup`; the ways
alternate inside one repetition.  The entry's last view is compared bit for bit with the loop's once per shape count.
Usage: python tools/shape_sets_cost.py [--reps 8] [--warmup 2] [--parent-lib PATH] [--out profiles/render_shape_sets.json]"""
import argparse, importlib.util, json, os, subprocess, sys, time
os.environ.setdefault("CRT_ENABLE_DEBUG_HOOKS", "1")      # the library reads its diagnostic environment switches only for processes that opt in
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("cpu_ray_tracer_amd", os.path.join(REPO, "cpu-ray-tracer_amd", "__init__.py"))
crt = importlib.util.module_from_spec(spec); sys.modules["cpu_ray_tracer_amd"] = crt; spec.loader.exec_module(crt)
sys.path.insert(0, os.path.join(REPO, "tests"))
A = os.path.join(REPO, "assets")
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=8); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--width", type=int, default=1280); ap.add_argument("--height", type=int, default=720)
ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library for the crt_render_shapes_device side of `lookup`")
ap.add_argument("--lookup-child", choices=("entry", "shapes"), default=None, help="(internal) time one side of `lookup` and print its JSON")
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "render_shape_sets.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
W, H = args.width, args.height
XML, CENTRE, RADIUS = "tlas_scene.xml", (0.0, -0.3, 3.3), 5.3
# the kernels' resource figures as DESIGN.md section 6 records them from the compiler's listing: COPIED here, not derived from a compile — the JSON says so
KERNELS = {"render_shape_sets_kernel": dict(vgprs=93, scratch_bytes_per_lane=0, waves_per_simd=5, instructions=2588),
           "render_shapes_kernel<1>": dict(vgprs=93, scratch_bytes_per_lane=0, waves_per_simd=5, instructions=2580),
           "shape_set_leaf_kernel": dict(vgprs=26, scratch_bytes_per_lane=0, lds_bytes=0), "shape_set_box_kernel": dict(vgprs=32, scratch_bytes_per_lane=0, lds_bytes=0)}


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), n=len(v))


def timed(fn, sync):
    t0 = time.perf_counter(); fn(); sync()
    return (time.perf_counter() - t0) * 1e3


def positions(hs, b):
    t = hs.bvh(b)["tris"]
    return np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1).astype(np.float32)


def set_shapes(p0s, count, step):
    """[count, setTris, 3, 3]: per shape the meshes' blocks; shape s > 0 of mesh m deformed by step * (s * M + m), shape 0 the uploaded vertices"""
    M = len(p0s)
    return np.ascontiguousarray(np.stack([np.concatenate([(p + np.float32(step * (s * M + m)) * (p[..., [1, 2, 0]] * p[..., [2, 0, 1]])).astype(np.float32) if s else p
                                                          for m, p in enumerate(p0s)]) for s in range(count)]))


def circle(n, centre, radius):
    import math
    return [((centre[0] + radius * math.cos(2 * math.pi * k / n), centre[1] + 0.6, centre[2] + radius * math.sin(2 * math.pi * k / n)), centre) for k in range(n)]


def perturbed(base, count, spread):
    """[count, N, 16]: pose p shifts instance i by up to `spread` and turns it about y where it stands (tools/shapes_cost.py)"""
    import math
    import tlas_device_inputs as inp                      # rigid()
    out = np.repeat(base[None].astype(np.float32), count, axis=0)
    for p in range(count):
        for i in range(base.shape[0]):
            a = 0.7 * p + 1.3 * i
            turn = inp.rigid((0.0, 0.0, 0.0), (0.0, 0.05 * p + 0.03 * i, 0.0))
            out[p, i, :3, :3] = (turn[:3, :3].astype(np.float64) @ base[i, :3, :3].astype(np.float64)).astype(np.float32)
            out[p, i, :3, 3] = base[i, :3, 3] + np.array([spread * math.sin(a), 0.3 * spread * math.cos(1.7 * a), spread * math.cos(a)], np.float32)
    return np.ascontiguousarray(out.reshape(count, base.shape[0], 16))


def scene(w, h, contexts=2):
    hs = crt.HostScene(os.path.join(A, "scenes", XML), 1, A)
    ctxs = [crt.Context(w, h) for _ in range(contexts)]
    for c in ctxs:
        hs.upload(c)
    base = np.stack([hs.blas_transform(i)[0].reshape(4, 4) for i in range(hs.bvh_count())]).astype(np.float32)
    return hs, ctxs, base


JOBS = (("64_shapes_x_1_frame", 64, 1), ("16_shapes_x_64_frames", 16, 64), ("4_shapes_x_256_frames", 4, 256))

# ---- one side of `lookup`, in a process of its own (the library is CRT_LIB_PATH's) ----
if args.lookup_child:
    st = torch.cuda.Stream(device=dev)
    hs, (ctx,), base = scene(W, H, 1)
    bvh = hs.bvh_count() - 1
    p0 = positions(hs, bvh)
    res = {}
    for name, K, frames in JOBS[:2]:
        pos = torch.from_numpy(set_shapes([p0], K, 0.4 / K)).to(dev)
        T = torch.from_numpy(perturbed(base, K, 0.3)).to(dev)
        cams = torch.from_numpy(crt.camera_records(W, H, circle(K, CENTRE, RADIUS))).to(dev)
        out = torch.zeros((K, H, W, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        if args.lookup_child == "entry":
            run = lambda: ctx.render_shape_sets_device(cams, [bvh], pos, out, 1, frames, T=T, stream=st)      # noqa: E731
        else:
            run = lambda: ctx.render_shapes_device(cams, bvh, pos, out, 1, frames, T=T, stream=st)            # noqa: E731
        wall = [timed(run, st.synchronize) for _ in range(args.warmup + args.reps)][args.warmup:]
        res[name] = dict(wall_ms=wall, checksum=int(out.view(torch.int32).to(torch.int64).sum().item()))
        del out, pos, T, cams
    ctx.close()
    print("LOOKUP_JSON " + json.dumps(res))
    sys.exit(0)

result = dict(tool="tools/shape_sets_cost.py", scene=XML, width=W, height=H, reps=args.reps, warmup=args.warmup, kernels=KERNELS,
              kernels_source="constants in tools/shape_sets_cost.py, copied from DESIGN.md section 6; not derived from the build that was measured", render={}, lookup={}, build={})

# ---- lookup: fresh processes, alternating, started before this process opens the GPU itself ----
sides = {"entry": dict(lib="this build", runs=[]), "shapes": dict(lib="the parent commit's build (--parent-lib)" if args.parent_lib else "this build", runs=[])}
if args.parent_lib:
    sides["shapes_here"] = dict(lib="this build", runs=[])                  # crt_render_shapes_device of THIS build: its kernels share their body with the entry's now
for rnd in range(2):
    for side in sides:
        env = dict(os.environ)
        if side == "shapes" and args.parent_lib:
            env["CRT_LIB_PATH"] = os.path.abspath(args.parent_lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--lookup-child", side.split("_")[0], "--reps", str(args.reps), "--warmup", str(args.warmup), "--width", str(W), "--height", str(H)]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        if p.returncode != 0:
            sys.exit("lookup child %s failed (%d):\n%s" % (side, p.returncode, p.stderr[-2000:]))
        sides[side]["runs"].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("LOOKUP_JSON ")][-1][12:]))
for name, K, frames in JOBS[:2]:
    e = [x for r in sides["entry"]["runs"] for x in r[name]["wall_ms"]]; s = [x for r in sides["shapes"]["runs"] for x in r[name]["wall_ms"]]
    sums = {r[name]["checksum"] for side in sides.values() for r in side["runs"]}
    assert len(sums) == 1, (name, "the two entries' images differ", sums)
    per = dict(entry=[float(np.median(r[name]["wall_ms"])) for r in sides["entry"]["runs"]], shapes=[float(np.median(r[name]["wall_ms"])) for r in sides["shapes"]["runs"]])
    result["lookup"][name] = dict(shapes=K, frames=frames, bvh=2, wall_ms=dict(entry_M1=stats(e), render_shapes=stats(s)), per_process_median_ms=per,
                                  render_shapes_library=sides["shapes"]["lib"], entry_over_render_shapes=float(np.median(e) / np.median(s)), images_bit_equal=True)
    if "shapes_here" in sides:
        h = [x for r in sides["shapes_here"]["runs"] for x in r[name]["wall_ms"]]
        result["lookup"][name]["wall_ms"]["render_shapes_this_build"] = stats(h)
        result["lookup"][name]["render_shapes_this_build_over_parent"] = float(np.median(h) / np.median(s))
        print("lookup %s: crt_render_shapes_device of this build %.2f ms (over the parent's: %.4f)" % (name, np.median(h), np.median(h) / np.median(s)), flush=True)
    print("lookup %s: entry with M = 1 %.2f ms, crt_render_shapes_device (%s) %.2f ms, ratio %.4f" % (name, np.median(e), sides["shapes"]["lib"], np.median(s), np.median(e) / np.median(s)), flush=True)

# ---- render: full size, all BLASes deforming ----
result["device"] = torch.cuda.get_device_name(0)
st = torch.cuda.Stream(device=dev)
hs, (ctx, ref), base = scene(W, H)
N = hs.bvh_count()
bvhs = list(range(N))
p0s = [positions(hs, b) for b in bvhs]
counts = [len(p) for p in p0s]
result["render"] = dict(bvhs=bvhs, triangles=counts)
for name, K, frames in JOBS:
    pairs = circle(K, CENTRE, RADIUS)
    pos = torch.from_numpy(set_shapes(p0s, K, 0.4 / (K * N))).to(dev)
    T = torch.from_numpy(perturbed(base, K, 0.3)).to(dev)
    cams = torch.from_numpy(crt.camera_records(W, H, pairs)).to(dev)
    offs = np.concatenate([[0], np.cumsum(counts)])
    pos_each = [[pos[s, offs[m]:offs[m + 1]].contiguous() for m in range(N)] for s in range(K)]; T_each = [T[s].contiguous() for s in range(K)]
    out = torch.zeros((K, H, W, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    wall = dict(entry=[], loop=[])

    def loop():
        for s, (eye, target) in enumerate(pairs):
            for m in range(N):
                ref.refit_device(bvhs[m], pos_each[s][m], root_box=False)
            ref.update_transforms_device(T_each[s])
            ref.set_camera_state(eye, target); ref.clear(); ref.render(1, frames, 1); ref.sync()
    for rep in range(args.warmup + args.reps):
        e = timed(lambda: ctx.render_shape_sets_device(cams, bvhs, pos, out, 1, frames, T=T, stream=st), st.synchronize)
        l = timed(loop, ref.sync)
        if rep >= args.warmup:
            wall["entry"].append(e); wall["loop"].append(l)
    same = bool(np.array_equal(ref.accumulator().view(np.uint32), out[K - 1].cpu().numpy().view(np.uint32)))     # the loop's last view is still in its accumulator
    assert same, (name, "the entry's last view differs from the loop's")
    s = {k: stats(v) for k, v in wall.items()}
    result["render"][name] = dict(shapes=K, frames=frames, view_frames=K * frames, wall_ms=s, loop_over_entry=s["loop"]["median"] / s["entry"]["median"], last_view_bit_equal=same)
    print("render %s: entry %.2f ms, loop %.2f ms (loop / entry = %.2f)" % (name, s["entry"]["median"], s["loop"]["median"], s["loop"]["median"] / s["entry"]["median"]), flush=True)
    del out, cams, pos, pos_each, T, T_each
ctx.close(); ref.close()

# ---- build: the shape builds alone, one tile ----
hs, (ctx, ref), base = scene(16, 16)
S = 64
pos = torch.from_numpy(set_shapes(p0s, S, 0.4 / (S * N))).to(dev)
pos_each = [[pos[s, offs[m]:offs[m + 1]].contiguous() for m in range(N)] for s in range(S)]
T = torch.from_numpy(np.repeat(base.reshape(1, -1, 16), S, axis=0).copy()).to(dev)      # the uploaded transforms for every shape: views_1_camera renders what the entry's one view renders
T_each = [T[s].contiguous() for s in range(S)]
cams = torch.from_numpy(crt.camera_records(16, 16, circle(1, CENTRE, RADIUS))).to(dev)
vs = torch.zeros((1,), dtype=torch.int32, device=dev)
out = torch.zeros((1, 16, 16, 4), dtype=torch.float32, device=dev); out_v = torch.zeros((1, 16, 16, 4), dtype=torch.float32, device=dev)
torch.cuda.synchronize()
wall = dict(entry_64_shapes=[], views_1_camera=[], refits_and_update_x64=[])


def refits():
    for s in range(S):
        for m in range(N):
            ref.refit_device(bvhs[m], pos_each[s][m], root_box=False)
        ref.update_transforms_device(T_each[s])


for rep in range(args.warmup + args.reps):
    e = timed(lambda: ctx.render_shape_sets_device(cams, bvhs, pos, out, 1, 1, T=T, view_shape=vs, stream=st), st.synchronize)
    v = timed(lambda: ctx.render_views_device(cams, out_v, 1, 1, stream=st), st.synchronize)
    u = timed(refits, ref.sync)
    if rep >= args.warmup:
        wall["entry_64_shapes"].append(e); wall["views_1_camera"].append(v); wall["refits_and_update_x64"].append(u)
assert torch.equal(out, out_v), "the entry's view of shape 0 differs from crt_render_views' of the uploaded scene"
s = {k: stats(v) for k, v in wall.items()}
part = s["entry_64_shapes"]["median"] - s["views_1_camera"]["median"]
result["build"] = dict(bvhs=bvhs, triangles=counts, shapes=S, loop_calls="%d crt_refit_device + crt_update_transforms_device" % N, wall_ms=s, build_part_ms=part,
                       loop_over_build_part=s["refits_and_update_x64"]["median"] / max(part, 1e-9))
print("build: entry (64 x %d shape builds + a one-lane job) %.3f ms, the one-lane job alone %.3f ms, 64 x (%s) %.3f ms"
      % (N, s["entry_64_shapes"]["median"], s["views_1_camera"]["median"], result["build"]["loop_calls"], s["refits_and_update_x64"]["median"]), flush=True)
ctx.close(); ref.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", args.out)
