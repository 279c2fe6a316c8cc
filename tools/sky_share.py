#!/usr/bin/env python3
"""What share of a job's summed tile cost belongs to kTileSky tiles?  Renders bench.py's default job shape (bunny 1280x720, 64 windows) twice — the first job
measures the tile costs, the second adopts them — with ONE pool launch for every tile (CRT_DEBUG_NO_SKY_KERNEL: the launch as it was before render_sky_kernel,
tile classes on), reads the planner's input back (crt_debug_job_costs) and sums it by class.  Then the same with the sky launch: what is left for the pool and
what the sky launch itself took in the measuring job.  Also per run: how many tiles carry the floor class (layout.h kTileFloor: every primary ray hits the
floor; crt_debug_tile_classes_ex) and what share of the summed NON-SKY tile cost they hold — the reach of the END pass's floor_ray.
    python tools/sky_share.py [scene.xml kind W H [windows]]        prints one JSON line"""
import ctypes as C, importlib.util, json, os, subprocess, sys
os.environ.setdefault("CRT_ENABLE_DEBUG_HOOKS", "1")      # the library reads its diagnostic environment switches only for processes that opt in
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(xml, kind, W, H, windows):
    spec = importlib.util.spec_from_file_location("cpu_ray_tracer_amd", os.path.join(REPO, "cpu-ray-tracer_amd", "__init__.py"))
    crt = importlib.util.module_from_spec(spec); spec.loader.exec_module(crt)
    A = os.path.join(REPO, "assets")
    sc = crt.HostScene(os.path.join(A, "scenes", xml), kind, A)
    ctx = crt.Context(W, H, max_frames_per_launch=64 * windows); sc.upload(ctx)
    cls = ctx.tile_classes()
    for i in range(2):
        ctx.clear(); ctx.render(1, 64 * windows, 1); ctx.sync()
    ctx.clear(); ctx.render(1, 64, 1); ctx.sync()          # (the costs are adopted by the render call that finds them arrived)
    cost = np.zeros(len(cls), np.uint32); pw, sw = C.c_double(0), C.c_double(0)
    f = ctx.L.crt_debug_job_costs; f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = f(ctx.h, cost.ctypes.data, C.addressof(pw), C.addressof(sw))
    if rc != 0: sys.exit("crt_debug_job_costs: %d" % rc)
    sky = cls == crt.TILE_SKY
    floor = (ctx.tile_classes(ex=True) & crt.TILE_FLOOR) == crt.TILE_FLOOR
    total = float(cost.astype(np.float64).sum())
    other = float(cost[~sky].astype(np.float64).sum())
    return {"floor_tiles": int(floor.sum()), "floor_cost_sum_ticks": float(cost[floor].astype(np.float64).sum()), "non_sky_cost_sum_ticks": other,
            "floor_share_of_non_sky_cost": float(cost[floor].astype(np.float64).sum()) / other if other else 0.0,
            "median_cost_floor_tile": float(np.median(cost[floor])) if floor.any() else 0.0,
            "tiles": int(len(cls)), "sky_tiles": int(sky.sum()), "cost_sum_ticks": total, "sky_cost_sum_ticks": float(cost[sky].astype(np.float64).sum()),
            "sky_cost_share": float(cost[sky].astype(np.float64).sum()) / total if total else 0.0,
            "median_cost_sky_tile": float(np.median(cost[sky])) if sky.any() else 0.0, "median_cost_other_tile": float(np.median(cost[~sky])) if (~sky).any() else 0.0,
            "pool_window_ms": pw.value * 1e-5, "sky_window_ms": sw.value * 1e-5}


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--child":
        print(json.dumps(measure(a[1], int(a[2]), int(a[3]), int(a[4]), int(a[5])))); sys.exit(0)
    xml, kind = (a[0], a[1]) if len(a) > 1 else ("bunny_scene.xml", "0")
    W, H = (a[2], a[3]) if len(a) > 3 else ("1280", "720")
    windows = a[4] if len(a) > 4 else "64"
    out = {"scene": xml, "size": [int(W), int(H)], "windows": int(windows)}
    for name, env in (("one_pool_launch", {"CRT_DEBUG_NO_SKY_KERNEL": "1"}), ("with_sky_launch", {})):      # each in a fresh process
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", xml, kind, W, H, windows], env=dict(os.environ, **env), capture_output=True, text=True)
        if r.returncode != 0: sys.exit("%s failed: %s" % (name, r.stderr[-400:]))
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
