#!/usr/bin/env python3
"""Which render kernel for a scene in the 32-bit pool-reference form?  One process, one context per variant of CRT_RENDER_KERNEL (tiles | pool_always | default:
the switch is read when a context is created), the same job on each in turn, `rounds` times over — interleaved repeats, so drift of the shared machine hits every
variant alike.  Per (variant, windows): the median job time (host clock around render + sync), G rays/s from the job's ray counter, and the scatter of the
repeats (max - min, and as a share of the median).  The accumulators of the variants are compared once per job size: they must be the same bits.

    python tools/pool_wide_bench.py [scene.xml kind [W H [rounds [K ...]]]] [--out FILE.json]
    default: bunny14_scene.xml 0 1280 720 5 20 64"""
import json, os, statistics, sys, time, zlib
os.environ.setdefault("CRT_ENABLE_DEBUG_HOOKS", "1")      # the library reads its diagnostic environment switches only for processes that opt in
import importlib.util
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("cpu_ray_tracer_amd", os.path.join(REPO, "cpu-ray-tracer_amd", "__init__.py"))
crt = importlib.util.module_from_spec(spec); spec.loader.exec_module(crt)

a = sys.argv[1:]
out_path = None
if "--out" in a:
    i = a.index("--out"); out_path = a[i + 1]; del a[i:i + 2]
scene, kind = (a[0], int(a[1])) if len(a) > 1 else ("bunny14_scene.xml", 0)
W, H = (int(a[2]), int(a[3])) if len(a) > 3 else (1280, 720)
rounds = int(a[4]) if len(a) > 4 else 5
Ks = [int(k) for k in a[5:]] or [20, 64]
A = os.path.join(REPO, "assets")
sc = crt.HostScene(os.path.join(A, "scenes", scene), kind, A)
VARIANTS = ["tiles", "pool_always", "default"]
ctxs = {}
for v in VARIANTS:
    if v == "default": os.environ.pop("CRT_RENDER_KERNEL", None)
    else: os.environ["CRT_RENDER_KERNEL"] = v
    c = crt.Context(W, H); sc.upload(c); c.reserve(64 * max(Ks), 1)
    ctxs[v] = c
os.environ.pop("CRT_RENDER_KERNEL", None)
need, limit, bits = ctxs["default"].pool_lds(64 * max(Ks))
res = dict(scene=scene, kind=kind, width=W, height=H, rounds=rounds, pool_ref_bits=bits, pool_lds_bytes=need, pool_lds_limit=limit,
           method="one process, one context per CRT_RENDER_KERNEL variant, jobs interleaved round-robin; first two jobs of every (variant, K) are warm-up "
                  "(the second is the first planned one); host clock around render + sync; scatter = max - min of the timed repeats", jobs=[])
for K in Ks:
    frames = 64 * K
    ms = {v: [] for v in VARIANTS}; rays = {}; pool = {}; crc = {}
    for r in range(rounds + 2):
        for v in VARIANTS:
            c = ctxs[v]
            c.clear(); c.reset_counters(); c.sync(); c.timing()
            t0 = time.perf_counter(); c.render(1, frames, 1); c.sync(); dt = (time.perf_counter() - t0) * 1e3
            t = c.timing()
            if r >= 2:
                ms[v].append(dt); rays[v] = c.counters()["rays"]; pool[v] = (t["pool_launches"], t["render_launches"], t["split_launches"])
            if r == rounds + 1: crc[v] = zlib.crc32(c.accumulator().tobytes())
    same = len(set(crc.values())) == 1
    for v in VARIANTS:
        med = statistics.median(ms[v]); sp = max(ms[v]) - min(ms[v])
        row = dict(windows=K, variant=v, ms_per_job=round(med, 2), grays_per_s=round(rays[v] / med / 1e6, 2), scatter_ms=round(sp, 2), scatter_pct=round(100 * sp / med, 2),
                   repeats_ms=[round(x, 2) for x in ms[v]], pool_launches=pool[v][0], render_launches=pool[v][1], split_launches=pool[v][2], accumulator_crc="%08x" % crc[v])
        res["jobs"].append(row)
        print("K=%-3d %-12s %8.2f ms/job  %6.2f G rays/s  scatter %.2f ms (%.1f %%)  pool %d/%d launches, split %d  crc %08x" % (K, v, med, row["grays_per_s"], sp, row["scatter_pct"], pool[v][0], pool[v][1], pool[v][2], crc[v]), flush=True)
    print("K=%d: accumulators %s" % (K, "identical" if same else "DIFFER"), flush=True)
    res.setdefault("accumulators_identical", {})[str(K)] = same
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
