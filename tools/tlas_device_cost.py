#!/usr/bin/env python3
"""Cost of one instance-motion step of a two-level scene whose transforms are produced on the GPU, two ways, for N = 3, 40 and 256 instances:
  (a) host route:   transforms tensor -> host copy -> crt_host_scene_set_transform for every instance (SetTransform + TLASBVH::Build each) ->
                    crt_host_scene_update(CRT_UPDATE_TRANSFORMS) -> sync
  (b) device route: crt_update_transforms_device (one kernel, the read-back it waits for, the copy into the geometry buffer) -> sync
Host clocks around work that ends in a synchronise; the two routes alternate step by step on contexts of their own; medians over the timed steps after a warm-up.
`kernel_ms` is the span of HIP events the library records around the build kernel on the stream (crt_debug_tlas_build_ms).
Usage: python tools/tlas_device_cost.py [--steps 200] [--warmup 20] [--out profiles/tlas_device.json]"""
import argparse, ctypes, importlib.util, json, os, sys, tempfile, time, pathlib
os.environ.setdefault("CRT_ENABLE_DEBUG_HOOKS", "1")      # the library reads its diagnostic environment switches only for processes that opt in
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("cpu_ray_tracer_amd", os.path.join(REPO, "cpu-ray-tracer_amd", "__init__.py"))
crt = importlib.util.module_from_spec(spec); spec.loader.exec_module(crt)
sys.path[:0] = [os.path.join(REPO, "tests"), REPO]
import tlas_device_inputs as inp                          # the scenes and transform sets of the tests
A = os.path.join(REPO, "assets")
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200); ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tlas_device.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
med = lambda v: float(sorted(v)[len(v) // 2])


def measure(name, tmp):
    xml = inp.scene_xml(tmp, name)
    T = inp.transforms(name)
    ha, hb = crt.HostScene(xml, 1, A), crt.HostScene(xml, 1, A)
    ca, cb = crt.Context(256, 160), crt.Context(256, 160)
    ha.upload(ca); hb.upload(cb)
    frames = []
    for k in range(4):                                     # four poses: every step moves every instance
        Tk = T.copy(); Tk[:, :3, 3] += np.float32(0.01 * k)
        frames.append(torch.from_numpy(Tk).to(dev))
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    host, device, kernel = [], [], []
    ms = ctypes.c_float()
    for f in range(args.warmup + args.steps):
        t = frames[f % 4]
        t0 = time.perf_counter()
        Th = t.cpu().numpy()
        for i in range(len(Th)):
            ha.set_transform(i, Th[i])
        ha.update(ca, crt.UPDATE_TRANSFORMS); ca.sync()
        t1 = time.perf_counter()
        cb.update_transforms_device(t, stream=st); cb.sync()
        t2 = time.perf_counter()
        cb._ck(cb.L.crt_debug_tlas_build_ms(cb.h, ctypes.byref(ms)))
        if f >= args.warmup:
            host.append((t1 - t0) * 1e3); device.append((t2 - t1) * 1e3); kernel.append(ms.value)
    return dict(set=name, instances=int(len(T)), steps=args.steps, warmup=args.warmup, host_route_ms=med(host), device_route_ms=med(device), kernel_ms=med(kernel),
                host_route_ms_p10_p90=[float(np.percentile(host, 10)), float(np.percentile(host, 90))],
                device_route_ms_p10_p90=[float(np.percentile(device, 10)), float(np.percentile(device, 90))],
                kernel_ms_p10_p90=[float(np.percentile(kernel, 10)), float(np.percentile(kernel, 90))])


with tempfile.TemporaryDirectory() as d:
    out = dict(tool="tools/tlas_device_cost.py", device=torch.cuda.get_device_name(0), results=[measure(n, pathlib.Path(d)) for n in ("tlas3", "ring40", "rand256")])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
for r in out["results"]:
    print("%s (%d instances): host route %.3f ms | device route %.3f ms | build kernel %.3f ms" % (r["set"], r["instances"], r["host_route_ms"], r["device_route_ms"], r["kernel_ms"]))
