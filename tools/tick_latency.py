"""Per-Tick latency at 1280x720 (bunny, two-level scene): crt_render latency by frames per call, and the Tick of the reference's Tick loop
three ways — the plain three calls (crt_render(spp, 1) + crt_read_accumulator + crt_resolve_screen), crt_tick, and the facade's Renderer::Tick
(which calls crt_tick).  Prints one line per figure; with a path argument also writes them as JSON (profiles/tick_ahead.json)."""
import importlib.util, json, os, sys, time, numpy as np
os.environ.setdefault("CRT_ENABLE_DEBUG_HOOKS", "1")      # the library reads its diagnostic environment switches only for processes that opt in
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("cpu_ray_tracer_amd", os.path.join(REPO, "cpu-ray-tracer_amd", "__init__.py"))
crt = importlib.util.module_from_spec(spec); spec.loader.exec_module(crt)
A = os.path.join(REPO, "assets")
W, H = 1280, 720
TGT = (0.0, 0.0, 0.0)


def ms(f):
    t0 = time.perf_counter(); f(); return (time.perf_counter() - t0) * 1e3


def plain(ctx, spp, acc=True):
    ctx.render(spp, 1, 1)
    if acc:
        ctx.accumulator()
    ctx.resolve_screen(float(np.float32(1) / np.float32(spp + 1)))


def cam(i):
    return (0.01 * (i % 50), 0.05, -2.0 - 0.005 * (i % 40))


out = {}
for xml, kind in [("bunny_scene.xml", 0), ("tlas_scene.xml", 1)]:
    name = xml.split("_")[0]
    sc = crt.HostScene(os.path.join(A, "scenes", xml), kind, A)
    ctx = crt.Context(W, H); sc.upload(ctx)
    for frames in (1, 4, 16, 64):
        ts = []
        for i in range(6):
            t0 = time.perf_counter(); ctx.render(1 + i * frames, frames, 1); ctx.sync(); ts.append((time.perf_counter() - t0) * 1e3)
        print(xml, "frames per call", frames, "latency ms %.2f" % np.median(ts[1:]))
    r = {}
    pc = crt.Context(W, H); sc.upload(pc)                    # the plain three calls
    tc = crt.Context(W, H); sc.upload(tc)                    # crt_tick
    for c in (pc, tc):                                       # warm: probe, tuner, pool
        c.set_camera_state(cam(0), TGT)
        for s in range(1, 4):
            plain(c, s) if c is pc else c.tick(s)
    spp = 10
    # the moving-camera Tick (and the first Tick after a camera change): the camera differs every Tick
    for key, c, f in (("plain", pc, lambda c, s: plain(c, s)), ("crt_tick", tc, lambda c, s: c.tick(s))):
        ts = []
        for i in range(1, 31):
            c.set_camera_state(cam(i), TGT); c.clear()
            ts.append(ms(lambda: f(c, spp + i)))
        r["moving_%s_ms" % key] = float(np.median(ts[5:]))
        r["first_after_camera_change_%s_ms" % key] = float(np.median(ts))
    # a still camera: primed crt_tick (pixels + energy; + accumulator), plain Tick, 640 Ticks wall
    spp = 1000
    tc.set_camera_state(cam(99), TGT); pc.set_camera_state(cam(99), TGT)
    for i in range(100):
        tc.tick(spp, 1, accumulator=False); spp += 1
    r["primed_crt_tick_pixels_energy_ms"] = float(np.median([ms(lambda s=spp + i: tc.tick(s, 1, accumulator=False)) for i in range(50)])); spp += 50
    r["primed_crt_tick_with_accumulator_ms"] = float(np.median([ms(lambda s=spp + i: tc.tick(s, 1)) for i in range(50)])); spp += 50
    r["still_plain_ms"] = float(np.median([ms(lambda s=spp + i: plain(pc, s)) for i in range(20)]))
    # the first Tick after a discard that follows 100 still Ticks, with the render-ahead stream at low and at normal priority
    for prio in ("low", "normal"):
        if prio == "normal":
            os.environ["CRT_AHEAD_NORMAL_PRIORITY"] = "1"
        ts = []
        for rep in range(5):
            tc.set_camera_state(cam(200 + rep), TGT)
            for i in range(100):
                tc.tick(spp, 1, accumulator=False); spp += 1
            tc.set_camera_state(cam(300 + rep), TGT)
            ts.append(ms(lambda: tc.tick(spp))); spp += 1
        r["first_after_discard_%s_priority_ms" % prio] = float(np.median(ts))
        os.environ.pop("CRT_AHEAD_NORMAL_PRIORITY", None)
    # facade: Renderer::Tick (crt_tick with the accumulator) primed, and 640 back-to-back still Ticks
    fr = crt.HostRenderer(sc, W, H); fr.init()
    for _ in range(3):
        fr.tick(0.0)
    t0 = time.perf_counter()
    for _ in range(640):
        fr.tick(0.0)
    r["facade_640_still_ticks_s"] = time.perf_counter() - t0
    r["facade_primed_tick_ms"] = float(np.median([ms(lambda: fr.tick(0.0)) for _ in range(50)]))
    t = fr.context().timing()
    r["facade_render_launches_693_ticks"] = int(t["render_launches"])
    t0 = time.perf_counter()
    for i in range(640):
        plain(pc, 5000 + i)
    r["plain_640_still_ticks_s"] = time.perf_counter() - t0
    for k, v in r.items():
        print(name, k, "%.3f" % v if isinstance(v, float) else v)
    out[name] = r
    for c in (ctx, pc, tc):
        c.close()
    fr.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump({"width": W, "height": H, "results": out}, f, indent=1)
