"""The shading queries on the GPU (crt_abi.h "scene queries"): crt_get_hit_info / crt_get_hit_info_device, crt_get_sky_color / _device, crt_get_light.

The yardstick is tests/hit_info_restate.py (numpy float32), which tests/test_hit_info_cpu.py pins to the oracle's Whitted image and sky on the CPU.  Every
comparison here is == on the uint32 view of the records.  The hit records fed in are the ORACLE's (o.find_nearest) unless a test says otherwise, so these tests
do not lean on the find-nearest kernels.  No test hands a kernel an index that could leave its buffers: the refusals below all stop on the host."""
import ctypes as C

import numpy as np
import pytest

import hit_info_restate as hr
from conftest import ASSETS, scene_path
from test_gpu_scene_queries import camera_rays, up_rays, unit, ray_records, shadow_records, rigid
from test_hit_info_cpu import W, H, CAMERA, whitted_xml, load, primary_rays, check_image_conditions, assemble, sky_directions, oracle_sky, bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = {"bunny": ("bunny_scene.xml", 0), "tower": ("tower_scene.xml", 0), "tlas": ("tlas_scene.xml", 1)}
N_RAYS = 1 << 16
FIELDS = ("I", "material", "N", "u", "albedo", "v")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def ray_set(o, light, n=N_RAYS, seed=5):
    """camera rays over a window that holds the meshes, the floor, the sky and the light; rays from below aimed up at the light's plane; and bounce rays that
    start just in front of / just behind the camera rays' mesh hits in random directions (the ones from behind meet the surfaces from inside).  inside on half."""
    n1, n2 = 26000, 10000
    Oa, Da = camera_rays(n1 // 2, seed, cam=(0.0, 0.5, -3.0), half=(2.6, 2.7))            # wide: floor, sky, the light
    Ob, Db = camera_rays(n1 - n1 // 2, seed + 3, cam=(0.0, 0.5, -3.0), half=(1.3, 0.9))   # narrow: the meshes
    O1, D1 = np.concatenate([Oa, Ob]), np.concatenate([Da, Db])
    O2, D2 = up_rays(n2, seed + 1, light, (-2.0, 2.0), (1.0, 5.0), -0.9, 2.0, spread=0.8)
    h1 = o.find_nearest(O1, D1)
    m = np.flatnonzero(h1["objIdx"] >= 2)
    assert len(m) >= 1000
    rng = np.random.default_rng(seed + 2)
    k = n - n1 - n2
    pick = m[rng.integers(0, len(m), k)]
    I = (O1[pick] + h1["t"][pick, None] * D1[pick]).astype(np.float32)
    side = np.where(np.arange(k) % 2 == 0, np.float32(-1e-3), np.float32(1e-3))[:, None]
    O3 = (I + side * D1[pick]).astype(np.float32)
    D3 = unit(rng.normal(size=(k, 3)))
    O = np.concatenate([O1, O2, O3]); D = np.concatenate([D1, D2, D3])
    return O, D, (np.arange(n) % 2).astype(np.int32)


_cases = {}


def record_case(orc, name):
    """(o, sh, O, D, inside, oracle hits, restated records) of a scene, its conditions asserted; built once per session"""
    if name in _cases:
        return _cases[name]
    xml, kind = CASES[name]
    o, sh = load(orc, scene_path(xml), kind)
    O, D, inside = ray_set(o, tuple(float(v) for v in sh.light))
    hits = o.find_nearest(O, D, inside)
    want, flip = sh.hit_info(O, D, hits, with_flip=True)
    obj = hits["objIdx"]
    counts = dict(light=int((obj == 0).sum()), floor=int((obj == 1).sum()), mesh=int((obj >= 2).sum()), miss=int((obj == -1).sum()))
    assert min(counts.values()) >= 500, counts
    if kind == 1:
        per_blas = [int((obj == 2 + b).sum()) for b in range(o.bvh_count())]
        assert min(per_blas) >= 500, per_blas
        assert len(set(want["material"][obj >= 2])) == 3
    assert (flip & (obj >= 2)).sum() >= 100 and (~flip & (obj >= 2)).sum() >= 100
    _cases[name] = (o, sh, O, D, inside, hits, want)
    return _cases[name]


def product(crt, name, W_=64, H_=64):
    xml, kind = CASES[name]
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    ctx = crt.Context(W_, H_)
    hs.upload(ctx)
    return hs, ctx


def hit_records(crt, hits):
    h = np.ascontiguousarray(hits, crt.HIT_DTYPE)
    return torch.from_numpy(h.view(np.float32).reshape(-1, 7).copy()).to(torch.device("cuda", 0))


def info_np(crt, t):
    return t.cpu().numpy().view(crt.HIT_INFO_DTYPE).reshape(-1)


def assert_info_equal(got, want, what):
    for f in FIELDS:
        a, b = bits(got[f]), bits(want[f])
        assert np.array_equal(a, b), (what, f, int((a != b).reshape(len(got), -1).any(axis=1).sum()))


def raw_get_hit_info(crt, ctx, O, D, hits, out):
    rays = np.zeros(len(O), crt.RAY_DTYPE); rays["O"], rays["D"] = O, D
    h = np.ascontiguousarray(hits, crt.HIT_DTYPE)
    return ctx.L.crt_get_hit_info(ctx.h, rays.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_size_t(len(O)))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 1. records == the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_records_equal_the_restatement(crt, orc, name):
    o, sh, O, D, inside, hits, want = record_case(orc, name)
    hs, ctx = product(crt, name)
    c0 = ctx.counters()
    got = ctx.get_hit_info(O, D, hits)
    assert_info_equal(got, want, "host entry")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d = ctx.get_hit_info_device(ray_records(O, D, inside), hit_records(crt, hits))
    side.synchronize()
    assert_info_equal(info_np(crt, d), want, "device entry")
    # the default stream too (the binding's side stream), a short batch and a single record
    assert_info_equal(info_np(crt, ctx.get_hit_info_device(ray_records(O[:100], D[:100]), hit_records(crt, hits[:100]))), want[:100], "default stream")
    assert_info_equal(ctx.get_hit_info(O[77:78], D[77:78], hits[77:78]), want[77:78], "one record")
    assert len(ctx.get_hit_info(O[:0], D[:0], hits[:0])) == 0
    assert ctx.counters() == c0                                           # the shading queries count nothing
    pos, col = ctx.get_light()
    assert np.array_equal(pos, sh.light_pos()) and np.array_equal(col, np.float32([24, 24, 22]))
    ctx.close(); hs.close()


def test_records_of_alt_accelerator_hits(crt, orc):
    """hit records of the KD-tree / grid entries fed straight in: the query does not depend on the accelerator that produced the hit.  The records fed in are
    the product's own here (find_nearest_alt, checked against the restatements of those walks elsewhere); the expected hit info is restated from those same records."""
    for name in ("bunny", "tlas"):
        o, sh, O, D, inside, _, _ = record_case(orc, name)
        hs, ctx = product(crt, name)
        for code in (crt.ACCEL_KDTREE, crt.ACCEL_GRID):
            hs.build_alt(code); hs.upload_alt(ctx, code)
            hits = ctx.find_nearest_alt(code, O, D)
            assert (hits["objIdx"] >= 2).sum() >= 500
            want = sh.hit_info(O, D, hits)
            assert_info_equal(ctx.get_hit_info(O, D, hits), want, (name, code, "host"))
            ctx.set_render_accel(code)                                    # ... nor on crt_set_render_accel
            d = ctx.get_hit_info_device(ray_records(O, D), hit_records(crt, hits), stream=torch.cuda.Stream())
            torch.cuda.synchronize()
            assert_info_equal(info_np(crt, d), want, (name, code, "device"))
            ctx.set_render_accel(0)
        ctx.close(); hs.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 2. sky
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_sky_equals_oracle(crt, orc):
    o, sh = load(orc, scene_path("bunny_scene.xml"))
    O, D = sky_directions()
    want = oracle_sky(o, O, D)
    hs, ctx = product(crt, "bunny")
    c0 = ctx.counters()
    assert np.array_equal(bits(ctx.get_sky_color(D)), bits(want))
    d = ctx.get_sky_color_device(O=torch.from_numpy(O).cuda(), D=torch.from_numpy(D).cuda(), stream=torch.cuda.Stream())
    torch.cuda.synchronize()
    assert np.array_equal(bits(d.cpu().numpy()), bits(want))
    assert ctx.counters() == c0
    ctx.close(); hs.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 3. the Whitted renderer's Trace written outside the library, on device tensors
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bunny", "cube", "tower_small", "tower"])
def test_whitted_from_device_queries_equals_oracle(crt, orc, tmp_path, name):
    """find_nearest_device, get_hit_info_device and is_occluded_device on one non-default stream, one read-back, then Trace's float32 arithmetic in numpy.
    The shadow rays are DirectIllumination's, formed in numpy float32 from the restated records of the oracle's hits and uploaded beforehand; the records read
    back must equal those bit for bit (asserted), so they are the shadow rays of the device's own records.  tower_scene.xml needs no condition on the scene
    here: the occlusion comes from the device query."""
    xml = whitted_xml(name, tmp_path)
    o, sh = load(orc, xml)
    o.renderer_init(W, H); o.set_camera_state(*CAMERA)
    O, D = primary_rays(o)
    ohits = o.find_nearest(O, D)
    check_image_conditions(ohits)
    restated = sh.hit_info(O, D, ohits)
    org, L, t, _, _ = hr.shadow_rays(restated, sh.light_pos())
    hs = crt.HostScene(xml, 0, ASSETS)
    ctx = crt.Context(W, H)
    hs.upload(ctx); ctx.set_camera_state(*CAMERA)
    rays = ray_records(O, D)
    with np.errstate(all="ignore"):
        finite = np.isfinite(org).all(axis=1) & np.isfinite(L).all(axis=1) & np.isfinite(t)
    srays = shadow_records(np.where(finite[:, None], org, 0).astype(np.float32), np.where(finite[:, None], L, [0, 1, 0]).astype(np.float32), np.where(finite, t, 0).astype(np.float32))
    st = torch.cuda.Stream()
    hits = ctx.find_nearest_device(rays, stream=st)
    info = ctx.get_hit_info_device(rays, hits, stream=st)
    occ = ctx.is_occluded_device(srays, stream=st)
    with torch.cuda.stream(st):
        back = torch.cat([info, occ.view(torch.float32).reshape(-1, 1)], 1).cpu()       # the one read-back
    info_h = np.ascontiguousarray(back[:, :12].numpy()).view(crt.HIT_INFO_DTYPE).reshape(-1)
    occ_h = np.ascontiguousarray(back[:, 12].numpy()).view(np.int32) != 0
    assert_info_equal(info_h, restated, "records of the device's own hits")
    assert finite[info_h["material"] >= 1].all()
    img = assemble(sh, O, D, None, info_h, lambda a, b, c: occ_h)
    o.whitted()
    want = o.accumulator()
    bad = (bits(img) != bits(want)).any(axis=2)
    assert not bad.any(), ("pixels that differ from the oracle", int(bad.sum()), np.argwhere(bad)[:5].tolist())
    # agreement of two product paths: the library's own Whitted Tick
    ctx.whitted_tick()
    assert np.array_equal(bits(ctx.accumulator()), bits(img))
    ctx.close(); hs.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 4. ordering
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_ordering_across_update_and_upload(crt, orc):
    o, sh, O, D, inside, hits0, want0 = record_case(orc, "tlas")
    o2, sh2 = load(orc, scene_path("tlas_scene.xml"), 1)                  # a second oracle: the session's case keeps its transforms
    T0 = o2.blas_transform(0)[0].reshape(4, 4)
    T1 = rigid(0.6, T0[:3, 3] + np.array([0.25, 0.1, -0.2], np.float32))
    o2.set_transform(0, T1); sh2.refresh_transforms(o2)
    hits1 = o2.find_nearest(O, D, inside)
    want1 = sh2.hit_info(O, D, hits1)
    moved = (hits1["objIdx"] == 2)
    assert moved.sum() >= 1000 and not np.array_equal(bits(want1["N"][moved & (hits0["objIdx"] == 2)]), bits(want0["N"][moved & (hits0["objIdx"] == 2)]))
    hs, ctx = product(crt, "tlas")
    r, h0, h1 = ray_records(O, D, inside), hit_records(crt, hits0), hit_records(crt, hits1)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    first = [ctx.get_hit_info_device(r, h0, stream=s1) for _ in range(4)]
    hs.set_transform(0, T1)
    hs.update(ctx, crt.UPDATE_TRANSFORMS)                                 # ordered behind the queries in flight; no host wait
    second = ctx.get_hit_info_device(r, h1, stream=s2)
    torch.cuda.synchronize()
    for f in first:
        assert_info_equal(info_np(crt, f), want0, "before the update")
    assert_info_equal(info_np(crt, second), want1, "after the update")
    # a different scene uploaded into the same context
    ob, shb, Ob, Db, insb, hitsb, wantb = record_case(orc, "bunny")
    pending = ctx.get_hit_info_device(r, h1, stream=s1)                   # crt_upload_scene waits for it before the buffers go
    hb = crt.HostScene(scene_path("bunny_scene.xml"), 0, ASSETS)
    hb.upload(ctx)
    d = ctx.get_hit_info_device(ray_records(Ob, Db, insb), hit_records(crt, hitsb), stream=s2)
    torch.cuda.synchronize()
    assert_info_equal(info_np(crt, pending), want1, "in flight across the upload")
    assert_info_equal(info_np(crt, d), wantb, "after the upload")
    ctx.close(); hs.close(); hb.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 5. refusals: all on paths that validate on the host and launch nothing
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(crt, orc):
    for name in ("bunny", "tlas"):
        o, sh, O, D, inside, hits, want = record_case(orc, name)
        hs, ctx = product(crt, name)
        objects = sh.objects
        mesh = int(np.flatnonzero(hits["objIdx"] >= 2)[0])
        tri_count = len(sh.tris[hits["objIdx"][mesh] - 2 if CASES[name][1] == 1 else 0])
        for field, value, at in (("objIdx", objects + 2, 5), ("objIdx", -2, 5), ("triIdx", tri_count, mesh), ("triIdx", -1, mesh)):
            bad = hits[:200].copy(); bad[field][at] = value
            out = np.full(200 * 12, 0xABABABAB, np.uint32)
            assert raw_get_hit_info(crt, ctx, O[:200], D[:200], bad, out) == -1, (field, value)
            assert ("record %d " % at) in ctx.L.crt_last_error(ctx.h).decode()
            assert (out == 0xABABABAB).all()
        # the largest indices the scene does have pass
        okay = hits[:200].copy(); okay["triIdx"][mesh] = tri_count - 1
        out = np.zeros(200 * 12, np.uint32)
        assert raw_get_hit_info(crt, ctx, O[:200], D[:200], okay, out) == 0
        # device entry: a host pointer, a misaligned output
        r, h = ray_records(O[:200], D[:200]), hit_records(crt, hits[:200])
        host_out = np.zeros(200 * 12, np.float32)
        assert ctx.L.crt_get_hit_info_device(ctx.h, C.c_void_p(r.data_ptr()), C.c_void_p(h.data_ptr()), host_out.ctypes.data_as(C.c_void_p), C.c_size_t(200), None) == -1
        dev_out = torch.zeros(200 * 12 + 4, dtype=torch.float32, device="cuda")
        assert dev_out.data_ptr() % 16 == 0
        assert ctx.L.crt_get_hit_info_device(ctx.h, C.c_void_p(r.data_ptr()), C.c_void_p(h.data_ptr()), C.c_void_p(dev_out.data_ptr() + 4), C.c_size_t(200), None) == -1
        assert "16-byte aligned" in ctx.L.crt_last_error(ctx.h).decode()
        torch.cuda.synchronize()
        assert not dev_out.any()
        assert ctx.L.crt_get_hit_info_device(ctx.h, C.c_void_p(r.data_ptr()), C.c_void_p(h.data_ptr()), C.c_void_p(dev_out.data_ptr()), C.c_size_t(1 << 31), None) == -4
        ctx.close(); hs.close()
    o, sh, O, D, inside, hits, want = record_case(orc, "bunny")
    empty = crt.Context(64, 64)                                           # no scene
    with pytest.raises(crt.CrtError) as e:
        empty.get_hit_info(O[:10], D[:10], hits[:10])
    assert e.value.code == -5
    with pytest.raises(crt.CrtError) as e:
        empty.get_sky_color(D[:10])
    assert e.value.code == -5
    with pytest.raises(crt.CrtError) as e:
        empty.get_light()
    assert e.value.code == -5
    ps = crt.HostPrimitiveScene(ASSETS)                                   # the PrimitiveScene: a (black) sky, no hit info
    ps.upload(empty)
    with pytest.raises(crt.CrtError) as e:
        empty.get_hit_info(O[:10], D[:10], hits[:10])
    assert e.value.code == -4
    with pytest.raises(crt.CrtError) as e:
        empty.get_hit_info_device(ray_records(O[:10], D[:10]), hit_records(crt, hits[:10]))
    assert e.value.code == -4
    assert not ctx_sky_any(empty, D[:300])
    empty.close(); ps.close()


def ctx_sky_any(ctx, D):
    host = ctx.get_sky_color(D)
    dev = ctx.get_sky_color_device(D=torch.from_numpy(D).cuda(), O=torch.zeros((len(D), 3), dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    return bool(host.any()) or bool(dev.any().item())


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 6. crt_tick's render-ahead is not disturbed
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_tick_sequence_still_renders_ahead(crt, orc):
    """a hit-info and a sky query between the Ticks of a still sequence: the same pictures and exactly as many render launches as the same sequence without
    them (frames rendered ahead keep being used; told apart by the launch count, as tests/test_gpu_tick_ahead.py does)"""
    o, sh, O, D, inside, hits, want = record_case(orc, "bunny")
    Wt, Ht = 128, 80
    hs, ctx = product(crt, "bunny", Wt, Ht)
    twin = crt.Context(Wt, Ht); hs.upload(twin)
    for k in range(1, 131):
        a, b = ctx.tick(k), twin.tick(k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], k
        if k in (40, 90):
            assert_info_equal(ctx.get_hit_info(O[:4096], D[:4096], hits[:4096]), want[:4096], k)
            ctx.get_sky_color(D[:4096])
            d = ctx.get_hit_info_device(ray_records(O[:4096], D[:4096]), hit_records(crt, hits[:4096]), stream=torch.cuda.Stream())
            torch.cuda.synchronize()
            assert_info_equal(info_np(crt, d), want[:4096], k)
    la, lb = ctx.timing()["render_launches"], twin.timing()["render_launches"]
    assert la == lb and la <= 10, (la, lb)
    ctx.close(); twin.close(); hs.close()
