"""crt_render_looks / crt_render_looks_device: the frames of many cameras over many job-local looks of the live scene in one render job (csrc/device/look_build.hip,
render_looks.h).  Every comparison is bit for bit (np.array_equal on the bit patterns) against
  the update loop   update_look(look) + set_camera_state + clear + render + accumulator per view, on a SECOND context;
  the fresh loop    HostScene.set_look(look) + upload + the same render per view, on a THIRD context: what a scene uploaded with that look renders;
  the oracle        a scene built with that look (render_looks_inputs.make_oracle).
The scenes, looks, cameras and cases are tests/render_looks_inputs.py's; tests/test_render_looks_cpu.py holds, without a GPU, that every look changes the image, so
a lane that shades with the wrong look or ignores one of its fields cannot pass here."""
import ctypes as C

import numpy as np
import pytest

import render_looks_inputs as li
from conftest import ASSETS, scene_path

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H = li.W, li.H
SENTINEL_F, SENTINEL_U = np.float32(-7.25), np.uint32(0xDEADBEEF)
INVALID, DEVICE, UNSUPPORTED, STATE = -1, -2, -4, -5


def dev():
    return torch.device("cuda", 0)


def to_dev(a, dtype=np.float32):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev())
    torch.cuda.synchronize()
    return t


def looks_to_dev(rec):
    return to_dev(np.ascontiguousarray(rec, np.uint32).view(np.int32), np.int32)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


class Rig:
    """a scene on three contexts — `ctx` takes the entry under test, `ref` runs the update-look loop, `fresh` is uploaded anew per look — and its oracles; every
    reference is computed once and kept unchanged"""

    def __init__(self, crt, orc, scene, width=W, height=H, **cfg):
        self.crt, self.orc, self.scene, self.W, self.H, self.cfg = crt, orc, scene, width, height, cfg
        xml, kind = li.SCENES[scene]
        self.hs, self.hs_fresh = crt.HostScene(scene_path(xml), kind, ASSETS), crt.HostScene(scene_path(xml), kind, ASSETS)
        self.base = crt.look_dicts(self.hs.look())[0]
        self.looks = li.looks(scene, self.base)
        self.rec = {n: crt.look_records([k])[0] for n, k in self.looks.items()}
        self.ctx, self.ref, self.fresh = (crt.Context(width, height, **cfg) for _ in range(3))
        self.hs.upload(self.ctx); self.hs.upload(self.ref)
        self._oracles, self._cache = {}, {}

    def records(self, c):
        return self.crt.camera_records(self.W, self.H, [c.camera(k) for k in range(c.K)])

    def look_array(self, c):
        return np.stack([self.rec[n] for n in c.names])

    def _views(self, c, views, how, render):
        out = []
        for k in (range(c.K) if views is None else views):
            key = (how, c.look_of(k), c.camera(k), c.spp_first, c.frames, c.passes)
            if key not in self._cache:
                a = render(c.look_of(k), c.camera(k)); a.setflags(write=False)
                self._cache[key] = a
            out.append(self._cache[key])
        return np.stack(out)

    def loop(self, c, views=None):
        def render(name, camera):
            self.ref.update_look(self.rec[name])
            self.ref.set_camera_state(*camera); self.ref.clear(); self.ref.render(c.spp_first, c.frames, c.passes)
            return self.ref.accumulator()
        return self._views(c, views, "loop", render)

    def upload_fresh(self, name, ctx=None):
        self.hs_fresh.set_look(self.rec[name]); self.hs_fresh.upload(ctx or self.fresh)

    def fresh_loop(self, c, views=None):
        def render(name, camera):
            self.upload_fresh(name)
            self.fresh.set_camera_state(*camera); self.fresh.clear(); self.fresh.render(c.spp_first, c.frames, c.passes)
            return self.fresh.accumulator()
        return self._views(c, views, "fresh", render)

    def oracle_views(self, c):
        """{view: accumulator} of every view"""
        ks = list(range(c.K))

        def render(name, camera):
            if name not in self._oracles:
                self._oracles[name] = li.make_oracle(self.orc, self.scene, self.looks[name], self.W, self.H)
            return li.oracle_render(self._oracles[name], camera, c.spp_first, c.frames, c.passes)
        return dict(zip(ks, self._views(c, ks, "oracle", render)))

    def run(self, c, ctx=None, **kw):
        return (ctx or self.ctx).render_looks(self.records(c), self.look_array(c), c.spp_first, c.frames, c.passes, view_look=c.view_look, **kw)

    def close(self):
        for x in (self.ctx, self.ref, self.fresh):
            x.close()


@pytest.fixture(scope="module")
def rigs(crt, orc):
    cache = {}

    def get(scene):
        if scene not in cache:
            cache[scene] = Rig(crt, orc, scene)
        return cache[scene]
    yield get
    for r in cache.values():
        r.close()


def raw_looks(ctx, cams, looks, vl, spp_first, frames, passes, scale, acc, px, K=None, L=None):
    """crt_render_looks into arrays the caller has filled"""
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    return ctx.L.crt_render_looks(ctx.h, p(cams), C.c_uint32(len(cams) if K is None else K), p(looks), C.c_uint32(len(looks) if L is None else L), p(vl),
                                  C.c_uint32(spp_first), C.c_uint32(frames), C.c_uint32(passes), C.c_float(scale), p(acc), p(px))


# 1: both loops and the oracle — 65 view-frames (a second window of one lane; lanes of different looks in one wavefront), passes = 2, K != L with repeats and a permutation,
# on a scene of one material and on the one with the most
@pytest.mark.parametrize("name", sorted(li.CASES))
def test_looks_equal_both_loops_and_the_oracle(rigs, name):
    c = li.CASES[name]; r = rigs(c.scene)
    scale = 1.0 / (c.spp_first + c.frames * c.passes)
    acc, px = r.run(c, scale=scale)
    assert acc.shape == (c.K, H, W, 4) and px.shape == (c.K, H, W)
    want = r.loop(c)
    bad = [v for v in range(c.K) if not same(acc[v], want[v])]
    assert not bad, (name, "update-look loop", bad)
    fresh = r.fresh_loop(c)
    bad = [v for v in range(c.K) if not same(acc[v], fresh[v])]
    assert not bad, (name, "fresh-upload loop", bad)
    told = r.oracle_views(c)
    assert len(told) == c.K, name
    bad = [v for v, a in told.items() if not same(acc[v], a)]
    assert not bad, (name, "oracle", bad)
    assert (acc[..., 3].view(np.uint32) == 0).all()                        # w = +0
    r.ref.update_look(r.rec[c.look_of(0)]); r.ref.set_camera_state(*c.camera(0)); r.ref.clear(); r.ref.render(c.spp_first, c.frames, c.passes)
    assert np.array_equal(px[0], r.ref.resolve_screen(scale)[0])
    assert same(r.run(c), acc)                                              # no pixels asked for
    distinct = {acc[v].tobytes() for v in range(c.K)}
    assert len(distinct) == c.K                                             # every view has a camera of its own: no two images are alike


# 2: one look, the live one: the job is crt_render_views'
@pytest.mark.parametrize("scene", sorted(li.SCENES))
def test_one_live_look_equals_render_views(rigs, scene):
    r = rigs(scene)
    c = li.Case(scene, ["base"], [0] * 5, 3, 13, 1)
    acc = r.run(c)
    assert same(acc, r.ctx.render_views(r.records(c), c.spp_first, c.frames, c.passes))
    assert same(acc, r.loop(c))


# 3: the live scene is not changed: its look, its camera, the accumulator, the frames rendered ahead
def test_the_live_scene_is_untouched(crt, orc):
    c = li.CASES["cube_permuted"]
    a, b = Rig(crt, None, c.scene), Rig(crt, None, c.scene)
    cam = c.camera(2)
    a.ctx.set_camera_state(*cam); b.ctx.set_camera_state(*cam)
    light0 = a.ctx.get_light()
    for spp in range(1, 7):
        if spp == 4:
            a.run(c)                                                        # behind three still Ticks: frames are rendered ahead
        pa, ra, ea = a.ctx.tick(spp)
        pb, rb, eb = b.ctx.tick(spp)
        assert np.array_equal(pa, pb) and same(ra, rb) and ea == eb, spp
    assert all(np.array_equal(x, y) for x, y in zip(light0, a.ctx.get_light()))
    a.ctx.clear(); a.ctx.render(1, 2, 1)
    b.ctx.clear(); b.ctx.render(1, 2, 1)
    assert same(a.ctx.accumulator(), b.ctx.accumulator())
    # counters: the job's growth is the loop's
    keys = ("rays", "primary", "mesh_hits")
    a.ctx.sync(); c0 = a.ctx.counters()
    a.run(c)
    a.ctx.sync(); c1 = a.ctx.counters()
    b.ref.sync(); r0 = b.ref.counters()
    b.loop(c)
    b.ref.sync(); r1 = b.ref.counters()
    assert {k: c1[k] - c0[k] for k in keys} == {k: r1[k] - r0[k] for k in keys}
    assert c1["primary"] - c0["primary"] == c.K * c.frames * c.passes * 12 * 256 and c1["mesh_hits"] > c0["mesh_hits"]
    a.close(); b.close()


# 4: the rows the tiling truncates and the tiles the context does not own stay as the caller left them
@pytest.mark.parametrize("own", ["all", "strided"])
def test_ownership_and_truncation(crt, own):
    cfg = dict(tile_first=1, tile_stride=2, tile_count=3) if own == "strided" else {}
    c0 = li.CASES["cube_passes2"]
    r = Rig(crt, None, c0.scene, 48, 40, **cfg)
    c = li.Case(c0.scene, c0.names, None, 1, 2, 1)
    acc = np.full((3, 40, 48, 4), SENTINEL_F, np.float32); px = np.full((3, 40, 48), SENTINEL_U, np.uint32)
    assert raw_looks(r.ctx, r.records(c), r.look_array(c), None, 1, 2, 1, 0.5, acc, px) == 0
    owned = np.zeros((40, 48), bool)
    for t in ([1, 3, 5] if own == "strided" else range(6)):
        owned[16 * (t // 3):16 * (t // 3) + 16, 16 * (t % 3):16 * (t % 3) + 16] = True
    want = r.loop(c)
    for k in range(3):
        assert same(acc[k][owned], want[k][owned]), k
        assert (acc[k][~owned] == SENTINEL_F).all() and (px[k][~owned] == SENTINEL_U).all(), k
        assert (px[k][owned] != SENTINEL_U).all(), k
    r.close()


# 5: the device entry, on a stream that is not the default one
@pytest.mark.parametrize("name", ["cube_5x13", "tlas_permuted"])
def test_device_entry_on_a_side_stream(rigs, name):
    c = li.CASES[name]; r = rigs(c.scene)
    scale = 0.25
    acc, px = r.run(c, scale=scale)
    side = torch.cuda.Stream(device=dev())
    with torch.cuda.stream(side):
        cams = torch.from_numpy(r.records(c)).to(dev()); looks = torch.from_numpy(r.look_array(c).view(np.int32)).to(dev())
        vl = torch.tensor(c.view_look, dtype=torch.int32, device=dev()) if c.view_look is not None else None
        out = torch.full((c.K, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
        pix = torch.full((c.K, H, W), 0x5A5A5A5A, dtype=torch.int32, device=dev())
    got, gpx = r.ctx.render_looks_device(cams, looks, out, c.spp_first, c.frames, c.passes, scale=scale, pixels=pix, view_look=vl, stream=side)
    side.synchronize()
    assert got is out and gpx is pix
    assert same(out.cpu().numpy(), acc) and np.array_equal(pix.cpu().numpy().view(np.uint32), px)
    assert same(acc, r.loop(c))
    out2 = torch.full((c.K, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
    r.ctx.render_looks_device(cams, looks, out2, c.spp_first, c.frames, c.passes, view_look=vl)      # the current (default) stream, no pixels
    torch.cuda.synchronize()
    assert same(out2.cpu().numpy(), acc)


def test_a_job_of_two_launches(crt, rigs):
    c = li.CASES["cube_5x13"]; r = rigs(c.scene)
    uncut = r.run(c, scale=0.5)
    cut = crt.Context(W, H, max_frames_per_launch=64)                        # one window of 64 view-frames per launch: view 4 straddles the two
    r.hs.upload(cut)
    got = r.run(c, ctx=cut, scale=0.5)
    assert same(got[0], uncut[0]) and np.array_equal(got[1], uncut[1])
    cut.close()


# 6: every refusal, the outputs' sentinel intact
def test_refusals_leave_the_outputs_alone(rigs, crt):
    c = li.CASES["tlas_permuted"]; r = rigs(c.scene); ctx = r.ctx; L = ctx.L
    k, n = c.K, len(c.names)
    cams_h, looks_h = r.records(c), r.look_array(c)
    cams, looks = to_dev(cams_h), looks_to_dev(looks_h)
    out = torch.full((k * H * W * 4 + 4,), float(SENTINEL_F), dtype=torch.float32, device=dev())
    vl = to_dev(c.view_look, np.int32)
    host_out = np.zeros((k, H, W, 4), np.float32)
    ntex = 3

    def call(d_cams, d_looks, d_out, c_=ctx, kk=k, nl=n, d_vl=vl.data_ptr(), frames=1, passes=1, stream=None):
        return L.crt_render_looks_device(c_.h, C.c_void_p(d_cams), C.c_uint32(kk), C.c_void_p(d_looks), C.c_uint32(nl), C.c_void_p(d_vl), C.c_uint32(1), C.c_uint32(frames),
                                         C.c_uint32(passes), C.c_float(1.0), C.c_void_p(d_out), None, stream)
    a, t, o = cams.data_ptr(), looks.data_ptr(), out.data_ptr()
    assert call(a, t, o, nl=0) == INVALID                                    # L = 0
    assert call(a, t, o, d_vl=None) == INVALID and b"must equal K" in L.crt_last_error(ctx.h)      # view_look NULL with K != L
    assert call(a, t, o, nl=3) == INVALID and b"view_look[0]" in L.crt_last_error(ctx.h)           # an entry (3) outside [0, 3): found by the build launch
    assert call(a, t, o, passes=0) == INVALID and call(a, t, o, passes=5) == INVALID
    assert call(a, t, host_out.ctypes.data) == INVALID                       # host pointers to the device entry
    assert call(cams_h.ctypes.data, t, o) == INVALID
    assert call(a, looks_h.ctypes.data, o) == INVALID and b"host pointer" in L.crt_last_error(ctx.h)
    assert call(a, t, o, d_vl=np.zeros(k, np.int32).ctypes.data) == INVALID
    assert call(a, t, o + 4) == INVALID and b"16-byte" in L.crt_last_error(ctx.h)
    assert call(a, t + 2, o) == INVALID                                      # misaligned
    assert call(None, t, o) == INVALID and call(a, None, o) == INVALID and call(a, t, None) == INVALID
    assert call(a, t, o, kk=1 << 16, frames=1 << 16) == UNSUPPORTED          # more than 2^31-1 view-frames
    assert call(a, t, o, nl=1 << 25) == UNSUPPORTED and b"4 GiB" in L.crt_last_error(ctx.h)
    assert call(None, None, None, kk=0, nl=0, d_vl=None) == 0 and call(None, None, None, frames=0) == 0 and call(None, None, None, kk=0, nl=0, passes=9) == INVALID
    # a bad texture index in look 3 of a device buffer: the build launch finds it, whether a view uses the look or not
    for field, word, value in (("material 1: texture", 36 + 6 * 1 + 5, ntex), ("material 2: texture", 36 + 6 * 2 + 5, -2), ("floorTexture", 33, -1), ("skyTexture", 34, ntex)):
        bad = looks_h.copy(); bad.view(np.int32)[3, word] = value
        for view_look in (c.view_look, [0, 1, 1, 0, 2, 2]):
            assert call(a, looks_to_dev(bad).data_ptr(), o, d_vl=to_dev(view_look, np.int32).data_ptr()) == INVALID
            msg = L.crt_last_error(ctx.h).decode()
            assert "look 3" in msg and field in msg and "crt_render_looks_device" in msg, msg
        acc = np.full((k, H, W, 4), SENTINEL_F, np.float32)                  # ... and the host entry, on the host
        assert raw_looks(ctx, cams_h, bad, np.array(c.view_look, np.int32), 1, 1, 1, 1.0, acc, None) == INVALID
        msg = L.crt_last_error(ctx.h).decode()
        assert "look 3" in msg and field in msg and (acc == SENTINEL_F).all(), msg
    two = looks_h.copy(); two.view(np.int32)[1, 34] = 7; two.view(np.int32)[2, 33] = 7; two.view(np.int32)[1, 36 + 5] = 7
    assert call(a, looks_to_dev(two).data_ptr(), o) == INVALID               # several: the lowest look, and in it the first field
    assert b"look 1: skyTexture" in L.crt_last_error(ctx.h)
    # the host entry's own: NULL buffers, view_look looked at before anything runs
    acc = np.full((k, H, W, 4), SENTINEL_F, np.float32)
    assert raw_looks(ctx, cams_h, looks_h, np.array([0, 4, 1, 0, 2, 3], np.int32), 1, 1, 1, 1.0, acc, None) == INVALID and b"view_look[1] = 4" in L.crt_last_error(ctx.h)
    assert raw_looks(ctx, cams_h, looks_h, np.array(c.view_look, np.int32), 1, 1, 1, 1.0, None, None) == INVALID
    assert raw_looks(ctx, cams_h, looks_h, None, 1, 1, 1, 1.0, acc, None) == INVALID
    assert raw_looks(ctx, cams_h, looks_h, np.array(c.view_look, np.int32), 1, 0, 1, 1.0, acc, None) == 0 and (acc == SENTINEL_F).all()
    # another accelerator selected
    hs = crt.HostScene(scene_path(li.SCENES[c.scene][0]), 1, ASSETS); hs.build_alt(crt.ACCEL_KDTREE)
    kd = crt.Context(W, H); hs.upload(kd); hs.upload_alt(kd, crt.ACCEL_KDTREE); kd.set_render_accel(crt.ACCEL_KDTREE)
    assert call(a, t, o, c_=kd) == UNSUPPORTED
    kd.set_render_accel(0)
    assert call(a, t, o, c_=kd) == 0                                         # ... and with the BVH selected again the job runs
    torch.cuda.synchronize()
    assert same(out.cpu().numpy()[:k * H * W * 4].reshape(k, H, W, 4), r.loop(c))
    out.fill_(float(SENTINEL_F)); torch.cuda.synchronize()
    kd.close()
    # no scene; a PrimitiveScene
    fresh = crt.Context(W, H)
    assert call(a, t, o, c_=fresh) == STATE
    fresh.close()
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(0.0)
    pc = crt.Context(W, H); ps.upload(pc)
    assert call(a, t, o, c_=pc) == UNSUPPORTED
    pc.close()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL_F).all() and not host_out.any() and (acc == SENTINEL_F).all()
    assert same(r.run(c), r.loop(c))                                         # the context takes the next job as usual
