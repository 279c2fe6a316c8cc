"""crt_render_shapes / crt_render_shapes_device: the frames of many cameras over many job-local shapes of one refitted BVH in one render job
(csrc/device/shape_build.hip, render_shapes.h, tlas_build.hip's per-shape build).  Every comparison is bit for bit (np.array_equal on the uint32 views) against
  the loop    refit_device(bvh, positions[s]) (+ update_transforms_device(T[s])) + set_camera_state + clear + render + accumulator per view, through the existing
              entries, on a SECOND context;
  the oracle  move_and_refit (+ set_transform for every instance), set_camera_state, render.
The scenes, shapes and cameras are tests/render_shapes_inputs.py's; tests/test_render_shapes_cpu.py holds, without a GPU, that every camera sees the deforming mesh,
that no two views of a case are alike and that a refit does not depend on the one before, so a lane that walks the wrong image cannot pass here."""
import ctypes as C

import numpy as np
import pytest

import render_shapes_inputs as si
import tlas_device_inputs as inp
from conftest import ASSETS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H = si.W, si.H
SENTINEL_F, SENTINEL_U = np.float32(-7.25), np.uint32(0xDEADBEEF)
INVALID, DEVICE, UNSUPPORTED, STATE = -1, -2, -4, -5


def dev():
    return torch.device("cuda", 0)


def to_dev(a, dtype=np.float32):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev())
    torch.cuda.synchronize()
    return t


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


class Rig:
    """a scene on two contexts — `ctx` takes the entry, `ref` runs the loop — and its oracle; every reference is computed once and kept unchanged"""

    def __init__(self, crt, orc, tmp, scene, width=W, height=H, **cfg):
        self.crt, self.W, self.H = crt, width, height
        self.xml, self.kind = si.scene_xml(tmp, scene)
        self.hs = crt.HostScene(self.xml, self.kind, ASSETS)
        self.ctx, self.ref = crt.Context(width, height, **cfg), crt.Context(width, height, **cfg)
        self.hs.upload(self.ctx); self.hs.upload(self.ref)
        self.o = si.make_oracle(orc, tmp, scene, width, height) if orc is not None else None
        self._loop, self._oracle = {}, {}

    def case(self, name, **kw):
        return si.case(name, self.hs, **kw)

    def records(self, cameras):
        return self.crt.camera_records(self.W, self.H, cameras)

    def _key(self, c, k):
        s = c.shape_of(k)
        return (c.bvh, c.pos[s].tobytes(), None if c.T is None else c.T[s].tobytes(), c.cameras[k], c.spp_first, c.frames, c.passes)

    def loop(self, c, views=None, scale=None):
        """(accumulators, pixels or None, {shape: box}, {shape: nodes}) of the views through the existing entries on `ref`"""
        acc, px, boxes, nodes = [], [], {}, {}
        for k in (range(len(c.cameras)) if views is None else views):
            s = c.shape_of(k)
            key = self._key(c, k) + (scale,)
            if key not in self._loop:
                box = self.ref.refit_device(c.bvh, to_dev(c.pos[s]))
                n = self.ref.update_transforms_device(to_dev(c.T[s])) if c.T is not None else None
                self.ref.set_camera_state(*c.cameras[k]); self.ref.clear(); self.ref.render(c.spp_first, c.frames, c.passes)
                a = self.ref.accumulator(); a.setflags(write=False)
                self._loop[key] = (a, self.ref.resolve_screen(scale)[0] if scale is not None else None, box, n)
            a, x, box, n = self._loop[key]
            acc.append(a); px.append(x); boxes[s] = box; nodes[s] = n
        return np.stack(acc), (np.stack(px) if scale is not None else None), boxes, nodes

    def oracle(self, c, views=None):
        out = []
        for k in (range(len(c.cameras)) if views is None else views):
            key = self._key(c, k)
            if key not in self._oracle:
                a = si.oracle_view(self.o, c, k)[0]; a.setflags(write=False)
                self._oracle[key] = a
            out.append(self._oracle[key])
        return np.stack(out)

    def run(self, c, ctx=None, **kw):
        T = None if c.T is None else c.T.reshape(len(c.T), -1, 16)
        return (ctx or self.ctx).render_shapes(self.records(c.cameras), c.bvh, c.pos, c.spp_first, c.frames, c.passes, T=T, view_shape=c.view_shape, **kw)

    def close(self):
        self.ctx.close(); self.ref.close()


@pytest.fixture(scope="module")
def rigs(crt, orc, tmp_path_factory):
    cache, tmp = {}, tmp_path_factory.mktemp("shapes")

    def get(scene):
        if scene not in cache:
            cache[scene] = Rig(crt, orc, tmp, scene)
        return cache[scene]
    yield get
    for r in cache.values():
        r.close()


def raw_shapes(ctx, cams, bvh, pos, T, vs, spp_first, frames, passes, scale, acc, px, boxes=None, nodes=None, S=None, tris=None, n=None, K=None):
    """crt_render_shapes into arrays the caller has filled"""
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    return ctx.L.crt_render_shapes(ctx.h, p(cams), C.c_uint32(len(cams) if K is None else K), C.c_uint32(bvh), p(pos), C.c_uint32(len(pos) if S is None else S),
                                   C.c_uint32(pos.shape[1] if tris is None else tris), p(T), C.c_uint32((0 if T is None else T.shape[1]) if n is None else n), p(vs),
                                   C.c_uint32(spp_first), C.c_uint32(frames), C.c_uint32(passes), C.c_float(scale), p(acc), p(px), p(boxes), p(nodes))


def check_against_loop_and_oracle(r, c, name, full=True):
    scale = 1.0 / (c.spp_first + c.frames * c.passes)
    tlas = c.T is not None
    got = r.run(c, scale=scale, want_root_boxes=True, want_tlas=tlas)
    acc, px, boxes = got[0], got[1], got[-1]
    k, S = len(c.cameras), len(c.pos)
    assert acc.shape == (k, H, W, 4) and px.shape == (k, H, W) and boxes.shape == (S, 2, 3)
    want, want_px, want_boxes, want_nodes = r.loop(c, scale=scale)
    bad = [v for v in range(k) if not same(acc[v], want[v])]
    assert not bad, (name, "loop", bad[:8])
    assert np.array_equal(px, want_px)
    for s, b in want_boxes.items():
        assert same(boxes[s], b), (name, "root box", s)
    if tlas:
        nodes = got[2]
        assert nodes.shape == (S, 2 * c.T.shape[1])
        for s, n in want_nodes.items():
            assert nodes[s].tobytes() == n.tobytes(), (name, "tlas", s)
    assert same(acc, r.oracle(c)), (name, "oracle")
    assert (acc[..., 3].view(np.uint32) == 0).all()                        # w = +0
    if full:
        assert same(r.run(c), acc)                                          # no pixels, no boxes, no nodes asked for
    return acc


# 1: the loop and the oracle
@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("name", si.LOOP_CASES)
def test_shapes_equal_the_loop_and_the_oracle(rigs, name, passes):
    r = rigs(si.case_scene(name))
    c = r.case(name, passes=passes)
    assert len(c.cameras) == len(c.pos) == 3 and c.frames == 2
    check_against_loop_and_oracle(r, c, name)


# 2: a shape per lane (one full window and a partial one); 3: views that straddle windows, three views over two shapes
@pytest.mark.parametrize("name", ["lanes_69", "windows_48", "tlas3_windows"])
def test_a_shape_per_lane_and_views_across_windows(rigs, name):
    r = rigs(si.case_scene(name))
    c = r.case(name)
    acc = r.run(c)
    want = r.loop(c)[0]
    bad = [v for v in range(len(c.cameras)) if not same(acc[v], want[v])]
    assert not bad, (name, "loop", bad[:8])
    assert same(acc, r.oracle(c)), (name, "oracle")


# 4: node 1 keeps the live scene's box; a root that is a leaf has no pair at all
@pytest.mark.parametrize("name", ["stale_node1", "leaf_root"])
def test_stale_node1_and_a_leaf_root(rigs, name):
    r = rigs(si.case_scene(name))
    check_against_loop_and_oracle(r, r.case(name), name)


# 5: shapes whose TLASes differ in height in one job, and the job with the shapes reversed
def test_mixed_heights_in_one_job_and_reversed(rigs):
    r = rigs("ring40")
    c = r.case("mixed_heights")
    acc = check_against_loop_and_oracle(r, c, "mixed_heights", full=False)
    got = r.run(c.reversed(), want_root_boxes=True, want_tlas=True)
    fwd = r.run(c, want_root_boxes=True, want_tlas=True)
    assert same(got[0], acc[::-1]) and got[1].tobytes() == fwd[1][::-1].tobytes() and same(got[2], fwd[2][::-1])
    heights = [inp.restate(np.stack([fwd[2][s] if i == c.bvh else np.stack([r.hs.bvh(i)["nodes"][0]["aabbMin"], r.hs.bvh(i)["nodes"][0]["aabbMax"]])
                                     for i in range(r.hs.bvh_count())]), c.T[s])["height"] for s in (0, 1)]
    assert heights[0] != heights[1], heights


# 6: the live scene is not changed
@pytest.mark.parametrize("scene,name", [("cube", "cube_loop"), ("tlas3", "tlas3_loop")])
def test_the_live_scene_is_untouched(crt, tmp_path, scene, name):
    r = Rig(crt, None, tmp_path, scene)
    c = r.case(name)
    ctx = r.ctx
    live_T = to_dev(np.stack([r.hs.blas_transform(i)[0].reshape(4, 4) for i in range(r.hs.bvh_count())])) if c.T is not None else None
    lo, hi = c.pos[0].reshape(-1, 3).min(0), c.pos[0].reshape(-1, 3).max(0)
    if c.T is not None:
        O, D = inp.aimed_rays(np.stack([r.hs.blas_transform(i)[0].reshape(4, 4) for i in range(r.hs.bvh_count())]))
    else:
        from test_gpu_refit_device import aimed_rays
        O, D = aimed_rays(lo, hi, 1500, 7)

    def state(x):
        b = x.get_bvh(c.bvh)
        x.set_camera_state(*c.cameras[0]); x.clear(); x.render(1, 2, 1)
        hits = x.find_nearest(O, D)
        nodes = x.update_transforms_device(live_T).tobytes() if live_T is not None else b""
        return (b["nodes"].tobytes(), b["indices"].tobytes(), x.accumulator().tobytes(), tuple(hits[f].tobytes() for f in ("t", "u", "v", "objIdx", "triIdx", "traversed", "tested")), nodes), hits

    before, hits = state(ctx)
    assert state(r.ref)[0] == before                                         # (the second context goes through the same calls, the job apart)
    assert (hits["objIdx"] >= 2).sum() > 50
    r.run(c, scale=0.5, want_root_boxes=True, want_tlas=c.T is not None)
    assert state(ctx)[0] == before and state(r.ref)[0] == before
    # the camera and crt_tick's rendered-ahead frames survive the job: the Ticks of the context that runs it in between equal those of the one that does not
    ctx.set_camera_state(*c.cameras[1]); r.ref.set_camera_state(*c.cameras[1])
    for spp in range(1, 6):
        if spp == 4:
            r.run(c)
        pa, ra, ea = ctx.tick(spp)
        pb, rb, eb = r.ref.tick(spp)
        assert np.array_equal(pa, pb) and same(ra, rb) and ea == eb, spp
    r.close()


# 7: the device entry, positions produced on the same side stream immediately before the call
@pytest.mark.parametrize("scene,name", [("cube", "cube_loop"), ("tlas3", "tlas3_loop")])
def test_device_entry_behind_a_torch_operation(rigs, scene, name):
    r = rigs(scene)
    c0 = r.case(name)
    a = [0.05, 0.11, 0.17]
    pos = np.stack([si.deform_by(c0.pos[0], x) for x in a])
    c = si.Case(c0.scene, c0.bvh, pos, c0.T, c0.cameras, [2, 0, 1], 1, 3, 1)
    scale = 0.25
    tlas = c.T is not None
    want = r.run(c, scale=scale, want_root_boxes=True, want_tlas=tlas)
    k = len(c.cameras)
    side = torch.cuda.Stream(device=dev())
    base = to_dev(c0.pos[0]); fac = to_dev(np.array(a, np.float32))
    cams = to_dev(r.records(c.cameras)); vs = to_dev(c.view_shape, np.int32)
    T = to_dev(c.T.reshape(len(c.T), -1, 16)) if tlas else None
    out = torch.full((k, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
    pix = torch.full((k, H, W), 0x5A5A5A5A, dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_pos = (base[None] + fac[:, None, None, None] * (base[..., [1, 2, 0]] * base[..., [2, 0, 1]])[None]).contiguous()      # no synchronisation before the call
        got = r.ctx.render_shapes_device(cams, c.bvh, d_pos, out, c.spp_first, c.frames, c.passes, scale=scale, pixels=pix, T=T, view_shape=vs, want_root_boxes=True,
                                         want_tlas=tlas, stream=side)
    side.synchronize()
    assert same(d_pos.cpu().numpy(), pos)                                    # (the torch expression is the numpy one, operation for operation)
    assert got[0] is out and got[1] is pix
    assert same(out.cpu().numpy(), want[0]) and np.array_equal(pix.cpu().numpy().view(np.uint32), want[1])
    assert same(got[-1], want[-1])
    if tlas:
        assert got[2].tobytes() == want[2].tobytes()
    out2 = torch.full((k, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
    r.ctx.render_shapes_device(cams, c.bvh, d_pos, out2, c.spp_first, c.frames, c.passes, T=T, view_shape=vs)      # the current (default) stream, no optional output
    torch.cuda.synchronize()
    assert same(out2.cpu().numpy(), want[0])


# 8: a bad shape among good ones; a view_shape entry out of range
def test_a_bad_shape_refuses_the_job(rigs, crt):
    r = rigs("tlas3"); ctx = r.ctx
    c = r.case("bad_shape")
    cams, T = r.records(c.cameras), np.ascontiguousarray(c.T.reshape(3, -1, 16))
    ctx.set_camera_state(*c.cameras[0]); ctx.clear(); ctx.render(1, 2, 1)
    before = ctx.accumulator()
    acc = np.full((3, H, W, 4), SENTINEL_F, np.float32); px = np.full((3, H, W), SENTINEL_U, np.uint32)
    boxes = np.full((3, 2, 3), SENTINEL_F, np.float32)
    nodes = np.zeros((3, 6), inp.TLAS_DTYPE); nodes.view(np.uint8)[:] = 0x5A
    keep = nodes.tobytes()
    assert raw_shapes(ctx, cams, c.bvh, c.pos, T, None, 1, 1, 1, 1.0, acc, px, boxes, nodes) == INVALID
    msg = ctx.L.crt_last_error(ctx.h).decode()
    assert "shape 1" in msg and "FindBestMatch" in msg and "crt_render_shapes" in msg, msg
    assert (acc == SENTINEL_F).all() and (px == SENTINEL_U).all() and (boxes == SENTINEL_F).all() and nodes.tobytes() == keep
    d_acc = torch.full((3, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev()); d_px = torch.full((3, H, W), 0x5A5A5A5A, dtype=torch.int32, device=dev())
    with pytest.raises(crt.CrtError) as e:                                   # the device entry learns of it with the headers
        ctx.render_shapes_device(to_dev(cams), c.bvh, to_dev(c.pos), d_acc, 1, 1, scale=1.0, pixels=d_px, T=to_dev(T), want_tlas=True, want_root_boxes=True)
    assert e.value.code == INVALID and "shape 1" in str(e.value) and "crt_render_shapes_device" in str(e.value)
    torch.cuda.synchronize()
    assert (d_acc.cpu().numpy() == SENTINEL_F).all() and (d_px.cpu().numpy() == 0x5A5A5A5A).all()
    assert raw_shapes(ctx, cams, c.bvh, c.pos, T, np.array([0, 2, 2], np.int32), 1, 1, 1, 1.0, acc, px) == INVALID      # no view uses shape 1: it is still built, and still bad
    assert (acc == SENTINEL_F).all()
    ok = si.Case(c.scene, c.bvh, c.pos[[0, 2]], c.T[[0, 2]], c.cameras, [0, 1, 1], 1, 1, 1)                               # the job without the bad shape runs
    assert same(r.run(ok), r.loop(ok)[0])
    # view_shape out of range: the host entry, then the device entry (which learns of it from the build launch), on the two-level scene and on a FileScene
    pos_ok, T_ok = np.ascontiguousarray(c.pos[[0, 2]]), np.ascontiguousarray(T[[0, 2]])
    for bad_vs in ([0, 2, 1], [0, -1, 1]):
        assert raw_shapes(ctx, cams, c.bvh, pos_ok, T_ok, np.array(bad_vs, np.int32), 1, 1, 1, 1.0, acc, px) == INVALID
        assert b"view_shape[1]" in ctx.L.crt_last_error(ctx.h)
        d_out = torch.full((3, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
        with pytest.raises(crt.CrtError) as e:
            ctx.render_shapes_device(to_dev(cams), c.bvh, to_dev(pos_ok), d_out, 1, 1, T=to_dev(T_ok), view_shape=to_dev(bad_vs, np.int32))
        assert e.value.code == INVALID and "view_shape[1]" in str(e.value)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == SENTINEL_F).all() and (acc == SENTINEL_F).all() and (px == SENTINEL_U).all()
    cube = rigs("cube"); cc = cube.case("cube_loop")
    d_out = torch.full((3, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
    with pytest.raises(crt.CrtError) as e:
        cube.ctx.render_shapes_device(to_dev(cube.records(cc.cameras)), 0, to_dev(cc.pos), d_out, 1, 1, view_shape=to_dev([0, 1, 3], np.int32))
    assert e.value.code == INVALID and "view_shape[2]" in str(e.value)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == SENTINEL_F).all()
    ctx.clear(); ctx.render(1, 2, 1)                                         # a render afterwards equals the one before
    assert same(ctx.accumulator(), before)


# 8: every row of the refusal table, the outputs' sentinel intact
def test_refusals_leave_the_outputs_alone(rigs, crt, tmp_path):
    r = rigs("tlas3"); ctx = r.ctx; L = ctx.L
    c = r.case("tlas3_loop")
    k, n, tris = 3, c.T.shape[1], c.pos.shape[1]
    cams_h, T_h, pos_h = r.records(c.cameras), np.ascontiguousarray(c.T.reshape(3, -1, 16)), np.ascontiguousarray(c.pos)
    cams, T, pos = to_dev(cams_h), to_dev(T_h), to_dev(pos_h)
    out = torch.full((k * H * W * 4 + 4,), float(SENTINEL_F), dtype=torch.float32, device=dev())
    vs = to_dev([0, 1, 2], np.int32)
    host_out = np.zeros((k, H, W, 4), np.float32)
    boxes = np.full((3, 2, 3), SENTINEL_F, np.float32)

    def call(d_cams, d_pos, d_T, d_out, c_=ctx, kk=k, bvh=c.bvh, S=3, nt=tris, blas=n, d_vs=None, frames=1, passes=1, stream=None):
        return L.crt_render_shapes_device(c_.h, C.c_void_p(d_cams), C.c_uint32(kk), C.c_uint32(bvh), C.c_void_p(d_pos), C.c_uint32(S), C.c_uint32(nt), C.c_void_p(d_T), C.c_uint32(blas),
                                          C.c_void_p(d_vs), C.c_uint32(1), C.c_uint32(frames), C.c_uint32(passes), C.c_float(1.0), C.c_void_p(d_out), None,
                                          boxes.ctypes.data_as(C.c_void_p), None, stream)
    a, p, t, o = cams.data_ptr(), pos.data_ptr(), T.data_ptr(), out.data_ptr()
    assert call(a, p, t, o, bvh=n) == INVALID                                # 3: bvh out of range, triCount
    assert call(a, p, t, o, nt=tris - 1) == INVALID
    assert call(a, p, None, o) == INVALID and call(a, p, t, o, blas=n + 1) == INVALID and call(a, p, None, o, blas=0) == INVALID       # 5
    assert call(a, p, t, o, passes=0) == INVALID and call(a, p, t, o, passes=5) == INVALID                                              # 7
    assert call(a, p, t, o, kk=1 << 16, S=1 << 16, frames=1 << 16) == UNSUPPORTED                                                       # 8: more than 2^31-1 view-frames
    assert call(a, p, t, o, S=0) == INVALID                                  # 10: no shape; view_shape NULL with S != K
    assert call(a, p, t, o, S=2) == INVALID
    assert call(a, p, t, o, kk=1, S=1 << 26, d_vs=vs.data_ptr()) == UNSUPPORTED and b"4 GiB" in L.crt_last_error(ctx.h)                 # 11
    assert call(a, p, t, o, S=2, d_vs=vs.data_ptr()) == INVALID              # 13: an entry outside [0, S): the device entry's check
    assert b"view_shape[2]" in L.crt_last_error(ctx.h)
    assert call(a, p, t, host_out.ctypes.data) == INVALID                    # 12: host pointers
    assert call(cams_h.ctypes.data, p, t, o) == INVALID
    assert call(a, pos_h.ctypes.data, t, o) == INVALID
    assert call(a, p, T_h.ctypes.data, o) == INVALID
    assert call(a, p, t, o, d_vs=np.zeros(3, np.int32).ctypes.data) == INVALID
    assert call(a, p, t, o + 4) == INVALID and b"16-byte" in L.crt_last_error(ctx.h)
    assert call(a, p + 2, t, o) == INVALID and call(a, p, t + 2, o) == INVALID                                                          # misaligned
    assert call(None, p, t, o) == INVALID and call(a, None, t, o) == INVALID and call(a, p, t, None) == INVALID
    if torch.cuda.device_count() > 1:
        assert call(a, p, t, o, stream=C.c_void_p(torch.cuda.Stream(device=torch.device("cuda", 1)).cuda_stream)) == INVALID
    # K = 0 and frames = 0: no-ops after the checks that need no buffer
    assert call(None, None, t, None, kk=0, S=0) == 0 and call(None, None, t, None, frames=0) == 0 and call(None, None, t, None, kk=0, S=0, passes=9) == INVALID
    # the host entry's own: NULL buffers, view_shape looked at before anything runs
    acc = np.full((k, H, W, 4), SENTINEL_F, np.float32)
    assert raw_shapes(ctx, cams_h, c.bvh, pos_h, T_h, np.array([0, 3, 1], np.int32), 1, 1, 1, 1.0, acc, None) == INVALID and b"view_shape[1] = 3" in L.crt_last_error(ctx.h)
    assert raw_shapes(ctx, cams_h, c.bvh, pos_h, T_h, None, 1, 1, 1, 1.0, None, None) == INVALID
    assert raw_shapes(ctx, cams_h, c.bvh, pos_h, T_h, None, 1, 0, 1, 1.0, acc, None) == 0 and (acc == SENTINEL_F).all()
    # 9: another accelerator selected
    hs = crt.HostScene(r.xml, 1, ASSETS); hs.build_alt(crt.ACCEL_KDTREE)
    kd = crt.Context(W, H); hs.upload(kd); hs.upload_alt(kd, crt.ACCEL_KDTREE); kd.set_render_accel(crt.ACCEL_KDTREE)
    assert call(a, p, t, o, c_=kd) == UNSUPPORTED
    assert (boxes == SENTINEL_F).all()
    kd.set_render_accel(0)
    assert call(a, p, t, o, c_=kd) == 0                                      # ... and with the BVH selected again the job runs
    torch.cuda.synchronize()
    one = si.Case(c.scene, c.bvh, c.pos, c.T, c.cameras, None, 1, 1, 1)
    want = r.loop(one)
    assert same(out.cpu().numpy()[:k * H * W * 4].reshape(k, H, W, 4), want[0]) and all(same(boxes[s], want[2][s]) for s in range(3))
    out.fill_(float(SENTINEL_F)); boxes[:] = SENTINEL_F; torch.cuda.synchronize()
    kd.close()
    # 1: no scene; 4: a FileScene with transforms; 2: a PrimitiveScene
    fresh = crt.Context(W, H)
    assert call(a, p, t, o, c_=fresh) == STATE
    cube = rigs("cube"); cc = cube.case("cube_loop"); cpos = to_dev(cc.pos)
    assert call(a, cpos.data_ptr(), t, o, c_=cube.ctx, bvh=0, nt=12, blas=0) == INVALID
    assert call(a, cpos.data_ptr(), None, o, c_=cube.ctx, bvh=0, nt=12, blas=1) == INVALID
    assert call(a, cpos.data_ptr(), None, o, c_=cube.ctx, bvh=1, nt=12, blas=0) == INVALID
    fresh.close()
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(0.0)
    pc = crt.Context(W, H); ps.upload(pc)
    assert call(a, p, t, o, c_=pc) == UNSUPPORTED
    pc.close()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL_F).all() and not host_out.any() and (acc == SENTINEL_F).all() and (boxes == SENTINEL_F).all()


def chain_scene(crt, N, tris, extra_nodes=0):
    """N chain BLASes (tests/test_gpu_tlas_device.py chain_blas) under the TLAS of a 4-wide grid of transforms; extra_nodes: unused TLAS records behind the 2 N"""
    from test_gpu_tlas_device import chain_blas
    bvhs = [chain_blas(crt, tris, i + 2) for i in range(N)]
    boxes = np.stack([np.stack([b["nodes"][0]["aabbMin"], b["nodes"][0]["aabbMax"]]) for b in bvhs])
    flat = np.stack([inp.rigid((i % 4 - 1.5, i // 4 - 1.5, 5.0)) for i in range(N)])
    first = inp.restate(boxes, flat)
    for b, t, it in zip(bvhs, flat, first["invT"]):
        b.update(T=t, invT=it.reshape(4, 4))
    tex = np.full((4, 4), 0x808080, np.uint32); ident = np.eye(4, dtype=np.float32)
    ctx = crt.Context(W, H)
    nodes = np.concatenate([first["nodes"], np.zeros(extra_nodes, inp.TLAS_DTYPE)])
    ctx.upload_desc(crt.SCENE_TLAS, bvhs, tlas_nodes=nodes, textures=[tex, tex], floor_texture=0, sky_texture=1, materials=[(0.0, 0.0, (0.0, 0.0, 0.0), -1)], light_T=ident,
                    light_invT=ident)
    t = bvhs[1]["tris"]
    pos = np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1).astype(np.float32)
    return ctx, boxes, flat, first, pos


def test_a_scene_with_spare_tlas_nodes_is_refused(crt):
    """row 6: TLASBVH::Build makes 2 * bvhCount nodes; a scene uploaded with more has no room laid out as the build's image"""
    ctx, _, flat, _, pos = chain_scene(crt, 2, 3, extra_nodes=2)
    cams = crt.camera_records(W, H, [((0.0, 0.0, 0.0), (0.0, 0.0, 5.0))])
    acc = np.full((1, H, W, 4), SENTINEL_F, np.float32)
    assert raw_shapes(ctx, cams, 1, pos[None].copy(), np.ascontiguousarray(flat.reshape(1, 2, 16)), None, 1, 1, 1, 1.0, acc, None) == UNSUPPORTED
    assert b"TLAS nodes" in ctx.L.crt_last_error(ctx.h) and (acc == SENTINEL_F).all()
    ctx.close()


def test_a_shape_too_tall_for_the_lds_stack_is_refused(crt):
    """row 15: 16 chain BLASes of height 40: under the TLAS of a 4 x 4 grid (height 5) the stack is 40 + 5 + 1 = 46 dwords per lane and the job runs; one shape whose
    transforms make a caterpillar (height 15) puts it at 56, beyond the 49 that four wavefronts' columns and factors leave of a workgroup's 64 KiB"""
    N = 16
    ctx, boxes, flat, first, pos = chain_scene(crt, N, 41)
    line = np.stack([inp.rigid((4.0 ** i, 0.0, 5.0)) for i in range(N)])
    assert first["height"] == 5 and inp.restate(boxes, line)["height"] == 15
    cams = crt.camera_records(W, H, [((0.0, 0.0, 0.0), (0.0, 0.0, 5.0)), ((0.5, 0.0, 0.0), (0.0, 0.0, 5.0))])
    both = np.stack([pos, pos * np.float32(1.25)])
    ok = ctx.render_shapes(cams, 1, both, 1, 1, T=np.stack([flat, flat]).reshape(2, N, 16))
    assert np.isfinite(ok).all()
    acc = np.full((2, H, W, 4), SENTINEL_F, np.float32); bx = np.full((2, 2, 3), SENTINEL_F, np.float32)
    assert raw_shapes(ctx, cams, 1, both, np.ascontiguousarray(np.stack([flat, line]).reshape(2, N, 16)), None, 1, 1, 1, 1.0, acc, None, bx) == UNSUPPORTED
    msg = ctx.L.crt_last_error(ctx.h).decode()
    assert "shape 1" in msg and (acc == SENTINEL_F).all() and (bx == SENTINEL_F).all(), msg
    assert same(ctx.render_shapes(cams, 1, both, 1, 1, T=np.stack([flat, flat]).reshape(2, N, 16)), ok)
    ctx.close()


def test_a_failed_device_allocation_is_refused(rigs):
    """row 16: the host entry's staging for 2^26 views of 32 x 16 pixels is 512 GiB, which hipMalloc refuses at once, before a camera, a position or an image is read.
    One shape and a view_shape of zeros keep the shape table small and K * frames below 2^31."""
    r = rigs("cube"); ctx = r.ctx
    c = r.case("cube_loop")
    want = r.loop(c)[0]
    assert same(r.run(c), want)                                              # (staging of the usual size is in place)
    K = 1 << 26
    cams = r.records(c.cameras[:1]); pos = np.ascontiguousarray(c.pos[:1])
    vs = np.zeros(K, np.int32)
    acc = np.full((1, H, W, 4), SENTINEL_F, np.float32); px = np.full((1, H, W), SENTINEL_U, np.uint32); bx = np.full((1, 2, 3), SENTINEL_F, np.float32)
    assert raw_shapes(ctx, cams, 0, pos, None, vs, 1, 1, 1, 1.0, acc, px, bx, K=K) == DEVICE
    assert "hipMalloc" in ctx.L.crt_last_error(ctx.h).decode()
    assert (acc == SENTINEL_F).all() and (px == SENTINEL_U).all() and (bx == SENTINEL_F).all()
    assert same(r.run(c), want)                                              # the context has dropped its staging and takes the next job as usual


# 9: the rows the tiling truncates and the tiles the context does not own stay as the caller left them
@pytest.mark.parametrize("own", ["all", "strided"])
def test_ownership_and_truncation(crt, tmp_path, own):
    cfg = dict(tile_first=1, tile_stride=2, tile_count=3) if own == "strided" else {}
    r = Rig(crt, None, tmp_path, "cube", 48, 40, **cfg)
    c = r.case("cube_loop")
    acc = np.full((3, 40, 48, 4), SENTINEL_F, np.float32); px = np.full((3, 40, 48), SENTINEL_U, np.uint32)
    assert raw_shapes(r.ctx, r.records(c.cameras), 0, np.ascontiguousarray(c.pos), None, None, c.spp_first, c.frames, c.passes, 0.5, acc, px) == 0
    owned = np.zeros((40, 48), bool)
    for t in ([1, 3, 5] if own == "strided" else range(6)):
        owned[16 * (t // 3):16 * (t // 3) + 16, 16 * (t % 3):16 * (t % 3) + 16] = True
    want = r.loop(c)[0]
    for k in range(3):
        assert same(acc[k][owned], want[k][owned]), k
        assert (acc[k][~owned] == SENTINEL_F).all() and (px[k][~owned] == SENTINEL_U).all(), k
        assert (px[k][owned] != SENTINEL_U).all(), k
    r.close()
