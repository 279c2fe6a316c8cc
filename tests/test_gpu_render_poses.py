"""crt_render_poses / crt_render_poses_device: the frames of many cameras over many job-local poses of a two-level scene's instances in one render job
(csrc/device/render_poses.h, tlas_build.hip's batched build).  Every comparison is bit for bit (np.array_equal) against one or both of
  the loop    update_transforms_device(T[p]) + set_camera_state + clear + render + accumulator per view, through the existing entries, on a SECOND context;
  the oracle  set_transform for every instance, set_camera_state, render.
The scenes, poses and cameras are tests/render_poses_inputs.py's; tests/test_render_poses_cpu.py holds, without a GPU, that every camera sees an instance in the
pose it is paired with and that no two views of a case are alike, so a lane that walks the wrong pose cannot pass here."""
import ctypes as C

import numpy as np
import pytest

import render_poses_inputs as pi
import tlas_device_inputs as inp
from conftest import ASSETS, scene_path
from test_oracle_pinning import deform

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H = pi.W, pi.H
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

    def __init__(self, crt, orc, xml, width=W, height=H, **cfg):
        self.crt, self.xml, self.W, self.H = crt, xml, width, height
        self.hs = crt.HostScene(xml, 1, ASSETS)
        self.ctx, self.ref = crt.Context(width, height, **cfg), crt.Context(width, height, **cfg)
        self.hs.upload(self.ctx); self.hs.upload(self.ref)
        self.o = pi.make_oracle(orc, ASSETS, xml, width, height) if orc is not None else None
        self._loop, self._oracle = {}, {}

    def records(self, cameras):
        return self.crt.camera_records(self.W, self.H, cameras)

    def boxes(self):
        return np.stack([np.stack([self.hs.bvh(i)["nodes"][0]["aabbMin"], self.hs.bvh(i)["nodes"][0]["aabbMax"]]) for i in range(self.hs.bvh_count())])

    def loop(self, c, views=None, scale=None):
        """(accumulators, pixels or None, {pose: nodes}) of the views through the existing entries on `ref`"""
        acc, px, nodes = [], [], {}
        for k in (range(len(c.cameras)) if views is None else views):
            p = c.pose_of(k)
            key = (c.T[p].tobytes(), c.cameras[k], c.spp_first, c.frames, c.passes, scale)
            if key not in self._loop:
                n = self.ref.update_transforms_device(to_dev(c.T[p]))
                self.ref.set_camera_state(*c.cameras[k]); self.ref.clear(); self.ref.render(c.spp_first, c.frames, c.passes)
                a = self.ref.accumulator(); a.setflags(write=False)
                self._loop[key] = (a, self.ref.resolve_screen(scale)[0] if scale is not None else None, n)
            a, x, n = self._loop[key]
            acc.append(a); px.append(x); nodes[p] = n
        return np.stack(acc), (np.stack(px) if scale is not None else None), nodes

    def oracle(self, c, views=None):
        out = []
        for k in (range(len(c.cameras)) if views is None else views):
            key = (c.T[c.pose_of(k)].tobytes(), c.cameras[k], c.spp_first, c.frames, c.passes)
            if key not in self._oracle:
                a = pi.oracle_view(self.o, c, k)[0]; a.setflags(write=False)
                self._oracle[key] = a
            out.append(self._oracle[key])
        return np.stack(out)

    def run(self, c, ctx=None, **kw):
        return (ctx or self.ctx).render_poses(self.records(c.cameras), c.T.reshape(len(c.T), -1, 16), c.spp_first, c.frames, c.passes, view_pose=c.view_pose, **kw)

    def close(self):
        self.ctx.close(); self.ref.close()


@pytest.fixture(scope="module")
def rigs(crt, orc, tmp_path_factory):
    cache, tmp = {}, tmp_path_factory.mktemp("poses")

    def get(scene):
        if scene not in cache:
            cache[scene] = Rig(crt, orc, inp.scene_xml(tmp, scene))
        return cache[scene]
    yield get
    for r in cache.values():
        r.close()


def raw_poses(ctx, cams, T, vp, spp_first, frames, passes, scale, acc, px, nodes=None, P=None, n=None):
    """crt_render_poses into arrays the caller has filled"""
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    return ctx.L.crt_render_poses(ctx.h, p(cams), C.c_uint32(len(cams)), p(T), C.c_uint32(len(T) if P is None else P), C.c_uint32(T.shape[1] if n is None else n), p(vp),
                                  C.c_uint32(spp_first), C.c_uint32(frames), C.c_uint32(passes), C.c_float(scale), p(acc), p(px), p(nodes))


# 1: the loop
@pytest.mark.parametrize("name", pi.LOOP_CASES)
def test_poses_equal_the_loop_and_the_oracle(rigs, name):
    c = pi.case(name); r = rigs(c.scene)
    scale = 1.0 / (c.spp_first + c.frames * c.passes)
    acc, px, nodes = r.run(c, scale=scale, want_tlas=True)
    k = len(c.cameras)
    assert acc.shape == (k, H, W, 4) and px.shape == (k, H, W) and nodes.shape == (len(c.T), 2 * c.T.shape[1])
    want, want_px, want_nodes = r.loop(c, scale=scale)
    bad = [v for v in range(k) if not same(acc[v], want[v])]
    assert not bad, (name, "loop", bad)
    assert np.array_equal(px, want_px)
    assert same(acc, r.oracle(c)), (name, "oracle")
    assert (acc[..., 3].view(np.uint32) == 0).all()                        # w = +0
    boxes = r.boxes()
    for p in range(len(c.T)):
        assert nodes[p].tobytes() == want_nodes[p].tobytes(), p
        assert nodes[p].tobytes() == inp.restate(boxes, c.T[p])["nodes"].tobytes(), p
    assert same(r.run(c), acc)                                              # no pixels, no nodes asked for


# 2, 3: lanes with different TLASes (a pose per lane, a partial last window); views that straddle windows
@pytest.mark.parametrize("name", pi.LANE_CASES + ("straddle_3",))
def test_a_pose_per_lane_and_views_across_windows(rigs, name):
    c = pi.case(name); r = rigs(c.scene)
    acc = r.run(c)
    want = r.loop(c)[0]
    bad = [v for v in range(len(c.cameras)) if not same(acc[v], want[v])]
    assert not bad, (name, "loop", bad[:8])
    assert same(acc, r.oracle(c)), (name, "oracle")


# 4: poses of different TLAS heights in one job
def test_mixed_heights_in_one_job(rigs):
    c = pi.case("mixed_heights"); r = rigs(c.scene)
    heights = [inp.restate(r.boxes(), c.T[p])["height"] for p in (0, 1)]
    assert heights[0] != heights[1], heights
    acc, nodes = r.run(c, want_tlas=True)
    want, _, want_nodes = r.loop(c)
    assert same(acc[0], want[0]) and same(acc[1], want[1])                   # the stack is the taller pose's; the shorter one is unharmed
    assert nodes[0].tobytes() == want_nodes[0].tobytes() and nodes[1].tobytes() == want_nodes[1].tobytes()
    assert same(acc, r.oracle(c))
    swapped = pi.Case(c.scene, c.T[::-1].copy(), c.cameras[::-1], None, c.spp_first, c.frames, c.passes)      # the taller pose first
    assert same(r.run(swapped), acc[::-1])


# 5: the list extremes
@pytest.mark.parametrize("name", pi.EXTREMES)
def test_list_extremes(rigs, name):
    c = pi.case(name); r = rigs(c.scene)
    acc, nodes = r.run(c, want_tlas=True)
    want, _, want_nodes = r.loop(c)
    for v in range(len(c.cameras)):
        assert same(acc[v], want[v]), (name, v)
        assert nodes[v].tobytes() == want_nodes[v].tobytes(), (name, v)
    assert same(acc, r.oracle(c)), (name, "oracle")
    if name == "rand256":
        assert all(inp.restate(r.boxes(), c.T[p])["stale_a"] > 0 for p in range(len(c.T)))


# 6: a bad pose among good ones; a view_pose entry out of range
def test_a_bad_pose_refuses_the_job(rigs, crt):
    c = pi.case("bad_pose"); r = rigs(c.scene); ctx = r.ctx
    cams, T = r.records(c.cameras), np.ascontiguousarray(c.T.reshape(3, -1, 16))
    ctx.set_camera_state(*c.cameras[0]); ctx.clear(); ctx.render(1, 2, 1)
    before = ctx.accumulator()
    acc = np.full((3, H, W, 4), SENTINEL_F, np.float32); px = np.full((3, H, W), SENTINEL_U, np.uint32)
    nodes = np.zeros((3, 16), inp.TLAS_DTYPE); nodes.view(np.uint8)[:] = 0x5A
    keep = nodes.tobytes()
    assert raw_poses(ctx, cams, T, None, 1, 1, 1, 1.0, acc, px, nodes) == INVALID
    msg = ctx.L.crt_last_error(ctx.h).decode()
    assert "pose 1" in msg and "FindBestMatch" in msg and "crt_render_poses" in msg, msg
    assert (acc == SENTINEL_F).all() and (px == SENTINEL_U).all() and nodes.tobytes() == keep
    d_acc = torch.full((3, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev()); d_px = torch.full((3, H, W), 0x5A5A5A5A, dtype=torch.int32, device=dev())
    with pytest.raises(crt.CrtError) as e:                                   # the device entry learns of it with the headers
        ctx.render_poses_device(to_dev(cams), to_dev(T), d_acc, 1, 1, scale=1.0, pixels=d_px, want_tlas=True)
    assert e.value.code == INVALID and "pose 1" in str(e.value) and "crt_render_poses_device" in str(e.value)
    torch.cuda.synchronize()
    assert (d_acc.cpu().numpy() == SENTINEL_F).all() and (d_px.cpu().numpy() == 0x5A5A5A5A).all()
    assert raw_poses(ctx, cams, T, np.array([0, 2, 2], np.int32), 1, 1, 1, 1.0, acc, px) == INVALID      # no view uses pose 1: it is still built, and still bad
    assert (acc == SENTINEL_F).all()
    T_ok = np.ascontiguousarray(T[[0, 2]])                                   # the job without the bad pose runs
    ok = pi.Case(c.scene, c.T[[0, 2]], c.cameras, [0, 1, 1], 1, 1, 1)
    assert same(r.run(ok), r.loop(ok)[0])
    # view_pose out of range: the host entry, then the device entry (which learns of it from the build launch)
    for bad_vp in ([0, 2, 1], [0, -1, 1]):
        assert raw_poses(ctx, cams, T_ok, np.array(bad_vp, np.int32), 1, 1, 1, 1.0, acc, px) == INVALID
        assert b"view_pose[1]" in ctx.L.crt_last_error(ctx.h)
        d_out = torch.full((3, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
        with pytest.raises(crt.CrtError) as e:
            ctx.render_poses_device(to_dev(cams), to_dev(T_ok), d_out, 1, 1, view_pose=to_dev(bad_vp, np.int32))
        assert e.value.code == INVALID and "view_pose[1]" in str(e.value)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == SENTINEL_F).all() and (acc == SENTINEL_F).all() and (px == SENTINEL_U).all()
    ctx.clear(); ctx.render(1, 2, 1)                                         # a render afterwards equals the one before
    assert same(ctx.accumulator(), before)


# 7: the live scene is not changed
def test_the_live_scene_is_untouched(crt, orc, tmp_path):
    c = pi.case("loop_5_of_2")
    a, b = Rig(crt, None, inp.scene_xml(tmp_path, c.scene)), Rig(crt, None, inp.scene_xml(tmp_path, c.scene))
    base = inp.transforms("tlas3")
    O, D = inp.aimed_rays(base)
    cam = c.cameras[3]
    hits0 = a.ctx.find_nearest(O, D)
    a.ctx.set_camera_state(*cam); b.ctx.set_camera_state(*cam)
    for spp in range(1, 7):
        if spp == 4:
            a.run(c)
        pa, ra, ea = a.ctx.tick(spp)
        pb, rb, eb = b.ctx.tick(spp)
        assert np.array_equal(pa, pb) and same(ra, rb) and ea == eb, spp
    hits1 = a.ctx.find_nearest(O, D)
    for f in ("t", "u", "v", "objIdx", "triIdx", "traversed", "tested"):
        assert hits0[f].tobytes() == hits1[f].tobytes(), f
    assert (hits0["objIdx"] >= 2).sum() > 100
    moved = pi.poses("tlas3", 3)[2]
    assert a.ctx.update_transforms_device(to_dev(moved)).tobytes() == b.ctx.update_transforms_device(to_dev(moved)).tobytes()
    # counters: the job's growth is the loop's
    keys = ("rays", "primary", "mesh_hits")
    a.ctx.sync(); c0 = a.ctx.counters()
    a.run(c)
    a.ctx.sync(); c1 = a.ctx.counters()
    b.ref.sync(); r0 = b.ref.counters()
    b.loop(c)
    b.ref.sync(); r1 = b.ref.counters()
    assert {k: c1[k] - c0[k] for k in keys} == {k: r1[k] - r0[k] for k in keys}
    assert c1["primary"] - c0["primary"] == 5 * c.frames * c.passes * 2 * 256 and c1["mesh_hits"] > c0["mesh_hits"]
    a.close(); b.close()


# 8: after a refit on the device the poses' world boxes are the refitted node-0 boxes, with nothing from the host in between
def test_after_a_refit_on_the_device(crt, tmp_path):
    xml = inp.scene_xml(tmp_path, "ring40")
    r = Rig(crt, None, xml)
    T = pi.poses("ring40", 2)
    c = pi.Case("ring40", T, pi.looking_at(T[0], 2), None, 1, 2, 1)
    plain = r.run(c)
    for i in (0, 1, 2, 3):                                                   # the instances the cameras look at
        t = r.hs.bvh(i)["tris"]
        moved = deform(np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1).astype(np.float32) * np.float32(1.7))
        r.ctx.refit_device(i, to_dev(moved), root_box=False)
        r.ref.refit_device(i, to_dev(moved), root_box=False)
    acc, nodes = r.run(c, want_tlas=True)
    want, _, want_nodes = r.loop(c)
    assert same(acc, want) and not same(acc, plain)
    assert all(nodes[p].tobytes() == want_nodes[p].tobytes() for p in (0, 1))
    assert nodes[0].tobytes() != inp.restate(r.boxes(), T[0])["nodes"].tobytes()          # (the host scene's boxes are the old ones)
    r.close()


# 9: the rows the tiling truncates and the tiles the context does not own stay as the caller left them
@pytest.mark.parametrize("own", ["all", "strided"])
def test_ownership_and_truncation(crt, tmp_path, own):
    cfg = dict(tile_first=1, tile_stride=2, tile_count=3) if own == "strided" else {}
    c0 = pi.case("loop_3")
    r = Rig(crt, None, inp.scene_xml(tmp_path, c0.scene), 48, 40, **cfg)
    c = pi.Case(c0.scene, c0.T, c0.cameras, None, 1, 2, 1)
    acc = np.full((3, 40, 48, 4), SENTINEL_F, np.float32); px = np.full((3, 40, 48), SENTINEL_U, np.uint32)
    assert raw_poses(r.ctx, r.records(c.cameras), np.ascontiguousarray(c.T.reshape(3, -1, 16)), None, 1, 2, 1, 0.5, acc, px) == 0
    owned = np.zeros((40, 48), bool)
    for t in ([1, 3, 5] if own == "strided" else range(6)):
        owned[16 * (t // 3):16 * (t // 3) + 16, 16 * (t % 3):16 * (t % 3) + 16] = True
    want = r.loop(c)[0]
    for k in range(3):
        assert same(acc[k][owned], want[k][owned]), k
        assert (acc[k][~owned] == SENTINEL_F).all() and (px[k][~owned] == SENTINEL_U).all(), k
        assert (px[k][owned] != SENTINEL_U).all(), k
    r.close()


# 10: the device entry
def test_device_entry_on_a_side_stream(rigs):
    c = pi.case("straddle_3"); r = rigs(c.scene)
    scale = 0.25
    acc, px, nodes = r.run(c, scale=scale, want_tlas=True)
    k = len(c.cameras)
    side = torch.cuda.Stream(device=dev())
    with torch.cuda.stream(side):
        cams = torch.from_numpy(r.records(c.cameras)).to(dev()); T = torch.from_numpy(np.ascontiguousarray(c.T.reshape(len(c.T), -1, 16))).to(dev())
        vp = torch.tensor(c.view_pose, dtype=torch.int32, device=dev())
        out = torch.full((k, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
        pix = torch.full((k, H, W), 0x5A5A5A5A, dtype=torch.int32, device=dev())
    got, gpx, gnodes = r.ctx.render_poses_device(cams, T, out, c.spp_first, c.frames, c.passes, scale=scale, pixels=pix, view_pose=vp, want_tlas=True, stream=side)
    side.synchronize()
    assert got is out and gpx is pix
    assert same(out.cpu().numpy(), acc) and np.array_equal(pix.cpu().numpy().view(np.uint32), px) and gnodes.tobytes() == nodes.tobytes()
    out2 = torch.full((k, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
    r.ctx.render_poses_device(cams, T, out2, c.spp_first, c.frames, c.passes, view_pose=vp)      # the current (default) stream, no pixels, no nodes
    torch.cuda.synchronize()
    assert same(out2.cpu().numpy(), acc)


def test_an_update_behind_the_call_does_not_disturb_it(crt, tmp_path):
    c0 = pi.case("loop_3")
    c = pi.Case(c0.scene, c0.T, c0.cameras, None, 1, 16, 1)
    r = Rig(crt, None, inp.scene_xml(tmp_path, c.scene))
    want = r.loop(c)[0]
    cams, T = to_dev(r.records(c.cameras)), to_dev(c.T.reshape(3, -1, 16))
    out1, out2 = torch.zeros((3, H, W, 4), device=dev()), torch.zeros((3, H, W, 4), device=dev())
    moved = to_dev(pi.poses("tlas3", 5)[4])
    side = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    r.ctx.render_poses_device(cams, T, out1, 1, 16, stream=side)
    r.ctx.update_transforms_device(moved, stream=side)                       # a scene write submitted behind the job
    r.ctx.render_poses_device(cams, T, out2, 1, 16, stream=side)             # poses do not depend on the live TLAS
    side.synchronize()
    assert same(out1.cpu().numpy(), want) and same(out2.cpu().numpy(), want)
    r.close()


def test_a_job_of_three_launches(crt, rigs, tmp_path):
    c = pi.case("lanes_130"); r = rigs(c.scene)
    uncut = r.run(c, scale=0.5)
    cut = crt.Context(W, H, max_frames_per_launch=64)                        # one window of 64 view-frames per launch
    r.hs.upload(cut)
    got = r.run(c, ctx=cut, scale=0.5)
    assert same(got[0], uncut[0]) and np.array_equal(got[1], uncut[1])
    assert same(got[0], r.loop(c)[0])
    cut.close()


# 11: every row of the refusal table, the outputs' sentinel intact
def test_refusals_leave_the_outputs_alone(rigs, crt, tmp_path):
    c = pi.case("loop_3"); r = rigs(c.scene); ctx = r.ctx; L = ctx.L
    k, n = 3, c.T.shape[1]
    cams_h, T_h = r.records(c.cameras), np.ascontiguousarray(c.T.reshape(3, -1, 16))
    cams, T = to_dev(cams_h), to_dev(T_h)
    out = torch.full((k * H * W * 4 + 4,), float(SENTINEL_F), dtype=torch.float32, device=dev())
    vp = to_dev([0, 1, 2], np.int32)
    host_out = np.zeros((k, H, W, 4), np.float32)

    def call(d_cams, d_T, d_out, c_=ctx, kk=k, P=3, blas=n, d_vp=None, frames=1, passes=1, stream=None):
        return L.crt_render_poses_device(c_.h, C.c_void_p(d_cams), C.c_uint32(kk), C.c_void_p(d_T), C.c_uint32(P), C.c_uint32(blas), C.c_void_p(d_vp), C.c_uint32(1), C.c_uint32(frames),
                                         C.c_uint32(passes), C.c_float(1.0), C.c_void_p(d_out), None, None, stream)
    a, t, o = cams.data_ptr(), T.data_ptr(), out.data_ptr()
    assert call(a, t, o, blas=n + 1) == INVALID                              # blasCount
    assert call(a, t, o, P=0) == INVALID                                     # no pose
    assert call(a, t, o, P=2) == INVALID                                     # view_pose NULL with P != K
    assert call(a, t, o, P=2, d_vp=vp.data_ptr()) == INVALID                 # an entry outside [0, P): the device entry's check
    assert b"view_pose[2]" in L.crt_last_error(ctx.h)
    assert call(a, t, o, passes=0) == INVALID and call(a, t, o, passes=5) == INVALID
    assert call(a, t, host_out.ctypes.data) == INVALID                       # host pointers
    assert call(cams_h.ctypes.data, t, o) == INVALID
    assert call(a, T_h.ctypes.data, o) == INVALID
    assert call(a, t, o, d_vp=np.zeros(3, np.int32).ctypes.data) == INVALID
    assert call(a, t, o + 4) == INVALID and b"16-byte" in L.crt_last_error(ctx.h)
    assert call(a, t + 2, o) == INVALID                                      # misaligned
    assert call(None, t, o) == INVALID and call(a, None, o) == INVALID and call(a, t, None) == INVALID
    if torch.cuda.device_count() > 1:
        assert call(a, t, o, stream=C.c_void_p(torch.cuda.Stream(device=torch.device("cuda", 1)).cuda_stream)) == INVALID
    assert call(a, t, o, kk=1 << 16, P=1 << 16, frames=1 << 16) == UNSUPPORTED         # more than 2^31-1 view-frames
    assert call(a, t, o, kk=1, P=1 << 23, d_vp=vp.data_ptr()) == UNSUPPORTED and b"4 GiB" in L.crt_last_error(ctx.h)     # 2^23 poses of three instances: a table of over 4 GiB
    # K = 0 and frames = 0: no-ops after the checks that need no buffer
    assert call(None, None, None, kk=0, P=0) == 0 and call(None, None, None, frames=0) == 0 and call(None, None, None, kk=0, P=0, passes=9) == INVALID
    # the host entry's own: NULL buffers, view_pose looked at before anything runs
    acc = np.full((k, H, W, 4), SENTINEL_F, np.float32)
    assert raw_poses(ctx, cams_h, T_h, np.array([0, 3, 1], np.int32), 1, 1, 1, 1.0, acc, None) == INVALID and b"view_pose[1] = 3" in L.crt_last_error(ctx.h)
    assert raw_poses(ctx, cams_h, T_h, None, 1, 1, 1, 1.0, None, None) == INVALID
    assert raw_poses(ctx, cams_h, T_h, None, 1, 0, 1, 1.0, acc, None) == 0 and (acc == SENTINEL_F).all()
    # another accelerator selected
    hs = crt.HostScene(r.xml, 1, ASSETS); hs.build_alt(crt.ACCEL_KDTREE)
    kd = crt.Context(W, H); hs.upload(kd); hs.upload_alt(kd, crt.ACCEL_KDTREE); kd.set_render_accel(crt.ACCEL_KDTREE)
    assert call(a, t, o, c_=kd) == UNSUPPORTED
    kd.set_render_accel(0)
    assert call(a, t, o, c_=kd) == 0                                         # ... and with the BVH selected again the job runs
    torch.cuda.synchronize()
    assert same(out.cpu().numpy()[:k * H * W * 4].reshape(k, H, W, 4), r.loop(pi.Case(c.scene, c.T, c.cameras, None, 1, 1, 1))[0])
    out.fill_(float(SENTINEL_F)); torch.cuda.synchronize()
    kd.close()
    # no scene; a FileScene; a PrimitiveScene
    fresh = crt.Context(W, H)
    assert call(a, t, o, c_=fresh) == STATE
    crt.HostScene(scene_path("cube_scene.xml"), 0, ASSETS).upload(fresh)
    assert call(a, t, o, c_=fresh, blas=1) == INVALID
    fresh.close()
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(0.0)
    pc = crt.Context(W, H); ps.upload(pc)
    assert call(a, t, o, c_=pc) == UNSUPPORTED
    pc.close()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL_F).all() and not host_out.any() and (acc == SENTINEL_F).all()


def test_a_pose_too_tall_for_the_lds_stack_is_refused(crt):
    """16 chain BLASes of height 40: under the TLAS of a 4 x 4 grid (height 5) the stack is 40 + 5 + 1 = 46 dwords per lane and the job runs; one pose whose transforms
    make a caterpillar (height 15) puts it at 56, beyond the 49 that four wavefronts' columns and factors leave of a workgroup's 64 KiB"""
    from test_gpu_tlas_device import chain_blas
    N, tris = 16, 41
    bvhs = [chain_blas(crt, tris, i + 2) for i in range(N)]
    boxes = np.stack([np.stack([b["nodes"][0]["aabbMin"], b["nodes"][0]["aabbMax"]]) for b in bvhs])
    flat = np.stack([inp.rigid((i % 4 - 1.5, i // 4 - 1.5, 5.0)) for i in range(N)])
    line = np.stack([inp.rigid((4.0 ** i, 0.0, 5.0)) for i in range(N)])
    first = inp.restate(boxes, flat)
    assert first["height"] == 5 and inp.restate(boxes, line)["height"] == 15
    for b, t, it in zip(bvhs, flat, first["invT"]):
        b.update(T=t, invT=it.reshape(4, 4))
    tex = np.full((4, 4), 0x808080, np.uint32); ident = np.eye(4, dtype=np.float32)
    ctx = crt.Context(W, H)
    ctx.upload_desc(crt.SCENE_TLAS, bvhs, tlas_nodes=first["nodes"], textures=[tex, tex], floor_texture=0, sky_texture=1, materials=[(0.0, 0.0, (0.0, 0.0, 0.0), -1)],
                    light_T=ident, light_invT=ident)
    cams = crt.camera_records(W, H, [((0.0, 0.0, 0.0), (0.0, 0.0, 5.0)), ((0.5, 0.0, 0.0), (0.0, 0.0, 5.0))])
    ok = ctx.render_poses(cams, np.stack([flat, flat]).reshape(2, N, 16), 1, 1)
    assert np.isfinite(ok).all()
    acc = np.full((2, H, W, 4), SENTINEL_F, np.float32)
    assert raw_poses(ctx, cams, np.ascontiguousarray(np.stack([flat, line]).reshape(2, N, 16)), None, 1, 1, 1, 1.0, acc, None) == UNSUPPORTED
    msg = ctx.L.crt_last_error(ctx.h).decode()
    assert "pose 1" in msg and (acc == SENTINEL_F).all(), msg
    assert same(ctx.render_poses(cams, np.stack([flat, flat]).reshape(2, N, 16), 1, 1), ok)
    ctx.close()


def test_a_failed_device_allocation_is_refused(rigs):
    """the refusal table's last row: the host entry's staging for 2^26 views of 32 x 16 pixels is 512 GiB, which hipMalloc refuses at once, before a camera, a
    transform or an image is read.  One pose and a view_pose of zeros keep the pose table small and K * frames below 2^31."""
    c = pi.case("loop_3"); r = rigs(c.scene); ctx = r.ctx
    want = r.loop(c)[0]
    assert same(r.run(c), want)                                              # (staging of the usual size is in place)
    K = 1 << 26
    cams = r.records(c.cameras[:1]); T = np.ascontiguousarray(c.T[:1].reshape(1, -1, 16))
    vp = np.zeros(K, np.int32)
    acc = np.full((1, H, W, 4), SENTINEL_F, np.float32); px = np.full((1, H, W), SENTINEL_U, np.uint32)
    nodes = np.zeros((1, 2 * T.shape[1]), inp.TLAS_DTYPE); nodes.view(np.uint8)[:] = 0x5A
    keep = nodes.tobytes()
    p = lambda a: a.ctypes.data_as(C.c_void_p)                               # noqa: E731
    rc = ctx.L.crt_render_poses(ctx.h, p(cams), C.c_uint32(K), p(T), C.c_uint32(1), C.c_uint32(T.shape[1]), p(vp), C.c_uint32(1), C.c_uint32(1), C.c_uint32(1), C.c_float(1.0),
                                p(acc), p(px), p(nodes))
    assert rc == DEVICE, rc
    msg = ctx.L.crt_last_error(ctx.h).decode()
    assert "hipMalloc" in msg, msg
    assert (acc == SENTINEL_F).all() and (px == SENTINEL_U).all() and nodes.tobytes() == keep
    assert same(r.run(c), want)                                              # the context has dropped its staging and takes the next job as usual
    scale = 0.25
    got = r.run(c, scale=scale, want_tlas=True)
    assert same(got[0], want) and np.array_equal(got[1], r.loop(c, scale=scale)[1])
