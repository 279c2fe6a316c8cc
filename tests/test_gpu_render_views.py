"""crt_render_views / crt_render_views_device: the frames of many cameras in one render job (csrc/device/render_views.h).  Every comparison is bit for bit
(np.array_equal) against one or both of
  the loop    set_camera_state + clear + render + accumulator per view, through the existing entries;
  the oracle  set_camera_state, set_spp, set_params, render.
The cameras and shapes are tests/render_views_inputs.py's; tests/test_render_views_cpu.py holds, without a GPU, that the oracle's views of every case see the mesh
and differ from each other, so a view-frame that lands in the wrong view cannot pass here.  Each case is there for a place the kernels can go wrong: the seed of a
non-zero start, the pass order, a camera per lane, a last window of one lane, views that straddle windows and launches, truncated rows, tile ownership, every world."""
import ctypes as C

import numpy as np
import pytest

import render_views_inputs as vi
from conftest import ASSETS, scene_path

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H = vi.W, vi.H
SENTINEL_F, SENTINEL_U = np.float32(-7.25), np.uint32(0xDEADBEEF)


class World:
    """a context with its scene, the oracle of the same scene, and the two references per view — each computed once and kept unchanged"""

    def __init__(self, crt, orc, world, width=W, height=H, **cfg):
        self.crt, self.world, self.W, self.H = crt, world, width, height
        self.ctx = crt.Context(width, height, **cfg)
        xml, kind = vi.scene_of(world)
        if xml is None:
            self.hs = crt.HostPrimitiveScene(ASSETS); self.hs.set_time(0.0); self.hs.upload(self.ctx)
        else:
            self.hs = crt.HostScene(scene_path(xml), kind, ASSETS)
            accel = {"kd": crt.ACCEL_KDTREE, "grid": crt.ACCEL_GRID, "tlas_kd": crt.ACCEL_KDTREE}.get(world, 0)
            if accel:
                self.hs.build_alt(accel)
            self.hs.upload(self.ctx)
            if accel:
                self.hs.upload_alt(self.ctx, accel); self.ctx.set_render_accel(accel)
        self.o = vi.make_oracle(orc, ASSETS, scene_path, world, width, height) if orc is not None else None
        self._loop, self._oracle = {}, {}

    def records(self, cameras):
        return self.crt.camera_records(self.W, self.H, cameras)

    def loop(self, cameras, spp_first, frames, passes=1):
        out = []
        for cam in cameras:
            key = (cam, spp_first, frames, passes)
            if key not in self._loop:
                self.ctx.set_camera_state(*cam); self.ctx.clear(); self.ctx.render(spp_first, frames, passes)
                a = self.ctx.accumulator(); a.setflags(write=False)
                self._loop[key] = a
            out.append(self._loop[key])
        return np.stack(out)

    def oracle(self, cameras, spp_first, frames, passes=1):
        out = []
        for cam in cameras:
            key = (cam, spp_first, frames, passes)
            if key not in self._oracle:
                a = vi.oracle_view(self.o, cam, spp_first, frames, passes)[0]; a.setflags(write=False)
                self._oracle[key] = a
            out.append(self._oracle[key])
        return np.stack(out)

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def worlds(crt, orc):
    cache = {}

    def get(world):
        if world not in cache:
            cache[world] = World(crt, orc, world)
        return cache[world]
    yield get
    for w in cache.values():
        w.close()


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def raw_views(ctx, cams, spp_first, frames, passes, scale, acc, px):
    """crt_render_views into arrays the caller has filled"""
    return ctx.L.crt_render_views(ctx.h, cams.ctypes.data_as(C.c_void_p), C.c_uint32(len(cams)), C.c_uint32(spp_first), C.c_uint32(frames), C.c_uint32(passes), C.c_float(scale),
                                  acc.ctypes.data_as(C.c_void_p), px.ctypes.data_as(C.c_void_p) if px is not None else None)


# 1 - 4: identity, a non-zero start with passes, a camera per lane over window boundaries, views that straddle windows
@pytest.mark.parametrize("case", list(vi.CASES))
def test_views_equal_the_loop_and_the_oracle(worlds, case):
    w = worlds("bvh")
    cameras, spp_first, frames, passes = vi.CASES[case]
    got = w.ctx.render_views(w.records(cameras), spp_first, frames, passes)
    assert got.shape == (len(cameras), H, W, 4) and got.dtype == np.float32
    want = w.oracle(cameras, spp_first, frames, passes)
    bad = [k for k in range(len(cameras)) if not same(got[k], want[k])]
    assert not bad, (case, "oracle", bad[:8])
    assert same(got, w.loop(cameras, spp_first, frames, passes)), (case, "loop")
    assert (got[..., 3].view(np.uint32) == 0).all()                        # w = +0, as crt_clear + the accumulate leave it


# 5: the rows the 16-row tiling truncates, and the tiles the context does not own, stay as the caller left them
@pytest.mark.parametrize("own", ["all", "strided"])
def test_truncated_rows_and_foreign_tiles_are_not_touched(crt, own):
    cfg = dict(tile_first=1, tile_stride=2, tile_count=3) if own == "strided" else {}
    w = World(crt, None, "bvh", 48, 40, **cfg)
    cameras = vi.ring(3)
    cams = w.records(cameras)
    acc = np.full((3, 40, 48, 4), SENTINEL_F, np.float32); px = np.full((3, 40, 48), SENTINEL_U, np.uint32)
    assert raw_views(w.ctx, cams, 1, 2, 1, 0.5, acc, px) == 0
    owned = np.zeros((40, 48), bool)
    for t in ([1, 3, 5] if own == "strided" else range(6)):
        owned[16 * (t // 3):16 * (t // 3) + 16, 16 * (t % 3):16 * (t % 3) + 16] = True
    assert not owned[32:].any() and owned.sum() == (3 if own == "strided" else 6) * 256
    want = w.loop(cameras, 1, 2, 1)
    for k in range(3):
        assert same(acc[k][owned], want[k][owned]), k
        assert (acc[k][~owned] == SENTINEL_F).all() and (px[k][~owned] == SENTINEL_U).all(), k
        assert (px[k][owned] != SENTINEL_U).all(), k
    w.close()


# 6: every world
@pytest.mark.parametrize("world", vi.WORLDS)
def test_every_world(worlds, world):
    w = worlds(world)
    cameras = vi.world_cameras(world)
    spp_first, frames, passes = vi.WORLD_SHAPE
    got = w.ctx.render_views(w.records(cameras), spp_first, frames, passes)
    assert same(got, w.oracle(cameras, spp_first, frames, passes)), (world, "oracle")
    assert same(got, w.loop(cameras, spp_first, frames, passes)), (world, "loop")


# 7: the lanes of a wavefront are independent
def test_lanes_are_independent(worlds):
    w = worlds("bvh")
    a, b = vi.ring(2)
    four = w.ctx.render_views(w.records([a, a, a, a]), 1, 1)
    assert same(four[0], w.loop([a], 1, 1)[0])
    for k in (1, 2, 3):
        assert same(four[k], four[0]), k
    mixed = w.ctx.render_views(w.records([a, a, b, a]), 1, 1)
    for k in (0, 1, 3):
        assert same(mixed[k], four[0]), k
    assert same(mixed[2], w.loop([b], 1, 1)[0]) and not same(mixed[2], four[0])


# 8: the pixels are resolve_screen's
def test_pixels_are_resolve_screens(worlds):
    w = worlds("bvh")
    cameras, spp_first, frames, passes = vi.CASES["start_and_passes"]
    scale = 1.0 / (spp_first + frames * passes)
    acc, px = w.ctx.render_views(w.records(cameras), spp_first, frames, passes, scale=scale)
    assert px.shape == (len(cameras), H, W) and px.dtype == np.uint32
    only = w.ctx.render_views(w.records(cameras), spp_first, frames, passes)              # no pixels asked for
    assert same(only, acc)
    for k, cam in enumerate(cameras):
        w.ctx.set_camera_state(*cam); w.ctx.clear(); w.ctx.render(spp_first, frames, passes)
        want, _ = w.ctx.resolve_screen(scale)
        assert same(acc[k], w.ctx.accumulator()) and np.array_equal(px[k], want), k
    assert len(np.unique(px)) > 8


# 9: the context's own state
def test_camera_and_accumulator_are_left_alone(worlds):
    w = worlds("bvh")
    cameras = vi.ring(5)
    home = cameras[4]
    w.ctx.set_camera_state(*home); w.ctx.clear(); w.ctx.render(3, 2, 1)
    before = w.ctx.accumulator()
    w.ctx.render_views(w.records(cameras[:4]), 1, 2)
    assert same(w.ctx.accumulator(), before)                                 # the accumulator
    w.ctx.render(5, 1, 1)                                                    # ... and the camera: the next frame is the home camera's
    after = w.ctx.accumulator()
    w.ctx.clear(); w.ctx.render(3, 3, 1)
    assert same(after, w.ctx.accumulator()) and not same(after, before)
    assert same(after, w.loop([home], 3, 3)[0])


def test_a_tick_sequence_around_the_call_keeps_its_pixels(crt):
    a, b = World(crt, None, "bvh"), World(crt, None, "bvh")
    cams = a.records(vi.ring(4))
    cam = vi.ring(7)[3]
    a.ctx.set_camera_state(*cam); b.ctx.set_camera_state(*cam)
    for spp in range(1, 7):
        if spp == 4:
            a.ctx.render_views(cams, 1, 2)
        pa, ra, ea = a.ctx.tick(spp)
        pb, rb, eb = b.ctx.tick(spp)
        assert np.array_equal(pa, pb) and same(ra, rb) and ea == eb, spp
    a.close(); b.close()


def test_counters_grow_as_for_the_loop(crt):
    w = World(crt, None, "bvh")
    cameras, spp_first, frames, passes = vi.ring(5), 2, 3, 2
    keys = ("rays", "primary", "mesh_hits")
    w.ctx.sync(); c0 = w.ctx.counters()
    w.ctx.render_views(w.records(cameras), spp_first, frames, passes)
    c1 = w.ctx.counters()
    w.loop(cameras, spp_first, frames, passes)
    w.ctx.sync(); c2 = w.ctx.counters()
    assert {k: c1[k] - c0[k] for k in keys} == {k: c2[k] - c1[k] for k in keys}
    assert c1["primary"] - c0["primary"] == 5 * 3 * 2 * 2 * 256 and c1["mesh_hits"] > c0["mesh_hits"]
    w.close()


# 10: the device entry
def dev():
    return torch.device("cuda", 0)


def test_device_entry_on_a_side_stream_equals_the_host_entry(worlds):
    w = worlds("bvh")
    cameras, spp_first, frames, passes = vi.CASES["straddle_3"]
    scale = 0.25
    acc, px = w.ctx.render_views(w.records(cameras), spp_first, frames, passes, scale=scale)
    k = len(cameras)
    side = torch.cuda.Stream(device=dev())
    with torch.cuda.stream(side):
        cams = torch.from_numpy(w.records(cameras)).to(dev(), non_blocking=False)
        out = torch.full((k, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
        pix = torch.full((k, H, W), 0x5A5A5A5A, dtype=torch.int32, device=dev())
    got, gpx = w.ctx.render_views_device(cams, out, spp_first, frames, passes, scale=scale, pixels=pix, stream=side)
    side.synchronize()
    assert got is out and gpx is pix
    assert same(out.cpu().numpy(), acc) and np.array_equal(pix.cpu().numpy().view(np.uint32), px)
    out2 = torch.full((k, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
    w.ctx.render_views_device(cams, out2, spp_first, frames, passes)                     # the current (default) stream, no pixels
    torch.cuda.synchronize()
    assert same(out2.cpu().numpy(), acc)


def test_a_scene_update_behind_the_call_does_not_change_its_result(crt, worlds):
    w = worlds("tlas")
    cameras = vi.ring(8, vi.TLAS_CENTRE, 5.0)
    before = w.loop(cameras, 1, 16)
    hs = crt.HostScene(scene_path("tlas_scene.xml"), 1, ASSETS); ctx = crt.Context(W, H); hs.upload(ctx)
    T = hs.blas_transform(2)[0].reshape(4, 4).copy()
    T[:3, 3] += np.array([-0.8, 0.5, 0.3], np.float32)                       # the teapot moves
    cams = torch.from_numpy(w.records(cameras)).to(dev())
    out1, out2 = torch.zeros((8, H, W, 4), device=dev()), torch.zeros((8, H, W, 4), device=dev())
    side = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    ctx.render_views_device(cams, out1, 1, 16, stream=side)
    hs.set_transform(2, T); hs.update(ctx, crt.UPDATE_TRANSFORMS)            # no host sync in between
    ctx.render_views_device(cams, out2, 1, 16, stream=side)
    side.synchronize()
    assert same(out1.cpu().numpy(), before)
    assert not same(out2.cpu().numpy(), before)                              # the move is visible from these cameras
    ctx.close()


def test_refusals_leave_the_output_alone(worlds, crt):
    w = worlds("bvh"); ctx = w.ctx
    k = 2
    cams = torch.from_numpy(w.records(vi.ring(k))).to(dev())
    out = torch.full((k * H * W * 4 + 4,), float(SENTINEL_F), dtype=torch.float32, device=dev())
    host = np.zeros((k, H, W, 4), np.float32)

    def call(d_cams, d_out, passes=1, kk=k, frames=1):
        return ctx.L.crt_render_views_device(ctx.h, C.c_void_p(d_cams), C.c_uint32(kk), C.c_uint32(1), C.c_uint32(frames), C.c_uint32(passes), C.c_float(1.0), C.c_void_p(d_out), None, None)
    assert call(cams.data_ptr(), host.ctypes.data) == -1                     # a host pointer
    assert call(host.ctypes.data, out.data_ptr()) == -1
    assert call(cams.data_ptr(), out.data_ptr() + 4) == -1                   # misaligned d_out_rgba (4-byte, not 16-byte aligned)
    assert b"16-byte" in ctx.L.crt_last_error(ctx.h)
    assert call(None, out.data_ptr()) == -1                                  # NULL d_cams
    assert call(cams.data_ptr(), None) == -1
    assert call(cams.data_ptr(), out.data_ptr(), passes=9) == -1             # crt_render's code
    assert call(cams.data_ptr(), out.data_ptr(), kk=1 << 16, frames=1 << 16) == -4      # more than 2^31-1 view-frames
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL_F).all() and not host.any()
    # K = 0 and frames = 0: no-ops after the checks that need no buffer
    assert call(None, None, kk=0) == 0 and call(None, None, frames=0) == 0 and call(None, None, kk=0, passes=9) == -1
    acc = np.full((k, H, W, 4), SENTINEL_F, np.float32)
    assert raw_views(ctx, w.records(vi.ring(k)), 1, 0, 1, 1.0, acc, None) == 0 and (acc == SENTINEL_F).all()
    assert raw_views(ctx, w.records(vi.ring(k)), 1, 1, 0, 1.0, acc, None) == -1 and (acc == SENTINEL_F).all()
    fresh = crt.Context(W, H)                                                # no scene
    assert fresh.L.crt_render_views_device(fresh.h, C.c_void_p(cams.data_ptr()), C.c_uint32(k), C.c_uint32(1), C.c_uint32(1), C.c_uint32(1), C.c_float(1.0), C.c_void_p(out.data_ptr()), None, None) == -5
    fresh.close()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL_F).all()


# 11: a job cut into several launches equals the uncut one
@pytest.mark.parametrize("case", ["lanes_130", "straddle_3", "straddle_70"])
def test_a_job_of_several_launches(crt, worlds, case):
    cameras, spp_first, frames, passes = vi.CASES[case]
    w = worlds("bvh")
    uncut = w.ctx.render_views(w.records(cameras), spp_first, frames, passes, scale=0.5)
    cut = World(crt, None, "bvh", max_frames_per_launch=64)                  # one window of 64 view-frames per launch: three launches
    got = cut.ctx.render_views(cut.records(cameras), spp_first, frames, passes, scale=0.5)
    assert same(got[0], uncut[0]) and np.array_equal(got[1], uncut[1])
    assert same(got[0], w.oracle(cameras, spp_first, frames, passes))
    cut.close()
