"""crt_render_shape_sets / crt_render_shape_sets_device: the frames of many cameras over many job-local shapes of a two-level scene in which SEVERAL BLASes deform
(csrc/device/shape_build.hip's set kernels, render_shape_sets.h).  Every comparison is bit for bit (np.array_equal on the uint32 views) against
  the loop    refit_device(bvhs[m], ...) for every m + update_transforms_device(T[s]) + set_camera_state + clear + render + accumulator per view, through the existing
              entries, on a SECOND context;
  the oracle  move_and_refit of every BVH of the set, set_transform for every instance, set_camera_state, render.
The scenes, sets and cameras are tests/render_shape_sets_inputs.py's; tests/test_render_shape_sets_cpu.py holds, without a GPU, that the refits of a set commute, that
every mesh of every case is seen deforming and that no two shapes look alike through one camera, so a lane that walks the wrong sub-image cannot pass here."""
import ctypes as C

import numpy as np
import pytest

import render_shape_sets_inputs as ss
import render_shapes_inputs as si
import tlas_device_inputs as inp
from conftest import ASSETS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H = ss.W, ss.H
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
    """a scene on two contexts — `ctx` takes the entry, `ref` runs the loop — and its oracle.  `ref` and the oracle keep what the last refit left in a BVH, so a rig
    serves ONE set of BVHs: every loop iteration and every oracle view refits all of them.  Every reference is computed once and kept unchanged."""

    def __init__(self, crt, orc, tmp, scene, width=W, height=H, **cfg):
        self.crt, self.W, self.H = crt, width, height
        self.xml, self.kind = ss.scene_xml(tmp, scene)
        self.hs = crt.HostScene(self.xml, self.kind, ASSETS)
        self.ctx, self.ref = crt.Context(width, height, **cfg), crt.Context(width, height, **cfg)
        self.hs.upload(self.ctx); self.hs.upload(self.ref)
        self.o = ss.make_oracle(orc, tmp, scene, width, height) if orc is not None else None
        self._loop, self._oracle = {}, {}

    def case(self, name, **kw):
        return ss.case(name, self.hs, **kw)

    def records(self, cameras):
        return self.crt.camera_records(self.W, self.H, cameras)

    def _key(self, c, k):
        s = c.shape_of(k)
        return (tuple(c.bvhs), tuple(p[s].tobytes() for p in c.pos), c.T[s].tobytes(), c.cameras[k], c.spp_first, c.frames, c.passes)

    def loop(self, c, views=None, scale=None):
        """(accumulators, pixels or None, {(shape, m): box}, {shape: nodes}) of the views through the existing entries on `ref`; the refits in the order of bvhs for even
        shapes and in the opposite order for odd ones"""
        acc, px, boxes, nodes = [], [], {}, {}
        for k in (range(len(c.cameras)) if views is None else views):
            s = c.shape_of(k)
            key = self._key(c, k) + (scale,)
            if key not in self._loop:
                order = list(range(len(c.bvhs)))[::-1 if s % 2 else 1]
                box = {m: self.ref.refit_device(c.bvhs[m], to_dev(c.pos[m][s])) for m in order}
                n = self.ref.update_transforms_device(to_dev(c.T[s]))
                self.ref.set_camera_state(*c.cameras[k]); self.ref.clear(); self.ref.render(c.spp_first, c.frames, c.passes)
                a = self.ref.accumulator(); a.setflags(write=False)
                self._loop[key] = (a, self.ref.resolve_screen(scale)[0] if scale is not None else None, box, n)
            a, x, box, n = self._loop[key]
            acc.append(a); px.append(x); nodes[s] = n
            for m, b in box.items():
                boxes[(s, m)] = b
        return np.stack(acc), (np.stack(px) if scale is not None else None), boxes, nodes

    def oracle(self, c, views=None):
        out = []
        for k in (range(len(c.cameras)) if views is None else views):
            key = self._key(c, k)
            if key not in self._oracle:
                a = ss.oracle_view(self.o, c, k)[0]; a.setflags(write=False)
                self._oracle[key] = a
            out.append(self._oracle[key])
        return np.stack(out)

    def run(self, c, ctx=None, flat=False, **kw):
        T = c.T.reshape(len(c.T), -1, 16)
        return (ctx or self.ctx).render_shape_sets(self.records(c.cameras), c.bvhs, c.set_positions() if flat else c.pos, c.spp_first, c.frames, c.passes, T=T,
                                                   view_shape=c.view_shape, **kw)

    def close(self):
        self.ctx.close(); self.ref.close()


@pytest.fixture(scope="module")
def rigs(crt, orc, tmp_path_factory):
    cache, tmp = {}, tmp_path_factory.mktemp("shape_sets")

    def get(name):
        """the rig of case `name`'s scene and set"""
        key = (ss.case_scene(name), tuple(sorted(ss.CASE_BVHS[name])))
        if key not in cache:
            cache[key] = Rig(crt, orc, tmp, key[0])
        return cache[key]
    yield get
    for r in cache.values():
        r.close()


def raw_sets(ctx, cams, bvhs, pos, T, vs, spp_first, frames, passes, scale, acc, px, boxes=None, nodes=None, S=None, tris=None, n=None, K=None, M=None):
    """crt_render_shape_sets into arrays the caller has filled"""
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    ids = None if bvhs is None else np.ascontiguousarray(bvhs, np.uint32)
    return ctx.L.crt_render_shape_sets(ctx.h, p(cams), C.c_uint32(len(cams) if K is None else K), p(ids), C.c_uint32((0 if ids is None else len(ids)) if M is None else M), p(pos),
                                       C.c_uint32(len(pos) if S is None else S), C.c_uint32(pos.shape[1] if tris is None else tris), p(T),
                                       C.c_uint32((0 if T is None else T.shape[1]) if n is None else n), p(vs), C.c_uint32(spp_first), C.c_uint32(frames), C.c_uint32(passes),
                                       C.c_float(scale), p(acc), p(px), p(boxes), p(nodes))


def check_against_loop_and_oracle(r, c, name, full=True):
    scale = 1.0 / (c.spp_first + c.frames * c.passes)
    acc, px, nodes, boxes = r.run(c, scale=scale, want_root_boxes=True, want_tlas=True)
    k, S, M = len(c.cameras), len(c.T), len(c.bvhs)
    assert acc.shape == (k, H, W, 4) and px.shape == (k, H, W) and boxes.shape == (S, M, 2, 3) and nodes.shape == (S, 2 * c.T.shape[1])
    want, want_px, want_boxes, want_nodes = r.loop(c, scale=scale)
    bad = [v for v in range(k) if not same(acc[v], want[v])]
    assert not bad, (name, "loop", bad[:8])
    assert np.array_equal(px, want_px)
    for (s, m), b in want_boxes.items():
        assert same(boxes[s, m], b), (name, "root box", s, m)
    for s, n in want_nodes.items():
        assert nodes[s].tobytes() == n.tobytes(), (name, "tlas", s)
    assert same(acc, r.oracle(c)), (name, "oracle")
    assert (acc[..., 3].view(np.uint32) == 0).all()                        # w = +0
    if full:
        assert same(r.run(c, flat=True), acc)                               # one [S, setTris, 9] array; no pixels, no boxes, no nodes asked for
    return acc


# the loop and the oracle: accumulator, pixels with a scale, root boxes, TLAS nodes, counters
@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("name", ss.LOOP_CASES)
def test_sets_equal_the_loop_and_the_oracle(rigs, name, passes):
    r = rigs(name)
    c = r.case(name, passes=passes)
    assert len(c.cameras) == len(c.T) == 3 and c.frames == 2
    check_against_loop_and_oracle(r, c, name)
    # counters: the job's three grow by what the loop's K renders add (the refits and TLAS builds count nothing)
    fields = ("rays", "primary", "mesh_hits")
    r.ctx.reset_counters(); r.ref.reset_counters()
    r.run(c)
    r._loop.clear(); r.loop(c)
    got, want = r.ctx.counters(), r.ref.counters()
    assert got["primary"] == 3 * 2 * 256 * c.frames * c.passes and got["mesh_hits"] > 0
    assert {f: got[f] for f in fields} == {f: want[f] for f in fields}


# M = 1: bit for bit what crt_render_shapes gives for the same job
def test_one_mesh_is_render_shapes(rigs):
    r = rigs("tlas3_two")
    c = si.case("tlas3_loop", r.hs)
    cams, T = r.records(c.cameras), c.T.reshape(len(c.T), -1, 16)
    want = r.ctx.render_shapes(cams, c.bvh, c.pos, c.spp_first, c.frames, c.passes, scale=0.2, T=T, want_root_boxes=True, want_tlas=True)
    for positions in ([c.pos], c.pos.reshape(len(c.pos), -1, 9)):
        got = r.ctx.render_shape_sets(cams, [c.bvh], positions, c.spp_first, c.frames, c.passes, scale=0.2, T=T, want_root_boxes=True, want_tlas=True)
        assert same(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()
        assert got[3].shape == (3, 1, 2, 3) and same(got[3][:, 0], want[3])


# a shape per lane (one full window and a partial one); views that straddle windows, three views over two shapes
@pytest.mark.parametrize("name", ["ring40_five", "windows_48"])
def test_a_shape_per_lane_and_views_across_windows(rigs, name):
    r = rigs(name)
    c = r.case(name)
    acc = r.run(c)
    assert same(acc, r.oracle(c)), (name, "oracle")
    views = [0, 1, 63, 64, 68] if name == "ring40_five" else None            # (the loop for the window's edges; the oracle holds every view)
    want = r.loop(c, views)[0]
    bad = [v for i, v in enumerate(views or range(len(c.cameras))) if not same(acc[v], want[i])]
    assert not bad, (name, "loop", bad)


# node 1 of EACH deforming BVH keeps the live scene's box; roots that are leaves have no pair at all
@pytest.mark.parametrize("name", ["stale_node1", "leaf_root"])
def test_stale_node1_and_leaf_roots(rigs, name):
    r = rigs(name)
    check_against_loop_and_oracle(r, r.case(name), name)


# every BLAS of the scene deforms; shapes whose TLASes differ in height in one job, and the job with the shapes reversed
def test_all_forty_deform_with_mixed_heights_and_reversed(rigs):
    r = rigs("ring40_all")
    c = r.case("ring40_all")
    fwd = r.run(c, want_root_boxes=True, want_tlas=True)
    assert same(fwd[0], r.oracle(c))
    want, _, want_boxes, want_nodes = r.loop(c)
    assert same(fwd[0], want)
    assert all(same(fwd[2][s, m], b) for (s, m), b in want_boxes.items()) and all(fwd[1][s].tobytes() == n.tobytes() for s, n in want_nodes.items())
    got = r.run(c.reversed(), want_root_boxes=True, want_tlas=True)
    assert same(got[0], fwd[0][::-1]) and got[1].tobytes() == fwd[1][::-1].tobytes() and same(got[2], fwd[2][::-1])
    boxes = np.zeros((2, 40, 2, 3), np.float32)
    boxes[:, c.bvhs] = fwd[2]
    heights = [inp.restate(boxes[s], c.T[s])["height"] for s in (0, 1)]
    assert heights[0] != heights[1], heights


# the live scene is not changed
def test_the_live_scene_is_untouched(crt, tmp_path):
    r = Rig(crt, None, tmp_path, "tlas3")
    c = r.case("tlas3_all")
    ctx = r.ctx
    live = np.stack([r.hs.blas_transform(i)[0].reshape(4, 4) for i in range(r.hs.bvh_count())])
    live_T = to_dev(live)
    O, D = inp.aimed_rays(live)

    def state(x):
        b = [x.get_bvh(i) for i in range(r.hs.bvh_count())]
        x.set_camera_state(*c.cameras[0]); x.clear(); x.render(1, 2, 1)
        hits = x.find_nearest(O, D)
        nodes = x.update_transforms_device(live_T).tobytes()
        return (tuple(i["nodes"].tobytes() + i["indices"].tobytes() for i in b), x.accumulator().tobytes(),
                tuple(hits[f].tobytes() for f in ("t", "u", "v", "objIdx", "triIdx", "traversed", "tested")), nodes), hits

    before, hits = state(ctx)
    assert state(r.ref)[0] == before                                         # (the second context goes through the same calls, the job apart)
    assert (hits["objIdx"] >= 2).sum() > 50
    r.run(c, scale=0.5, want_root_boxes=True, want_tlas=True)
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


# the device entry, positions produced on the same side stream immediately before the call
def test_device_entry_behind_a_torch_operation(rigs):
    r = rigs("tlas3_two")
    c0 = r.case("tlas3_two")
    c = ss.Case(c0.scene, c0.bvhs, [[0.05, 0.23], [0.11, 0.07], [0.17, 0.31]], c0.p0, c0.T, c0.cameras, [2, 0, 1], 1, 3, 1)
    scale = 0.25
    want = r.run(c, scale=scale, want_root_boxes=True, want_tlas=True)
    k = len(c.cameras)
    side = torch.cuda.Stream(device=dev())
    base = to_dev(np.concatenate([p.reshape(-1, 3, 3) for p in c.p0]))                                     # [setTris, 3, 3]
    fac = to_dev(np.concatenate([np.repeat(c.factors[:, m:m + 1], len(c.p0[m]), axis=1) for m in range(2)], axis=1))   # [S, setTris]
    cams = to_dev(r.records(c.cameras)); vs = to_dev(c.view_shape, np.int32)
    T = to_dev(c.T.reshape(len(c.T), -1, 16))
    out = torch.full((k, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
    pix = torch.full((k, H, W), 0x5A5A5A5A, dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_pos = (base[None] + fac[:, :, None, None] * (base[..., [1, 2, 0]] * base[..., [2, 0, 1]])[None]).contiguous()      # no synchronisation before the call
        got = r.ctx.render_shape_sets_device(cams, c.bvhs, d_pos, out, c.spp_first, c.frames, c.passes, scale=scale, pixels=pix, T=T, view_shape=vs, want_root_boxes=True,
                                             want_tlas=True, stream=side)
    side.synchronize()
    assert same(d_pos.cpu().numpy().reshape(3, -1, 9), c.set_positions())   # (the torch expression is the numpy one, operation for operation)
    assert got[0] is out and got[1] is pix
    assert same(out.cpu().numpy(), want[0]) and np.array_equal(pix.cpu().numpy().view(np.uint32), want[1])
    assert got[2].tobytes() == want[2].tobytes() and same(got[3], want[3])
    out2 = torch.full((k, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
    r.ctx.render_shape_sets_device(cams, c.bvhs, d_pos, out2, c.spp_first, c.frames, c.passes, T=T, view_shape=vs)      # the current (default) stream, no optional output
    torch.cuda.synchronize()
    assert same(out2.cpu().numpy(), want[0])
    assert same(want[0], r.oracle(c))


# non-finite positions in one mesh of one shape; a view_shape entry out of range
def test_a_bad_mesh_refuses_the_job(rigs, crt):
    r = rigs("bad_mesh"); ctx = r.ctx
    c = r.case("bad_mesh")
    cams, T, pos = r.records(c.cameras), np.ascontiguousarray(c.T.reshape(3, -1, 16)), c.set_positions()
    ctx.set_camera_state(*c.cameras[0]); ctx.clear(); ctx.render(1, 2, 1)
    before = ctx.accumulator()
    acc = np.full((3, H, W, 4), SENTINEL_F, np.float32); px = np.full((3, H, W), SENTINEL_U, np.uint32)
    boxes = np.full((3, 2, 2, 3), SENTINEL_F, np.float32)
    nodes = np.zeros((3, 6), inp.TLAS_DTYPE); nodes.view(np.uint8)[:] = 0x5A
    keep = nodes.tobytes()
    assert raw_sets(ctx, cams, c.bvhs, pos, T, None, 1, 1, 1, 1.0, acc, px, boxes, nodes) == INVALID
    msg = ctx.L.crt_last_error(ctx.h).decode()
    assert "shape 1" in msg and "FindBestMatch" in msg and "crt_render_shape_sets" in msg, msg
    assert (acc == SENTINEL_F).all() and (px == SENTINEL_U).all() and (boxes == SENTINEL_F).all() and nodes.tobytes() == keep
    d_acc = torch.full((3, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev()); d_px = torch.full((3, H, W), 0x5A5A5A5A, dtype=torch.int32, device=dev())
    with pytest.raises(crt.CrtError) as e:                                   # the device entry learns of it with the headers
        ctx.render_shape_sets_device(to_dev(cams), c.bvhs, to_dev(pos), d_acc, 1, 1, scale=1.0, pixels=d_px, T=to_dev(T), want_tlas=True, want_root_boxes=True)
    assert e.value.code == INVALID and "shape 1" in str(e.value) and "crt_render_shape_sets_device" in str(e.value)
    torch.cuda.synchronize()
    assert (d_acc.cpu().numpy() == SENTINEL_F).all() and (d_px.cpu().numpy() == 0x5A5A5A5A).all()
    assert raw_sets(ctx, cams, c.bvhs, pos, T, np.array([0, 2, 2], np.int32), 1, 1, 1, 1.0, acc, px) == INVALID      # no view uses shape 1: it is still built, and still bad
    assert (acc == SENTINEL_F).all()
    pos_ok, T_ok = np.ascontiguousarray(pos[[0, 2]]), np.ascontiguousarray(T[[0, 2]])                                 # the job without the bad shape runs
    vs_ok = np.array([0, 1, 1], np.int32)
    got = ctx.render_shape_sets(cams, c.bvhs, pos_ok, 1, 1, T=T_ok, view_shape=vs_ok)
    ok = ss.Case(c.scene, c.bvhs, c.factors[[0, 2]], c.p0, c.T[[0, 2]], c.cameras, [0, 1, 1], 1, 1, 1)
    assert same(ok.set_positions(), pos_ok) and same(got, r.loop(ok)[0])
    # view_shape out of range: the host entry, then the device entry (which learns of it from the build launch)
    for bad_vs in ([0, 2, 1], [0, -1, 1]):
        assert raw_sets(ctx, cams, c.bvhs, pos_ok, T_ok, np.array(bad_vs, np.int32), 1, 1, 1, 1.0, acc, px) == INVALID
        assert b"view_shape[1]" in ctx.L.crt_last_error(ctx.h)
        d_out = torch.full((3, H, W, 4), float(SENTINEL_F), dtype=torch.float32, device=dev())
        with pytest.raises(crt.CrtError) as e:
            ctx.render_shape_sets_device(to_dev(cams), c.bvhs, to_dev(pos_ok), d_out, 1, 1, T=to_dev(T_ok), view_shape=to_dev(bad_vs, np.int32))
        assert e.value.code == INVALID and "view_shape[1]" in str(e.value)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == SENTINEL_F).all() and (acc == SENTINEL_F).all() and (px == SENTINEL_U).all()
    ctx.clear(); ctx.render(1, 2, 1)                                         # a render afterwards equals the one before
    assert same(ctx.accumulator(), before)


# every row of the refusal table in its order, the outputs' sentinel intact
def test_refusals_leave_the_outputs_alone(rigs, crt, tmp_path):
    r = rigs("tlas3_two"); ctx = r.ctx; L = ctx.L
    c = r.case("tlas3_two")
    k, n = 3, c.T.shape[1]
    cams_h, T_h, pos_h = r.records(c.cameras), np.ascontiguousarray(c.T.reshape(3, -1, 16)), c.set_positions()
    tris = pos_h.shape[1]
    cams, T, pos = to_dev(cams_h), to_dev(T_h), to_dev(pos_h)
    out = torch.full((k * H * W * 4 + 4,), float(SENTINEL_F), dtype=torch.float32, device=dev())
    vs = to_dev([0, 1, 2], np.int32)
    host_out = np.zeros((k, H, W, 4), np.float32)
    boxes = np.full((3, 2, 2, 3), SENTINEL_F, np.float32)
    good = np.array(c.bvhs, np.uint32)

    def call(d_cams, d_pos, d_T, d_out, c_=ctx, kk=k, ids=good, M=None, S=3, nt=tris, blas=n, d_vs=None, frames=1, passes=1, stream=None):
        ids = None if ids is None else np.ascontiguousarray(ids, np.uint32)
        return L.crt_render_shape_sets_device(c_.h, C.c_void_p(d_cams), C.c_uint32(kk), None if ids is None else ids.ctypes.data_as(C.c_void_p),
                                              C.c_uint32((0 if ids is None else len(ids)) if M is None else M), C.c_void_p(d_pos), C.c_uint32(S), C.c_uint32(nt), C.c_void_p(d_T),
                                              C.c_uint32(blas), C.c_void_p(d_vs), C.c_uint32(1), C.c_uint32(frames), C.c_uint32(passes), C.c_float(1.0), C.c_void_p(d_out), None,
                                              boxes.ctypes.data_as(C.c_void_p), None, stream)
    err = lambda: L.crt_last_error(ctx.h)                                     # noqa: E731
    a, p, t, o = cams.data_ptr(), pos.data_ptr(), T.data_ptr(), out.data_ptr()
    # the order: each call breaks the named row AND every later one it can, and the named row answers
    assert call(a, p, t, o, ids=None, passes=9) == INVALID and b"bvhs is NULL" in err()                              # 4 before everything behind it
    assert call(a, p, t, o, ids=good, M=0, nt=0) == INVALID and b"no BVH" in err()
    assert call(a, p, t, o, ids=[0, n], nt=tris + 1, blas=n + 1) == INVALID and b"bvhs[1] = 3" in err()              # 5: out of range, named twice
    assert call(a, p, t, o, ids=[2, 0, 2], nt=tris + 1) == INVALID and b"bvhs[2] = 2 is named twice" in err()
    assert call(a, p, t, o, nt=tris - 1, blas=n + 1) == INVALID and b"triangles per shape" in err()                  # 6: setTris
    assert call(a, p, t, o, ids=[0], blas=n + 1) == INVALID and b"triangles per shape" in err()                      # (the count of another set)
    assert call(a, p, None, o, passes=0) == INVALID and b"T is NULL" in err()                                        # 7: T / blasCount
    assert call(a, p, t, o, blas=n + 1, passes=0) == INVALID and b"transforms per shape" in err()
    assert call(a, p, t, o, passes=0, kk=1 << 16, S=1 << 16, frames=1 << 16) == INVALID and call(a, p, t, o, passes=5) == INVALID       # passes
    assert call(a, p, t, o, kk=1 << 16, S=1 << 16, frames=1 << 16) == UNSUPPORTED                                    # more than 2^31-1 view-frames
    assert call(a, p, t, o, S=0) == INVALID and b"no shape" in err()         # no shape; view_shape NULL with S != K
    assert call(a, p, t, o, S=2) == INVALID
    assert call(a, p, t, o, kk=1, S=1 << 26, d_vs=vs.data_ptr()) == UNSUPPORTED and b"4 GiB" in err()
    assert call(a, p, t, o, S=2, d_vs=vs.data_ptr()) == INVALID              # an entry outside [0, S): the device entry's check
    assert b"view_shape[2]" in err()
    assert call(a, p, t, host_out.ctypes.data) == INVALID                    # host pointers
    assert call(cams_h.ctypes.data, p, t, o) == INVALID
    assert call(a, pos_h.ctypes.data, t, o) == INVALID
    assert call(a, p, T_h.ctypes.data, o) == INVALID
    assert call(a, p, t, o, d_vs=np.zeros(3, np.int32).ctypes.data) == INVALID
    assert call(a, p, t, o + 4) == INVALID and b"16-byte" in err()
    assert call(a, p + 2, t, o) == INVALID and call(a, p, t + 2, o) == INVALID                                       # misaligned
    assert call(None, p, t, o) == INVALID and call(a, None, t, o) == INVALID and call(a, p, t, None) == INVALID
    if torch.cuda.device_count() > 1:
        assert call(a, p, t, o, stream=C.c_void_p(torch.cuda.Stream(device=torch.device("cuda", 1)).cuda_stream)) == INVALID
    # K = 0 and frames = 0: no-ops after the checks that need no buffer
    assert call(None, None, t, None, kk=0, S=0) == 0 and call(None, None, t, None, frames=0) == 0 and call(None, None, t, None, kk=0, S=0, passes=9) == INVALID
    assert call(None, None, t, None, kk=0, S=0, ids=good, M=0, nt=0) == 0
    # the host entry's own: NULL buffers, view_shape looked at before anything runs
    acc = np.full((k, H, W, 4), SENTINEL_F, np.float32)
    assert raw_sets(ctx, cams_h, good, pos_h, T_h, np.array([0, 3, 1], np.int32), 1, 1, 1, 1.0, acc, None) == INVALID and b"view_shape[1] = 3" in err()
    assert raw_sets(ctx, cams_h, good, pos_h, T_h, None, 1, 1, 1, 1.0, None, None) == INVALID
    assert raw_sets(ctx, cams_h, None, pos_h, T_h, None, 1, 1, 1, 1.0, acc, None) == INVALID
    assert raw_sets(ctx, cams_h, good, pos_h, T_h, None, 1, 0, 1, 1.0, acc, None) == 0 and (acc == SENTINEL_F).all()
    # another accelerator selected
    hs = crt.HostScene(r.xml, 1, ASSETS); hs.build_alt(crt.ACCEL_KDTREE)
    kd = crt.Context(W, H); hs.upload(kd); hs.upload_alt(kd, crt.ACCEL_KDTREE); kd.set_render_accel(crt.ACCEL_KDTREE)
    assert call(a, p, t, o, c_=kd) == UNSUPPORTED
    assert call(a, p, t, o, c_=kd, S=0) == UNSUPPORTED                       # (... which comes before S / view_shape)
    assert (boxes == SENTINEL_F).all()
    kd.set_render_accel(0)
    assert call(a, p, t, o, c_=kd) == 0                                      # ... and with the BVH selected again the job runs
    torch.cuda.synchronize()
    one = ss.Case(c.scene, c.bvhs, c.factors, c.p0, c.T, c.cameras, None, 1, 1, 1)
    want = r.loop(one)
    assert same(out.cpu().numpy()[:k * H * W * 4].reshape(k, H, W, 4), want[0]) and all(same(boxes[s, m], b) for (s, m), b in want[2].items())
    out.fill_(float(SENTINEL_F)); boxes[:] = SENTINEL_F; torch.cuda.synchronize()
    kd.close()
    # 1: no scene; 3: a FileScene, whatever else is wrong; 2: a PrimitiveScene
    fresh = crt.Context(W, H)
    assert call(a, p, t, o, c_=fresh, ids=None) == STATE
    fresh.close()
    cube = crt.Context(W, H); crt.HostScene(si.scene_xml(tmp_path, "cube")[0], 0, ASSETS).upload(cube)
    assert call(a, p, t, o, c_=cube, ids=None) == INVALID and b"crt_render_shapes" in L.crt_last_error(cube.h)
    assert call(a, p, None, o, c_=cube, ids=[0], nt=12, blas=0) == INVALID and b"crt_render_shapes" in L.crt_last_error(cube.h)
    cube.close()
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(0.0)
    pc = crt.Context(W, H); ps.upload(pc)
    assert call(a, p, t, o, c_=pc, ids=None) == UNSUPPORTED
    pc.close()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL_F).all() and not host_out.any() and (acc == SENTINEL_F).all() and (boxes == SENTINEL_F).all()


def test_spare_tlas_nodes_a_tall_shape_and_a_failed_allocation_are_refused(crt, rigs):
    """the rows behind the pointers, as crt_render_shapes has them: a scene uploaded with spare TLAS nodes; 16 chain BLASes of height 40 whose second shape's transforms
    make a caterpillar (stack 40 + 15 + 1 = 56 dwords per lane, beyond the 49 the kernel's LDS leaves); staging of 512 GiB"""
    from test_gpu_render_shapes import chain_scene
    ctx, _, flat, _, pos = chain_scene(crt, 2, 3, extra_nodes=2)
    cams = crt.camera_records(W, H, [((0.0, 0.0, 0.0), (0.0, 0.0, 5.0))])
    acc = np.full((1, H, W, 4), SENTINEL_F, np.float32)
    both = np.ascontiguousarray(np.concatenate([pos, pos]).reshape(1, -1, 9))
    assert raw_sets(ctx, cams, [1, 0], both, np.ascontiguousarray(flat.reshape(1, 2, 16)), None, 1, 1, 1, 1.0, acc, None) == UNSUPPORTED
    assert b"TLAS nodes" in ctx.L.crt_last_error(ctx.h) and (acc == SENTINEL_F).all()
    ctx.close()
    N = 16
    ctx, boxes, flat, first, pos = chain_scene(crt, N, 41)
    line = np.stack([inp.rigid((4.0 ** i, 0.0, 5.0)) for i in range(N)])
    assert first["height"] == 5 and inp.restate(boxes, line)["height"] == 15
    cams = crt.camera_records(W, H, [((0.0, 0.0, 0.0), (0.0, 0.0, 5.0)), ((0.5, 0.0, 0.0), (0.0, 0.0, 5.0))])
    two = [np.stack([pos, pos * np.float32(1.25)]), np.stack([pos * np.float32(1.125), pos])]                         # BLAS 1 and BLAS 2 (chain BLASes share their triangles)
    ok = ctx.render_shape_sets(cams, [1, 2], two, 1, 1, T=np.stack([flat, flat]).reshape(2, N, 16))
    assert np.isfinite(ok).all()
    acc = np.full((2, H, W, 4), SENTINEL_F, np.float32); bx = np.full((2, 2, 2, 3), SENTINEL_F, np.float32)
    flat_pos = np.ascontiguousarray(np.concatenate([p.reshape(2, -1, 9) for p in two], axis=1))
    assert raw_sets(ctx, cams, [1, 2], flat_pos, np.ascontiguousarray(np.stack([flat, line]).reshape(2, N, 16)), None, 1, 1, 1, 1.0, acc, None, bx) == UNSUPPORTED
    msg = ctx.L.crt_last_error(ctx.h).decode()
    assert "shape 1" in msg and (acc == SENTINEL_F).all() and (bx == SENTINEL_F).all(), msg
    assert same(ctx.render_shape_sets(cams, [1, 2], two, 1, 1, T=np.stack([flat, flat]).reshape(2, N, 16)), ok)
    ctx.close()
    # the host entry's staging for 2^26 views of 32 x 16 pixels is 512 GiB, which hipMalloc refuses at once; one shape and a view_shape of zeros keep the table small
    r = rigs("tlas3_two"); c = r.case("tlas3_two")
    want = r.loop(c)[0]
    assert same(r.run(c), want)
    K = 1 << 26
    acc = np.full((1, H, W, 4), SENTINEL_F, np.float32); px = np.full((1, H, W), SENTINEL_U, np.uint32); bx = np.full((1, 2, 2, 3), SENTINEL_F, np.float32)
    assert raw_sets(r.ctx, r.records(c.cameras[:1]), c.bvhs, np.ascontiguousarray(c.set_positions()[:1]), np.ascontiguousarray(c.T[:1].reshape(1, -1, 16)), np.zeros(K, np.int32),
                    1, 1, 1, 1.0, acc, px, bx, K=K) == DEVICE
    assert "hipMalloc" in r.ctx.L.crt_last_error(r.ctx.h).decode()
    assert (acc == SENTINEL_F).all() and (px == SENTINEL_U).all() and (bx == SENTINEL_F).all()
    assert same(r.run(c), want)                                              # the context has dropped its staging and takes the next job as usual


# the rows the tiling truncates and the tiles the context does not own stay as the caller left them
@pytest.mark.parametrize("own", ["all", "strided"])
def test_ownership_and_truncation(crt, tmp_path, own):
    cfg = dict(tile_first=1, tile_stride=2, tile_count=3) if own == "strided" else {}
    r = Rig(crt, None, tmp_path, "tlas3", 48, 40, **cfg)
    c = r.case("tlas3_two")
    acc = np.full((3, 40, 48, 4), SENTINEL_F, np.float32); px = np.full((3, 40, 48), SENTINEL_U, np.uint32)
    assert raw_sets(r.ctx, r.records(c.cameras), c.bvhs, c.set_positions(), np.ascontiguousarray(c.T.reshape(3, -1, 16)), None, c.spp_first, c.frames, c.passes, 0.5, acc, px) == 0
    owned = np.zeros((40, 48), bool)
    for t in ([1, 3, 5] if own == "strided" else range(6)):
        owned[16 * (t // 3):16 * (t // 3) + 16, 16 * (t % 3):16 * (t % 3) + 16] = True
    want = r.loop(c)[0]
    for k in range(3):
        assert same(acc[k][owned], want[k][owned]), k
        assert (acc[k][~owned] == SENTINEL_F).all() and (px[k][~owned] == SENTINEL_U).all(), k
        assert (px[k][owned] != SENTINEL_U).all(), k
    r.close()
