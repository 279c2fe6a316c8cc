"""render_pool_kernel at the last index of its 16-bit node references (layout.h): the scenes of tests/ref16_limit_inputs.py, which fill the form — 16 382
triangles, references with bit 13 set in half of the leaves and in the upper node pairs, the last leaf slot (reference 0x3ffe), a leaf of 64 triangles above slot
8 192, three BLASes whose records start above one another's, a description with 16 381 node pairs — and the scenes of one triangle more, which must be uploaded in
the 32-bit form.  Every render is forced onto the pool (CRT_RENDER_KERNEL=pool_always, as tests/test_gpu_pool_wide.py does), compared bit for bit with the oracle's
accumulator and ray count, and asserted to have been the pool's launch in the form the case expects.  No tolerances, no timing.

What the cases assume of the scenes — that the camera's rays do reach those slots and pairs — is tests/test_ref16_limit_cpu.py's."""
import numpy as np
import pytest

import bvh_build_inputs as B
import ref16_limit_inputs as I
import stack_fill as S
from conftest import ASSETS

torch = pytest.importorskip("torch")             # (before the library initialises HIP: the transforms and positions of the scene-write test are torch tensors)

import test_gpu_grid_device as TG                                          # noqa: E402  (helpers only; a module object is not collected)

pytestmark = pytest.mark.gpu

W, H = I.W, I.H
DEFAULT = None                                   # the camera a renderer starts with
STAT_KEYS = ("interior_iters", "leaf_iters", "tri_tests", "mesh_hits")


@pytest.fixture(autouse=True)
def pool_always(monkeypatch):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")


@pytest.fixture(scope="module")
def world(crt, orc, tmp_path_factory):
    """the meshes, their host builds, the two-level scene files and the oracle's renders, each made once and shared read-only"""
    tmp = tmp_path_factory.mktemp("ref16_limit"); memo = {}

    class Wd:
        def mesh(self, name):
            if ("mesh", name) not in memo:
                p = {"narrow": lambda: I.file_mesh(I.T_NARROW), "wide": lambda: I.file_mesh(I.T_WIDE), "big_leaf": I.big_leaf_mesh}[name]()
                p.setflags(write=False)
                memo["mesh", name] = (p, crt.host_bvh_build(p))
            return memo["mesh", name]

        def xml(self, total):
            if ("xml", total) not in memo:
                memo["xml", total] = I.write_two_level(tmp, total)
            return memo["xml", total]

        def second_camera(self):
            p, t = self.mesh("narrow")
            return I.close_camera(p, int(t["indices"][-1]))                  # the triangle in the last leaf slot

        def oracle(self, scene):
            """a fresh oracle of a FileScene mesh name or a two-level total"""
            if isinstance(scene, str):
                return S.mesh_oracle(orc, self.mesh(scene)[0])
            return orc.load_scene(self.xml(scene), 1, ASSETS)[0]

        def want(self, scene, camera, w, h, frames, passes=1):
            """(accumulator, counters) of the oracle's render"""
            key = ("render", scene, camera, w, h, frames, passes)
            if key not in memo:
                o = self.oracle(scene)
                o.renderer_init(w, h); o.set_params(5, passes)
                if camera is not None:
                    o.set_camera_state(*camera)
                o.render(frames, 8)
                acc = o.accumulator(); acc.setflags(write=False)
                memo[key] = (acc, o.counters())
            return memo[key]
    return Wd()


def file_context(crt, p, tree, w, h, stats=False):
    ctx = crt.Context(w, h, collect_stats=stats, max_frames_per_launch=4096)
    TG.upload_described(crt, ctx, I.described(crt, p, tree))
    return ctx


def two_level_context(crt, xml, w, h, stats=False):
    hs = crt.HostScene(xml, 1, ASSETS)
    ctx = crt.Context(w, h, collect_stats=stats, max_frames_per_launch=4096)
    hs.upload(ctx)
    return ctx, hs


def pool_render(ctx, frames, passes, bits, camera=None, what=""):
    """one job; every render launch must have been the pool's, on a scene in the `bits`-bit form.  Returns (accumulator, counters)."""
    assert ctx.pool_lds(frames)[2] == bits, (what, ctx.pool_lds(frames))
    if camera is not None:
        ctx.set_camera_state(*camera)
    ctx.render(1, frames, passes)
    acc = ctx.accumulator()
    t = ctx.timing()
    assert t["render_launches"] >= 1 and t["pool_launches"] == t["render_launches"], (what, t)
    return acc, ctx.counters()


def assert_equals_oracle(got, want, what, stats=False, keys=STAT_KEYS):
    (acc, cnt), (wacc, wcnt) = got, want
    if not np.array_equal(acc, wacc):
        bad = np.argwhere((acc != wacc).any(axis=-1))
        raise AssertionError((what, "accumulator differs in %d pixels" % len(bad), bad[:8].tolist()))
    assert cnt["rays"] == wcnt["rays"], (what, cnt["rays"], wcnt["rays"])
    if stats:
        assert cnt == wcnt, (what, cnt, wcnt)
        for k in keys:
            assert cnt[k] > 0, (what, k)


# 1. the largest narrow scene, with both cameras
@pytest.mark.parametrize("camera", ["default", "second"])
@pytest.mark.parametrize("w,h,frames,passes", I.SHAPES)
def test_narrow_limit_matches_the_oracle(crt, world, w, h, frames, passes, camera):
    p, tree = world.mesh("narrow")
    cam = world.second_camera() if camera == "second" else DEFAULT
    ctx = file_context(crt, p, tree, w, h)
    assert_equals_oracle(pool_render(ctx, frames, passes, 16, cam), world.want("narrow", cam, w, h, frames, passes), camera)


@pytest.mark.parametrize("camera", ["default", "second"])
def test_narrow_limit_statistics_build_counts_what_the_oracle_counts(crt, world, camera):
    p, tree = world.mesh("narrow")
    cam = world.second_camera() if camera == "second" else DEFAULT
    ctx = file_context(crt, p, tree, W, H, stats=True)
    assert_equals_oracle(pool_render(ctx, 130, 1, 16, cam), world.want("narrow", cam, W, H, 130), camera, stats=True)


# 2. one triangle more: the 32-bit form, and the form changes exactly between the two sizes
@pytest.mark.parametrize("w,h,frames,passes", I.SHAPES)
def test_one_triangle_more_is_wide_and_matches_the_oracle(crt, world, w, h, frames, passes):
    assert I.T_WIDE == I.T_NARROW + 1
    p, tree = world.mesh("narrow")
    assert len(p) == I.T_NARROW and file_context(crt, p, tree, w, h).pool_lds(frames)[2] == 16
    p, tree = world.mesh("wide")
    assert len(p) == I.T_WIDE
    ctx = file_context(crt, p, tree, w, h)
    assert_equals_oracle(pool_render(ctx, frames, passes, 32), world.want("wide", DEFAULT, w, h, frames, passes), "wide")


# 3. the narrow scene forced into the wide form: the same bits
def test_narrow_scene_forced_wide_renders_the_same_bits(crt, world, monkeypatch):
    p, tree = world.mesh("narrow")
    narrow = pool_render(file_context(crt, p, tree, W, H), 130, 1, 16)
    monkeypatch.setenv("CRT_DEBUG_NO_REF16", "1")
    wide = pool_render(file_context(crt, p, tree, W, H), 130, 1, 32)
    want = world.want("narrow", DEFAULT, W, H, 130)
    assert_equals_oracle(narrow, want, "narrow"); assert_equals_oracle(wide, want, "forced wide")
    assert np.array_equal(narrow[0], wide[0]) and narrow[1]["rays"] == wide[1]["rays"]


# 4. no root pair: every ray starts from Scene::rootRef16
@pytest.mark.parametrize("camera", ["default", "second"])
def test_narrow_limit_without_the_root_pair(crt, world, monkeypatch, camera):
    monkeypatch.setenv("CRT_DEBUG_NO_ROOTPAIR", "1")
    p, tree = world.mesh("narrow")
    cam = world.second_camera() if camera == "second" else DEFAULT
    assert_equals_oracle(pool_render(file_context(crt, p, tree, W, H), 130, 1, 16, cam), world.want("narrow", cam, W, H, 130), camera)


# 5. a leaf of 64 triangles above slot 8 192: `cur + 1` and `remain` at high slots; tied hits go to the leaf's first slot in both
@pytest.mark.parametrize("w,h,frames,passes", I.SHAPES)
def test_big_leaf_matches_the_oracle(crt, world, w, h, frames, passes):
    p, tree = world.mesh("big_leaf")
    assert tree["nodes"]["triCount"].max() == I.BIG_LEAF
    assert_equals_oracle(pool_render(file_context(crt, p, tree, w, h), frames, passes, 16), world.want("big_leaf", DEFAULT, w, h, frames, passes), "big leaf")


def test_big_leaf_statistics_build_tests_as_many_triangles(crt, world):
    p, tree = world.mesh("big_leaf")
    got = pool_render(file_context(crt, p, tree, W, H, stats=True), 130, 1, 16)
    want = world.want("big_leaf", DEFAULT, W, H, 130)
    assert got[1]["tri_tests"] == want[1]["tri_tests"]
    assert_equals_oracle(got, want, "big leaf", stats=True)


# 6. the two-level scenes of both totals
@pytest.mark.parametrize("w,h,frames,passes", I.SHAPES)
@pytest.mark.parametrize("total,bits", [(I.T_NARROW, 16), (I.T_WIDE, 32)])
def test_two_level_totals_match_the_oracle(crt, world, total, bits, w, h, frames, passes):
    ctx, hs = two_level_context(crt, world.xml(total), w, h)
    assert hs.triangle_count() == total
    assert_equals_oracle(pool_render(ctx, frames, passes, bits), world.want(total, DEFAULT, w, h, frames, passes), total)


@pytest.mark.parametrize("total,bits", [(I.T_NARROW, 16), (I.T_WIDE, 32)])
def test_two_level_statistics_build_counts_what_the_oracle_counts(crt, world, total, bits):
    ctx, _ = two_level_context(crt, world.xml(total), W, H, stats=True)
    assert_equals_oracle(pool_render(ctx, 130, 1, bits), world.want(total, DEFAULT, W, H, 130), total, stats=True, keys=STAT_KEYS + ("tlas_iters", "blas_visits"))


# 7. the scene writes at the limit: every one leaves the narrow two-level scene narrow and right
def test_scene_writes_at_the_limit_keep_the_narrow_form(crt, orc, world, tmp_path):
    from test_gpu_bvh_device import as_bvh
    from test_gpu_scene_update import rigid
    from test_oracle_pinning import deform
    frames = 130
    dev = torch.device("cuda", 0)
    xml = world.xml(I.T_NARROW)
    ctx, hs = two_level_context(crt, xml, W, H)
    n = hs.bvh_count()
    T = np.stack([hs.blas_transform(i)[0].reshape(4, 4) for i in range(n)]).astype(np.float32)
    state = dict(o=orc.load_scene(xml, 1, ASSETS)[0])
    state["o"].renderer_init(W, H)

    def check(what):
        o = state["o"]
        ctx.clear(); ctx.reset_counters(); o.clear(); o.reset_counters()
        ctx.timing()                                                         # (launches since the last call)
        got = pool_render(ctx, frames, 1, 16, what=what)
        o.render(frames, 8)
        assert_equals_oracle(got, (o.accumulator(), o.counters()), what)

    check("as uploaded")
    # a host set_transform + update(CRT_UPDATE_TRANSFORMS): the TLAS flattened on the host
    T[1] = rigid(0.5, T[1][:3, 3] + np.array([0.05, 0.1, -0.3], np.float32))
    hs.set_transform(1, T[1]); state["o"].set_transform(1, T[1])
    hs.update(ctx, crt.UPDATE_TRANSFORMS)
    check("set_transform + UPDATE_TRANSFORMS")
    # every transform from a tensor, the TLAS built on the device
    for i in range(n):
        T[i] = rigid(0.2 * (i + 1), T[i][:3, 3] + np.array([0.02 * i, 0.0, 0.1 * i], np.float32))
        state["o"].set_transform(i, T[i])
    hs.set_transforms_device(ctx, torch.from_numpy(T.copy()).to(dev))
    check("update_transforms_device")
    # a refit of BLAS 2 (global slots 10 000 .. 16 381) on the device, then the TLAS on the device
    p2 = I.piece(2, I.piece_sizes(I.T_NARROW)[2])
    moved = deform(p2)
    ctx.refit_device(2, torch.from_numpy(moved).to(dev), root_box=False)
    ctx.update_transforms_device(torch.from_numpy(T.copy()).to(dev))
    state["o"].move_and_refit(2, moved)
    check("refit_device + update_transforms_device")
    # a host refit + update(CRT_UPDATE_BOUNDS)
    moved2 = (p2 * np.float32(1.05) + np.float32(0.01)).astype(np.float32)
    hs.move_and_refit(2, moved2); state["o"].move_and_refit(2, moved2)
    hs.update(ctx, crt.UPDATE_BOUNDS)
    check("move_and_refit + UPDATE_BOUNDS")
    # BLAS 0 rebuilt on the device, twice: over wobbled triangles, whose tree has more or fewer pairs, and over its own again, which undoes that.  Either way the
    # later BLASes' pairs — references round and above index 8 192 — are rebased by a nonzero pairDelta, of either sign.  The oracle has no rebuild: it loads the
    # scene with those triangles in BLAS 0 and is taken through the writes above; so is a second host scene, whose fresh upload the live scene must equal.
    own = I.piece(0, I.PIECE_TRIS)
    pairs = [hs.bvh(0)["nodesUsed"] // 2]
    for step, (pos, tag) in enumerate([(I.wobbled_piece0(), "_wobbled"), (own, "")]):
        what = "build_bvh_device of BLAS 0, step %d" % step
        built = crt.host_bvh_build(pos)
        pairs.append(built["nodesUsed"] // 2)
        assert pairs[-1] != pairs[-2], pairs                                 # the pair count changes: a nonzero pairDelta
        ctx.build_bvh_device(0, torch.from_numpy(pos).to(dev))
        ctx.update_transforms_device(torch.from_numpy(T.copy()).to(dev))
        xml2 = I.write_two_level(tmp_path, I.T_NARROW, piece0=pos, tag=tag + "_step%d" % step)
        o2 = orc.load_scene(xml2, 1, ASSETS)[0]; o2.renderer_init(W, H)
        h2 = crt.HostScene(xml2, 1, ASSETS)
        for s in (o2, h2):
            for i in range(n):
                s.set_transform(i, T[i])
            s.move_and_refit(2, moved); s.move_and_refit(2, moved2)
        assert I.positions(o2.bvh(0)).tobytes() == pos.tobytes()
        B.assert_bvh_equal(as_bvh(h2.bvh(0)), built, what)
        state["o"] = o2
        check(what)
        c2 = crt.Context(W, H, max_frames_per_launch=4096); h2.upload(c2)
        for i in range(n):
            B.assert_bvh_equal(ctx.get_bvh(i), c2.get_bvh(i), "%s: BLAS %d" % (what, i))
        B.assert_bvh_equal(ctx.get_bvh(0), built, what)
        assert S.scene_words(ctx).tolist() == S.scene_words(c2).tolist(), what
        c2.close()
    assert (pairs[1] - pairs[0]) * (pairs[2] - pairs[1]) < 0, pairs         # one rebuild grew the count, the other shrank it


# 8. the last pair index: a description with T - 1 node pairs
@pytest.mark.parametrize("camera", ["default", "second"])
def test_releafed_description_reaches_the_last_pair_index(crt, world, monkeypatch, camera):
    p, tree = world.mesh("narrow")
    r = I.releaf(tree, p)
    assert r["nodesUsed"] // 2 == I.T_NARROW - 1
    cam = world.second_camera() if camera == "second" else DEFAULT
    want = world.want("narrow", cam, W, H, 130)                              # the built tree's render: the nearest hit does not depend on the tree
    ctx = file_context(crt, p, r, W, H)
    assert S.allotted(ctx)["bvh"] == r["height"] == tree["height"] + 1      # one more stack level than the built tree, and the library allots it
    pool = pool_render(ctx, 130, 1, 16, cam)
    monkeypatch.delenv("CRT_RENDER_KERNEL")                                 # the default kernel for a job this small: render_tiles_kernel, which reads only the offset form
    c2 = file_context(crt, p, r, W, H)
    if cam is not None:
        c2.set_camera_state(*cam)
    c2.render(1, 130, 1)
    t = c2.timing()
    assert t["render_launches"] >= 1 and t["pool_launches"] == 0, t
    tiles = (c2.accumulator(), c2.counters())
    # both differ from the oracle in the same pixels: an exact tie in t between two triangles of a former leaf (another seed); the pool alone: a reference bug
    assert_equals_oracle(tiles, want, "render_tiles_kernel")
    assert_equals_oracle(pool, want, "render_pool_kernel")
    assert np.array_equal(pool[0], tiles[0]) and pool[1]["rays"] == tiles[1]["rays"]
