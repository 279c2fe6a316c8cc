"""render_pool_kernel on scenes beyond its 16-bit node references: the same kernel instantiated for 32-bit pool references (layout.h), which a scene is uploaded
with when, and only when, it does not fit 16 bits.  Every case forces the pool (CRT_RENDER_KERNEL=pool_always, as tests/test_gpu_pool_kernel.py does), compares
bits with the oracle, and asserts that the launches really were the pool's (`pool_launches`): before the wide form such scenes went to render_tiles_kernel
without a word.

test_gpu_pool_kernel.py's test_scene_too_large_for_16_bit_references_falls_back still passes, but its name is history: the scene it forces out of the 16-bit
form (CRT_DEBUG_NO_REF16) is now uploaded in the 32-bit form and walks the wide pool kernel, with the same image.

The precondition — the test camera's primary rays do reach leaves on both sides of the 16-bit index — is tests/test_pool_wide_cpu.py's."""
import numpy as np
import pytest

from conftest import ASSETS, scene_path

torch = pytest.importorskip("torch")             # (before the library initialises HIP: the transforms and positions of test 5 are torch tensors)

pytestmark = pytest.mark.gpu

W, H = 96, 64
NEW = [("bunny4_scene.xml", 0), ("bunny14_scene.xml", 0), ("bunny4_tlas_scene.xml", 1)]
_oracle = {}


def oracle_render(orc, xml, kind, w, h, frames, passes=1):
    """(accumulator, counters) of the oracle's render, computed once per case and shared (read-only)"""
    key = (xml, kind, w, h, frames, passes)
    if key not in _oracle:
        o, _ = orc.load_scene(scene_path(xml), kind, ASSETS)
        o.renderer_init(w, h); o.set_params(5, passes); o.render(frames, 8)
        acc = o.accumulator(); acc.setflags(write=False)
        _oracle[key] = (acc, o.counters())
    return _oracle[key]


@pytest.fixture(autouse=True)
def pool_always(monkeypatch):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")


def render(crt, xml, kind, w, h, frames, passes=1, stats=False, launches=1):
    """one job on a fresh context; every render launch must have been the pool's.  Returns (accumulator, counters, context)"""
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    ctx = crt.Context(w, h, collect_stats=stats, max_frames_per_launch=4096)
    hs.upload(ctx)
    ctx.render(1, frames, passes)
    acc = ctx.accumulator()
    t = ctx.timing()
    assert t["render_launches"] == launches and t["pool_launches"] == launches, t
    return acc, ctx.counters(), ctx


# 1. each new scene against the oracle: a full 128-stream group + a 2-frame partial one (the refill tail), then S = 64 with two passes
@pytest.mark.parametrize("w,h,frames,passes", [(96, 64, 130, 1), (64, 48, 40, 2)])
@pytest.mark.parametrize("xml,kind", NEW)
def test_large_scenes_match_the_oracle(crt, orc, xml, kind, w, h, frames, passes):
    acc, cnt, ctx = render(crt, xml, kind, w, h, frames, passes)
    assert ctx.pool_lds(frames)[2] == 32
    want, wc = oracle_render(orc, xml, kind, w, h, frames, passes)
    assert np.array_equal(acc, want)
    assert cnt["rays"] == wc["rays"]


# 2. the statistics build
@pytest.mark.parametrize("xml,kind", [("bunny4_scene.xml", 0), ("bunny4_tlas_scene.xml", 1)])
def test_statistics_build_counts_what_the_oracle_counts(crt, orc, xml, kind):
    acc, cnt, _ = render(crt, xml, kind, 64, 48, 70, stats=True)
    want, wc = oracle_render(orc, xml, kind, 64, 48, 70)
    assert np.array_equal(acc, want)
    assert cnt == wc
    for k in ("interior_iters", "leaf_iters", "tri_tests", "mesh_hits") + (("tlas_iters", "blas_visits") if kind else ()):
        assert cnt[k] > 0, k


# 4. the shipped scenes forced into the wide form
@pytest.mark.parametrize("xml,kind,no_rootpair", [("bunny_scene.xml", 0, False), ("tlas_scene.xml", 1, False), ("cube_scene.xml", 0, False), ("cube_scene.xml", 0, True)])
def test_shipped_scenes_in_the_wide_form_render_the_same_bits(crt, orc, monkeypatch, xml, kind, no_rootpair):
    if no_rootpair:
        monkeypatch.setenv("CRT_DEBUG_NO_ROOTPAIR", "1")                     # every ray starts at Scene::rootRef16 instead of the root's child pair
    narrow, nc, ctx = render(crt, xml, kind, W, H, 130)
    assert ctx.pool_lds(130)[2] == 16
    monkeypatch.setenv("CRT_DEBUG_NO_REF16", "1")
    wide, wcnt, ctx = render(crt, xml, kind, W, H, 130)
    assert ctx.pool_lds(130)[2] == 32
    want, wc = oracle_render(orc, xml, kind, W, H, 130)
    assert np.array_equal(wide, narrow) and np.array_equal(wide, want)
    assert wcnt["rays"] == nc["rays"] == wc["rays"]


# 5. the four scene writes leave a wide scene wide
def test_scene_writes_keep_the_wide_form(crt, orc):
    from test_gpu_scene_update import rigid
    from test_oracle_pinning import deform
    xml, frames = "bunny4_tlas_scene.xml", 130
    dev = torch.device("cuda", 0)
    hs = crt.HostScene(scene_path(xml), 1, ASSETS)
    o, _ = orc.load_scene(scene_path(xml), 1, ASSETS); o.renderer_init(W, H)
    ctx = crt.Context(W, H, max_frames_per_launch=4096); hs.upload(ctx)
    n = hs.bvh_count()
    T = np.stack([hs.blas_transform(i)[0].reshape(4, 4) for i in range(n)]).astype(np.float32)

    def check(what):
        ctx.clear(); ctx.reset_counters(); o.clear(); o.reset_counters()
        ctx.render(1, frames, 1); o.render(frames, 8)
        assert np.array_equal(ctx.accumulator(), o.accumulator()), what
        assert ctx.counters()["rays"] == o.counters()["rays"], what
        t = ctx.timing()                                                     # (launches since the last call)
        assert t["render_launches"] == 1 and t["pool_launches"] == 1, (what, t)
        assert ctx.pool_lds(frames)[2] == 32, what

    check("as uploaded")
    # a host set_transform + update(CRT_UPDATE_TRANSFORMS): the TLAS flattened on the host
    T[1] = rigid(0.5, T[1][:3, 3] + np.array([0.2, 0.1, -0.3], np.float32))
    hs.set_transform(1, T[1]); o.set_transform(1, T[1])
    hs.update(ctx, crt.UPDATE_TRANSFORMS)
    check("set_transform + UPDATE_TRANSFORMS")
    # every transform from a tensor, the TLAS built on the device
    for i in range(n):
        T[i] = rigid(0.3 * (i + 1), T[i][:3, 3] + np.array([0.05 * i, 0.0, 0.1 * i], np.float32))
        o.set_transform(i, T[i])
    hs.set_transforms_device(ctx, torch.from_numpy(T.copy()).to(dev))
    check("update_transforms_device")
    # a refit of one BLAS on the device, then the TLAS on the device
    t = hs.bvh(2)["tris"]
    p0 = np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1).astype(np.float32)
    moved = deform(p0)
    ctx.refit_device(2, torch.from_numpy(moved).to(dev), root_box=False)
    ctx.update_transforms_device(torch.from_numpy(T.copy()).to(dev))
    o.move_and_refit(2, moved)
    check("refit_device + update_transforms_device")
    # a host refit + update(CRT_UPDATE_BOUNDS)
    moved2 = (p0 * np.float32(1.05) + np.float32(0.01)).astype(np.float32)
    hs.move_and_refit(2, moved2); o.move_and_refit(2, moved2)
    hs.update(ctx, crt.UPDATE_BOUNDS)
    check("move_and_refit + UPDATE_BOUNDS")


# 6. a split job: the expensive tiles through render_tiles_kernel's block table, the rest through the wide pool
def test_split_job_on_a_large_scene_matches_the_oracle(crt, orc, monkeypatch):
    monkeypatch.setenv("CRT_PLAN_NO_TRIAL", "1"); monkeypatch.setenv("CRT_SPLIT_FORCE", "5")
    xml, frames = "bunny4_scene.xml", 200
    want, wc = oracle_render(orc, xml, 0, W, H, frames)
    hs = crt.HostScene(scene_path(xml), 0, ASSETS)
    ctx = crt.Context(W, H); hs.upload(ctx)
    splits = []
    for i in range(3):
        ctx.clear(); ctx.reset_counters(); ctx.render(1, frames, 1); ctx.sync()
        assert np.array_equal(ctx.accumulator(), want), i
        assert ctx.counters()["rays"] == wc["rays"]
        t = ctx.timing()
        assert t["pool_launches"] == t["render_launches"] == 1, t            # (since the last call)
        splits.append(t["split_launches"])
    assert splits[0] == 0 and splits[-1] == 1, splits                       # the first job measures, later ones split


# 7. long wavefronts that refill their slots, with and without the tile classes
def test_refill_and_tile_classes_on_a_large_scene(crt, orc, monkeypatch):
    monkeypatch.setenv("CRT_POOL_WAVE_FRAMES", "256")
    xml, frames = "bunny4_scene.xml", 300
    want, wc = oracle_render(orc, xml, 0, W, H, frames)
    a, ca, ctx = render(crt, xml, 0, W, H, frames)
    assert ctx.tile_classes().any()                                          # the sky tiles above the bunnies are classified
    monkeypatch.setenv("CRT_DEBUG_NO_TILE_CLASS", "1")
    b, cb, _ = render(crt, xml, 0, W, H, frames)
    assert np.array_equal(a, want) and np.array_equal(a, b)
    assert ca["rays"] == cb["rays"] == wc["rays"]


# 8. the stack bound
def test_wide_stacks_stay_within_a_workgroups_lds_or_the_tiles_kernel_renders(crt, orc, monkeypatch):
    xml, frames = "bunny14_scene.xml", 130
    pool, pc, ctx = render(crt, xml, 0, W, H, frames)
    need, limit, bits = ctx.pool_lds(frames)
    assert bits == 32 and 0 < need <= limit <= 160 * 1024, (need, limit)
    depth = crt.HostScene(scene_path(xml), 0, ASSETS).bvh(0)["maxDepth"]
    assert need >= (depth + 1) * 64 * 4 + 14 * 128 * 4                       # 4-byte entries for the tree's height + the parked streams
    assert ctx.pool_lds(64)[0] < need                                        # 64 slots park half as much
    # a scene whose wavefront would not fit: no failed launch, render_tiles_kernel renders it, same bits
    extra = (limit - need + 256) // 256 * 256
    monkeypatch.setenv("CRT_DEBUG_EXTRA_LDS", str(extra))
    hs = crt.HostScene(scene_path(xml), 0, ASSETS)
    c2 = crt.Context(W, H, max_frames_per_launch=4096); hs.upload(c2)
    assert c2.pool_lds(frames)[0] > limit
    c2.render(1, frames, 1)
    t = c2.timing()
    assert t["render_launches"] == 1 and t["pool_launches"] == 0, t
    assert np.array_equal(c2.accumulator(), pool) and c2.counters()["rays"] == pc["rays"]
    want, wc = oracle_render(orc, xml, 0, W, H, frames)
    assert np.array_equal(pool, want) and pc["rays"] == wc["rays"]


# 9. the default routing follows the measurement (profiles/pool_wide.json): the wide pool did not beat one stream per lane at any job size
def test_large_job_of_a_wide_scene_is_the_tiles_kernels_by_default(crt, monkeypatch):
    """1280x720 x 20 windows = 72 000 (tile, window) pairs — a job size at which a 16-bit scene gets the pool (test_gpu_pool_kernel.py): a scene in the 32-bit form
    gets render_tiles_kernel unless the pool is forced; same bits both ways"""
    hs = crt.HostScene(scene_path("bunny14_scene.xml"), 0, ASSETS)
    out = {}
    for k in ("default", "pool_always"):
        if k == "default": monkeypatch.delenv("CRT_RENDER_KERNEL")
        else: monkeypatch.setenv("CRT_RENDER_KERNEL", k)
        ctx = crt.Context(1280, 720); hs.upload(ctx); ctx.render(1, 20 * 64, 1)
        out[k] = (ctx.accumulator(), ctx.counters()["rays"], ctx.timing()); ctx.close()
    assert out["default"][2]["render_launches"] == 1 and out["default"][2]["pool_launches"] == 0, out["default"][2]
    assert out["pool_always"][2]["render_launches"] == 1 and out["pool_always"][2]["pool_launches"] == 1, out["pool_always"][2]
    assert np.array_equal(out["default"][0], out["pool_always"][0]) and out["default"][1] == out["pool_always"][1]
