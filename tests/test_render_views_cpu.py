"""crt_render_views without a GPU: the two entries are exported, declared and bound, and the oracle side of tests/test_gpu_render_views.py is what that test
assumes — every test camera sees the mesh, and no two views of a case are alike, so a view-frame summed into the wrong view cannot pass by coincidence."""
import inspect
import os

import numpy as np
import pytest

import render_views_inputs as vi
from conftest import ASSETS, REPO, scene_path


def test_symbols_are_exported_declared_and_bound(crt):
    L = crt.lib()
    header = open(os.path.join(REPO, "include", "crt_abi.h")).read()
    for name in ("crt_render_views", "crt_render_views_device"):
        assert name in crt.ABI_SYMBOLS
        assert hasattr(L, name), name
        assert ("int  %s(crt_ctx* ctx, const float* " % name) in header, name
    assert "#define CRT_ABI_VERSION 3" in header and L.crt_abi_version() == 3
    host = inspect.signature(crt.Context.render_views)
    assert list(host.parameters) == ["self", "cameras", "spp_first", "frames", "passes", "scale"]
    dev = inspect.signature(crt.Context.render_views_device)
    assert list(dev.parameters) == ["self", "cams", "out", "spp_first", "frames", "passes", "scale", "pixels", "stream"]


def test_camera_records_are_set_camera_states_arguments(crt, orc):
    """the helper's records are the oracle's Camera for the same (position, target), bit for bit"""
    pairs = vi.ring(5) + vi.prim_cameras(2)
    rec = crt.camera_records(vi.W, vi.H, pairs)
    assert rec.shape == (7, 12) and rec.dtype == np.float32
    o = vi.make_oracle(orc, ASSETS, scene_path, "bvh")
    for k, pair in enumerate(pairs):
        o.set_camera_state(*pair)
        assert np.array_equal(np.concatenate(o.camera()).view(np.uint32), rec[k].view(np.uint32)), k


def views_of(o, cameras, spp_first, frames, passes):
    return [vi.oracle_view(o, cam, spp_first, frames, passes) for cam in cameras]


def assert_all_distinct(accs, what):
    seen = {}
    for k, a in enumerate(accs):
        key = a.tobytes()
        assert key not in seen, (what, "views", seen[key], k, "are equal")
        seen[key] = k


@pytest.fixture(scope="module")
def cube(orc):
    return vi.make_oracle(orc, ASSETS, scene_path, "bvh")


@pytest.mark.parametrize("case", ["start_and_passes", "straddle_3", "straddle_70"])
def test_case_cameras_see_the_mesh_and_differ(cube, case):
    cameras, spp_first, frames, passes = vi.CASES[case]
    views = views_of(cube, cameras, spp_first, frames, passes)
    for k, (acc, cnt) in enumerate(views):
        assert cnt["mesh_hits"] > 0 and cnt["primary"] == 2 * 256 * frames * passes, (case, k, cnt)
        assert np.isfinite(acc).all() and (acc[..., :3] > 0).any(), (case, k)
    assert_all_distinct([v[0] for v in views], case)
    if case == "straddle_3":                                             # the views that straddle a window boundary, against their neighbours
        for k in (21, 42):
            for n in (k - 1, k + 1):
                if n < len(views):
                    assert not np.array_equal(views[k][0], views[n][0]), (k, n)


def test_one_frame_cameras_see_the_mesh_and_differ(cube):
    """the 130 cameras of the frames = 1 cases (lanes_64 and lanes_65 are prefixes of the same ring)"""
    cameras, spp_first, frames, passes = vi.CASES["lanes_130"]
    assert vi.CASES["lanes_64"][0] == cameras[:64] and vi.CASES["lanes_65"][0] == cameras[:65]
    views = views_of(cube, cameras, spp_first, frames, passes)
    assert all(cnt["mesh_hits"] > 0 for _, cnt in views)
    assert_all_distinct([v[0] for v in views], "lanes_130")


@pytest.mark.parametrize("world", vi.WORLDS)
def test_world_cameras_see_the_mesh_and_differ(orc, world):
    o = vi.make_oracle(orc, ASSETS, scene_path, world)
    views = views_of(o, vi.world_cameras(world), *vi.WORLD_SHAPE)
    for k, (acc, cnt) in enumerate(views):
        assert np.isfinite(acc).all() and (acc[..., :3] > 0).any(), (world, k)
        if world != "prim":                                              # (the PrimitiveScene has no meshes to count)
            assert cnt["mesh_hits"] > 0, (world, k, cnt)
    assert_all_distinct([v[0] for v in views], world)
