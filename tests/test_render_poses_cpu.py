"""crt_render_poses without a GPU: the two entries are exported, declared and bound, and the oracle side of tests/test_gpu_render_poses.py is what that test
assumes — every test camera sees at least one instance in every pose it is paired with, and no two views of a case are alike, so a view rendered with the wrong
pose or the wrong camera cannot pass by coincidence; and the two poses of the mixed-height case build TLASes of different heights."""
import inspect
import os

import numpy as np
import pytest

import render_poses_inputs as pi
import tlas_device_inputs as inp
from conftest import ASSETS, REPO


def test_symbols_are_exported_declared_and_bound(crt):
    L = crt.lib()
    header = open(os.path.join(REPO, "include", "crt_abi.h")).read()
    for name in ("crt_render_poses", "crt_render_poses_device"):
        assert name in crt.ABI_SYMBOLS
        assert hasattr(L, name), name
        assert ("int  %s(crt_ctx* ctx, const float* " % name) in header, name
    assert "#define CRT_ABI_VERSION 3" in header and L.crt_abi_version() == 3
    host = inspect.signature(crt.Context.render_poses)
    assert list(host.parameters) == ["self", "cameras", "T", "spp_first", "frames", "passes", "scale", "view_pose", "want_tlas"]
    dev = inspect.signature(crt.Context.render_poses_device)
    assert list(dev.parameters)[:6] == ["self", "cams", "T", "out", "spp_first", "frames"]


def assert_all_distinct(accs, what):
    seen = {}
    for k, a in accs:
        key = a.tobytes()
        assert key not in seen, (what, "views", seen[key], k, "are equal")
        seen[key] = k


@pytest.mark.parametrize("name", pi.ALL_RENDERED + ("bad_pose",))
def test_case_cameras_see_an_instance_and_views_differ(orc, tmp_path, name):
    if name in ("lanes_64", "lanes_65"):                                  # prefixes of lanes_130's poses and cameras: checked there
        big, c = pi.case("lanes_130"), pi.case(name)
        n = len(c.cameras)
        assert c.cameras == big.cameras[:n] and np.array_equal(c.T, big.T[:n]) and (c.spp_first, c.frames, c.passes) == (big.spp_first, big.frames, big.passes)
        return
    c = pi.case(name)
    o = pi.make_oracle(orc, ASSETS, inp.scene_xml(tmp_path, c.scene))
    views = []
    for k in pi.good_views(c):
        acc, cnt = pi.oracle_view(o, c, k)
        assert cnt["mesh_hits"] > 0 and cnt["primary"] == 2 * 256 * c.frames * c.passes, (name, k, cnt)
        assert np.isfinite(acc).all() and (acc[..., :3] > 0).any(), (name, k)
        views.append((k, acc))
    assert len(views) >= 2
    assert_all_distinct(views, name)
    # every pose of the case is a different set of transforms, and (no view_pose) every camera a different one
    assert len({c.T[p].tobytes() for p in range(len(c.T))}) == len(c.T)
    assert len(set(c.cameras)) == len(c.cameras)


def test_a_view_with_the_wrong_pose_differs(orc, tmp_path):
    """loop_5_of_2: views 0 and 1 under each other's pose are not what the case expects of them"""
    c = pi.case("loop_5_of_2")
    o = pi.make_oracle(orc, ASSETS, inp.scene_xml(tmp_path, c.scene))
    right = [pi.oracle_view(o, c, k)[0] for k in (0, 1)]
    swapped = pi.Case(c.scene, c.T, c.cameras, [1 - p for p in c.view_pose], c.spp_first, c.frames, c.passes)
    for k in (0, 1):
        assert not np.array_equal(pi.oracle_view(o, swapped, k)[0], right[k]), k


def test_mixed_heights_premise(crt, tmp_path):
    """the ring pose and the line pose of the forty instances build TLASes of different heights (restate: the build as the kernel does it)"""
    c = pi.case("mixed_heights")
    hs = crt.HostScene(inp.scene_xml(tmp_path, c.scene), 1, ASSETS)
    boxes = np.stack([np.stack([hs.bvh(i)["nodes"][0]["aabbMin"], hs.bvh(i)["nodes"][0]["aabbMax"]]) for i in range(hs.bvh_count())])
    h = [inp.restate(boxes, c.T[p])["height"] for p in (0, 1)]
    assert h[0] != h[1] and max(h) >= 2 * min(h), h


def test_rand256_reaches_the_stale_a_quirk(crt, tmp_path):
    c = pi.case("rand256")
    hs = crt.HostScene(inp.scene_xml(tmp_path, c.scene), 1, ASSETS)
    boxes = np.stack([np.stack([hs.bvh(i)["nodes"][0]["aabbMin"], hs.bvh(i)["nodes"][0]["aabbMax"]]) for i in range(hs.bvh_count())])
    for p in range(len(c.T)):
        r = inp.restate(boxes, c.T[p])
        assert r["no_candidate"] is None and r["stale_a"] > 0, (p, r["stale_a"])


def test_bad_pose_is_the_middle_one(crt, tmp_path):
    c = pi.case("bad_pose")
    hs = crt.HostScene(inp.scene_xml(tmp_path, c.scene), 1, ASSETS)
    boxes = np.stack([np.stack([hs.bvh(i)["nodes"][0]["aabbMin"], hs.bvh(i)["nodes"][0]["aabbMax"]]) for i in range(hs.bvh_count())])
    assert [inp.restate(boxes, c.T[p])["no_candidate"] is None for p in range(3)] == [True, False, True]
