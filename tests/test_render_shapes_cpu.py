"""crt_render_shapes without a GPU: the two entries are exported, declared and bound, and the oracle side of tests/test_gpu_render_shapes.py is what that test
assumes — every camera of a case sees the deforming mesh in the shape it is paired with, no two views of a case are alike (so a lane that walks the wrong shape,
the wrong relocation or the live BVH cannot pass by coincidence), Refit does not depend on what was refitted before, the stale-node-1 case exercises the quirk,
the leaf-root case has no node pair, and the two shapes of the mixed-height case build TLASes of different heights."""
import inspect
import os

import numpy as np
import pytest

import render_shapes_inputs as si
import tlas_device_inputs as inp
from conftest import ASSETS, REPO


def test_symbols_are_exported_declared_and_bound(crt):
    L = crt.lib()
    header = open(os.path.join(REPO, "include", "crt_abi.h")).read()
    for name in ("crt_render_shapes", "crt_render_shapes_device"):
        assert name in crt.ABI_SYMBOLS
        assert hasattr(L, name), name
        assert ("int  %s(crt_ctx* ctx, const float* " % name) in header, name
    assert "#define CRT_ABI_VERSION 3" in header and L.crt_abi_version() == 3
    host = inspect.signature(crt.Context.render_shapes)
    assert list(host.parameters) == ["self", "cameras", "bvh", "positions", "spp_first", "frames", "passes", "scale", "T", "view_shape", "want_root_boxes", "want_tlas"]
    dev = inspect.signature(crt.Context.render_shapes_device)
    assert list(dev.parameters)[:7] == ["self", "cams", "bvh", "positions", "out", "spp_first", "frames"]


def pixel_centre_hits(o):
    xy = np.stack(np.meshgrid(np.arange(si.W) + 0.5, np.arange(si.H) + 0.5), axis=-1).reshape(-1, 2)
    return o.find_nearest(*o.primary_rays(xy))


@pytest.mark.parametrize("name", si.ALL_RENDERED)
def test_case_cameras_see_the_deforming_mesh_and_views_differ(orc, tmp_path, name):
    o = si.make_oracle(orc, tmp_path, si.case_scene(name))
    c = si.case(name, o)
    assert c.bvh != 0 or c.T is None                                       # a two-level case never deforms instance 0
    seen = {}
    for k in range(len(c.cameras)):
        acc, cnt = si.oracle_view(o, c, k)
        assert cnt["primary"] == 2 * 256 * c.frames * c.passes, (name, k, cnt)
        assert np.isfinite(acc).all() and (acc[..., :3] > 0).any(), (name, k)
        assert (pixel_centre_hits(o)["objIdx"] == 2 + c.bvh).any(), (name, "view", k, "does not see the deforming mesh")
        key = acc.tobytes()
        assert key not in seen, (name, "views", seen[key], k, "are equal")
        seen[key] = k
    assert len(seen) >= 2
    assert len({c.pos[s].tobytes() for s in range(len(c.pos))}) == len(c.pos)      # every shape of the case is a different one
    assert len(set(c.cameras)) == len(c.cameras)


def test_a_view_with_the_wrong_shape_differs(orc, tmp_path):
    """windows_48: views 0 and 1 under each other's shape are not what the case expects of them"""
    o = si.make_oracle(orc, tmp_path, "cube")
    c = si.case("windows_48", o)
    right = [si.oracle_view(o, c, k)[0] for k in (0, 1)]
    swapped = si.Case(c.scene, c.bvh, c.pos, c.T, c.cameras, [1 - s for s in c.view_shape], c.spp_first, c.frames, c.passes)
    for k in (0, 1):
        assert not np.array_equal(si.oracle_view(o, swapped, k)[0], right[k]), k


@pytest.mark.parametrize("name", ("cube_loop", "teapot_loop", "stale_node1", "tlas3_loop"))
def test_refit_does_not_depend_on_the_shape_before(orc, tmp_path, name):
    """shape s refitted after shape r gives the node boxes of shape s refitted from the upload: no refit writes node 1, which is all that could carry over"""
    scene = si.case_scene(name)
    fresh = si.make_oracle(orc, tmp_path, scene)
    c = si.case(name, fresh)
    uploaded = fresh.bvh(c.bvh)["nodes"].copy()
    want = []
    for s in range(len(c.pos)):
        o = si.make_oracle(orc, tmp_path, scene)
        o.move_and_refit(c.bvh, c.pos[s])
        want.append(o.bvh(c.bvh)["nodes"].tobytes())
    assert len(set(want)) == len(want)
    for r in range(len(c.pos)):
        for s in range(len(c.pos)):
            fresh.move_and_refit(c.bvh, c.pos[r]); fresh.move_and_refit(c.bvh, c.pos[s])
            nodes = fresh.bvh(c.bvh)["nodes"]
            assert nodes.tobytes() == want[s], (name, r, s)
            assert nodes[1].tobytes() == uploaded[1].tobytes(), (name, r, s)


def leaf_vertices(b, node, pos):
    """the vertices of the triangles in the leaves below `node`"""
    n = b["nodes"][node]
    if n["triCount"] > 0:
        return pos[b["triIndices"][n["leftFirst"]:n["leftFirst"] + n["triCount"]]].reshape(-1, 3)
    return np.concatenate([leaf_vertices(b, n["leftFirst"], pos), leaf_vertices(b, n["leftFirst"] + 1, pos)])


def test_stale_node1_case_exercises_the_quirk(orc, tmp_path):
    o = si.make_oracle(orc, tmp_path, "cube")
    c = si.case("stale_node1", o)
    for s in (1, 2):
        o.move_and_refit(0, c.pos[s])
        b = o.bvh(0)
        v = leaf_vertices(b, 1, c.pos[s])
        n1, n2 = b["nodes"][1], b["nodes"][2]
        assert ((v < n1["aabbMin"]) | (v > n1["aabbMax"])).any(), s          # node 1's box no longer holds its own triangles
        v2 = leaf_vertices(b, 2, c.pos[s])
        assert np.array_equal(v2.min(0), n2["aabbMin"]) and np.array_equal(v2.max(0), n2["aabbMax"]), s    # ... while node 2's was refitted


def test_leaf_root_case_has_no_node_pair(orc, crt, tmp_path):
    o = si.make_oracle(orc, tmp_path, "tiny")
    b = o.bvh(0)
    assert b["nodesUsed"] == 1 and b["nodes"][0]["triCount"] == 2
    xml, kind = si.scene_xml(tmp_path, "tiny")
    hb = crt.HostScene(xml, kind, ASSETS).bvh(0)
    assert hb["nodesUsed"] == 1 and np.array_equal(si.positions(o, 0), si.positions(crt.HostScene(xml, kind, ASSETS), 0))


def shape_boxes(o, c, s):
    """the node-0 boxes of every BLAS with the deforming one refitted to shape s"""
    o.move_and_refit(c.bvh, c.pos[s])
    return np.stack([np.stack([o.bvh(i)["nodes"][0]["aabbMin"], o.bvh(i)["nodes"][0]["aabbMax"]]) for i in range(o.bvh_count())])


def test_mixed_heights_premise(orc, tmp_path):
    o = si.make_oracle(orc, tmp_path, "ring40")
    c = si.case("mixed_heights", o)
    h = [inp.restate(shape_boxes(o, c, s), c.T[s])["height"] for s in (0, 1)]
    assert h[0] != h[1] and max(h) >= 2 * min(h), h


def test_bad_shape_is_the_middle_one(orc, tmp_path):
    """non-finite positions make the deforming BLAS's node-0 box NaN (a < b ? a : b keeps the NaN), and the build over it finds no partner"""
    o = si.make_oracle(orc, tmp_path, "tlas3")
    c = si.case("bad_shape", o)
    got = []
    for s in range(3):
        boxes = shape_boxes(o, c, s)
        if s == 1:
            assert np.isnan(boxes[c.bvh]).all() and np.isfinite(np.delete(boxes, c.bvh, axis=0)).all()
        got.append(inp.restate(boxes, c.T[s])["no_candidate"] is None)
    assert got == [True, False, True]
