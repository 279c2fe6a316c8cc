"""crt_render_shape_sets without a GPU: the two entries are exported, declared and bound, and the oracle side of tests/test_gpu_render_shape_sets.py is what that
test assumes — the refits of a set commute, every mesh of every case is seen deforming by some view of the case (so a lane that walks the live BVH, or the
sub-image of another mesh, cannot pass by coincidence), no two shapes look alike through the same camera, the stale-node-1 case exercises the quirk in BOTH of
its meshes, the leaf-root case has no node pair, and the two shapes of ring40_all build TLASes of different heights."""
import inspect
import os

import numpy as np
import pytest

import render_shape_sets_inputs as ss
import render_shapes_inputs as si
import tlas_device_inputs as inp
from conftest import ASSETS, REPO
from test_render_shapes_cpu import leaf_vertices


def test_symbols_are_exported_declared_and_bound(crt):
    L = crt.lib()
    header = open(os.path.join(REPO, "include", "crt_abi.h")).read()
    for name in ("crt_render_shape_sets", "crt_render_shape_sets_device"):
        assert name in crt.ABI_SYMBOLS
        assert hasattr(L, name), name
        assert ("int  %s(crt_ctx* ctx, const float* " % name) in header, name
    assert "#define CRT_ABI_VERSION 3" in header and L.crt_abi_version() == 3
    host = inspect.signature(crt.Context.render_shape_sets)
    assert list(host.parameters) == ["self", "cameras", "bvhs", "positions", "spp_first", "frames", "passes", "scale", "T", "view_shape", "want_root_boxes", "want_tlas"]
    dev = inspect.signature(crt.Context.render_shape_sets_device)
    assert list(dev.parameters)[:7] == ["self", "cams", "bvhs", "positions", "out", "spp_first", "frames"]


@pytest.mark.parametrize("name", ss.LOOP_CASES + ("stale_node1", "leaf_root"))
def test_the_refits_of_a_set_commute(orc, tmp_path, name):
    """move_and_refit of the set's BVHs in either order, followed by set_transform, gives the same accumulator (and the same nodes)"""
    a, b = ss.make_oracle(orc, tmp_path, ss.case_scene(name)), ss.make_oracle(orc, tmp_path, ss.case_scene(name))
    c = ss.case(name, a)
    for s in range(len(c.T)):
        for o, order in ((a, range(len(c.bvhs))), (b, reversed(range(len(c.bvhs))))):
            for m in order:
                o.move_and_refit(c.bvhs[m], c.pos[m][s])
            for i in range(len(c.T[s])):
                o.set_transform(i, c.T[s][i])
            o.set_camera_state(*c.cameras[s]); o.clear(); o.set_spp(c.spp_first); o.set_params(5, c.passes); o.render(c.frames, 4)
        assert a.accumulator().tobytes() == b.accumulator().tobytes(), (name, s)
        for i in c.bvhs:
            assert a.bvh(i)["nodes"].tobytes() == b.bvh(i)["nodes"].tobytes(), (name, s, i)


@pytest.mark.parametrize("name", ss.ALL_RENDERED)
def test_every_mesh_of_a_case_is_seen_deforming(orc, tmp_path, name):
    """for every m: some view of the case, rendered with only mesh m deformed (by the case's largest factor), differs from the same view with nothing deformed"""
    o = ss.make_oracle(orc, tmp_path, ss.case_scene(name))
    c = ss.case(name, o)
    big = c.with_factors(c.factors.max() + 1e-4 * np.arange(c.factors.size).reshape(c.factors.shape))
    views = list(range(min(len(c.cameras), 4)))
    plain = [ss.oracle_view(o, big, k, only=-1)[0].tobytes() for k in views]
    for k in views:
        cnt = ss.oracle_view(o, big, k)[1]
        assert cnt["primary"] == 2 * 256 * c.frames * c.passes, (name, k, cnt)
    for m in range(len(c.bvhs)):
        assert any(ss.oracle_view(o, big, k, only=m)[0].tobytes() != plain[k] for k in views), (name, "mesh", m, "BLAS", c.bvhs[m], "is not seen deforming")


@pytest.mark.parametrize("name", ss.ALL_RENDERED)
def test_shapes_differ_through_the_same_camera(orc, tmp_path, name):
    """view k under its own shape and under the next shape of the case are different images, and every view of the case is a different image"""
    o = ss.make_oracle(orc, tmp_path, ss.case_scene(name))
    c = ss.case(name, o)
    S, seen = len(c.T), {}
    for k in range(len(c.cameras)):
        acc = ss.oracle_view(o, c, k)[0]
        assert np.isfinite(acc).all() and (acc[..., :3] > 0).any(), (name, k)
        other = ss.oracle_view(o, c, k, shape=(c.shape_of(k) + 1) % S)[0]
        assert acc.tobytes() != other.tobytes(), (name, "view", k, "looks the same under the next shape")
        assert acc.tobytes() not in seen, (name, "views", seen[acc.tobytes()], k, "are equal")
        seen[acc.tobytes()] = k
    assert len(set(c.cameras)) == len(c.cameras)
    assert len({(m, c.pos[m][s].tobytes()) for m in range(len(c.bvhs)) for s in range(S)}) == S * len(c.bvhs)


def test_the_block_order_follows_bvhs(orc, tmp_path):
    """tlas3_all names the BLASes as [2, 0, 1]: its positions' blocks are theirs in that order, and no two blocks are alike"""
    o = ss.make_oracle(orc, tmp_path, "tlas3")
    c = ss.case("tlas3_all", o)
    assert c.bvhs == [2, 0, 1]
    counts = [o.bvh(b)["tris"].shape[0] for b in c.bvhs]
    flat = c.set_positions()
    assert flat.shape == (3, sum(counts), 9)
    at = 0
    for m, n in enumerate(counts):
        assert np.array_equal(flat[:, at:at + n].reshape(3, n, 3, 3), c.pos[m])
        at += n


def test_stale_node1_case_exercises_the_quirk_in_both_meshes(orc, tmp_path):
    o = ss.make_oracle(orc, tmp_path, "tlas3")
    c = ss.case("stale_node1", o)
    for s in range(len(c.T)):
        for m, bvh in enumerate(c.bvhs):
            o.move_and_refit(bvh, c.pos[m][s])
            b = o.bvh(bvh)
            v = leaf_vertices(b, 1, c.pos[m][s])
            n1 = b["nodes"][1]
            assert ((v < n1["aabbMin"]) | (v > n1["aabbMax"])).any(), (s, bvh)      # node 1's box no longer holds its own triangles


def test_leaf_root_case_has_no_node_pair(orc, crt, tmp_path):
    o = ss.make_oracle(orc, tmp_path, "tiny3")
    assert o.bvh_count() == 3
    xml, kind = ss.scene_xml(tmp_path, "tiny3")
    hs = crt.HostScene(xml, kind, ASSETS)
    for i in range(3):
        b = o.bvh(i)
        assert b["nodesUsed"] == 1 and b["nodes"][0]["triCount"] == 2
        assert hs.bvh(i)["nodesUsed"] == 1 and np.array_equal(si.positions(o, i), si.positions(hs, i))
        assert np.array_equal(hs.blas_transform(i)[0].reshape(4, 4), ss.tiny3_poses(1)[0][i])


def set_boxes(o, c, s):
    """the node-0 boxes of every BLAS with the set refitted to shape s"""
    for m, b in enumerate(c.bvhs):
        o.move_and_refit(b, c.pos[m][s])
    return np.stack([np.stack([o.bvh(i)["nodes"][0]["aabbMin"], o.bvh(i)["nodes"][0]["aabbMax"]]) for i in range(o.bvh_count())])


def test_ring40_all_mixes_tlas_heights(orc, tmp_path):
    o = ss.make_oracle(orc, tmp_path, "ring40")
    c = ss.case("ring40_all", o)
    assert sorted(c.bvhs) == list(range(40)) and c.bvhs != sorted(c.bvhs)
    h = [inp.restate(set_boxes(o, c, s), c.T[s])["height"] for s in (0, 1)]
    assert h[0] != h[1] and max(h) >= 2 * min(h), h


def test_bad_mesh_spoils_the_middle_shape_only(orc, tmp_path):
    """non-finite positions in one mesh of shape 1 make that BLAS's node-0 box NaN, and the build over the row finds no partner"""
    o = ss.make_oracle(orc, tmp_path, "tlas3")
    c = ss.case("bad_mesh", o)
    got = []
    for s in range(3):
        boxes = set_boxes(o, c, s)
        if s == 1:
            assert np.isnan(boxes[c.bvhs[1]]).all() and np.isfinite(np.delete(boxes, c.bvhs[1], axis=0)).all()
        got.append(inp.restate(boxes, c.T[s])["no_candidate"] is None)
    assert got == [True, False, True]
