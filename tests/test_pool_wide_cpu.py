"""The scenes that do not fit render_pool_kernel's 16-bit node references (assets/scenes/bunny4_scene.xml, bunny14_scene.xml, bunny4_tlas_scene.xml), without a
GPU: the host front loads and builds them as the oracle does, and — the precondition of tests/test_gpu_pool_wide.py — the primary rays of the test camera
really do hit triangles whose leaf-order index needs the wide reference, and triangles whose index does not."""
import numpy as np
import pytest

from conftest import ASSETS, scene_path

W, H = 96, 64                                    # the GPU tests' shape
SCENES = [("bunny4_scene.xml", 0, [19872]), ("bunny14_scene.xml", 0, [69552]), ("bunny4_tlas_scene.xml", 1, [4968] * 4)]


def leaf_positions_of_primary_hits(orc, xml):
    """leaf-order position (the index the pool reference of a leaf carries, minus one) of the triangle every primary ray of the W x H test camera hits"""
    o, _ = orc.load_scene(scene_path(xml), 0, ASSETS)
    o.renderer_init(W, H)
    xy = np.stack(np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5), -1).reshape(-1, 2)
    O, D = o.primary_rays(xy)
    h = o.find_nearest(O, D)
    idx = o.bvh(0)["triIndices"]
    where = np.empty(len(idx), np.int64)
    where[idx] = np.arange(len(idx))             # triangleIndices[position] = triIdx
    mesh = h["objIdx"] >= 2
    return where[h["triIdx"][mesh]], np.unique(h["objIdx"][mesh])


def test_bunny14_primary_rays_hit_leaves_on_both_sides_of_16_bits(orc):
    pos, objs = leaf_positions_of_primary_hits(orc, "bunny14_scene.xml")
    assert len(objs) == 14                       # the camera sees every bunny
    assert (pos > 65535).sum() >= 100 and (pos <= 16383).sum() >= 100, ((pos > 65535).sum(), (pos <= 16383).sum())


def test_bunny4_primary_rays_hit_leaves_past_the_14_bit_index(orc):
    pos, objs = leaf_positions_of_primary_hits(orc, "bunny4_scene.xml")
    assert len(objs) == 4
    assert (pos > 16383).sum() >= 100, (pos > 16383).sum()


@pytest.mark.parametrize("xml,kind,tris", SCENES)
def test_host_front_builds_the_large_scenes_as_the_oracle_does(crt, orc, xml, kind, tris):
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    o, _ = orc.load_scene(scene_path(xml), kind, ASSETS)
    assert hs.bvh_count() == o.bvh_count() == len(tris)
    for i, n in enumerate(tris):
        a, b = hs.bvh(i), o.bvh(i)
        assert len(a["tris"]) == len(b["tris"]) == n
        assert a["nodesUsed"] == b["nodesUsed"] and a["maxDepth"] == b["maxDepth"]
        assert a["nodes"].tobytes() == b["nodes"].tobytes() and np.array_equal(a["triIndices"], b["triIndices"])
    if kind == 1:
        assert hs.tlas()[0].tobytes() == o.tlas()[0].tobytes()
    # every one of them is past the 16-bit form's limit: <= 16383 node pairs and < 16383 triangles over all BVHs
    assert sum(tris) >= 16383
