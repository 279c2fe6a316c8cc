"""crt_build_bvh_device / crt_get_bvh — what runs without a GPU: the entries are exported and declared, the HOST BVH::Build over bare positions that the device build
is held to (crt_host_bvh_build) equals HostScene's own build and, where oracle/_ref is built, the reference's bvh.cpp byte for byte on every mesh of
tests/bvh_build_inputs.py (else what that gave, recorded in tests/golden/bvh_build_live.json); each mesh has the shape it is there for; and the closed form of the
partition loop that the device build scatters by (the kernel's own lines, compiled for the host) equals the loop for every left / right pattern of up to 10 slots."""
import ctypes as C
import itertools
import json
import os
import re
import zlib

import numpy as np
import pytest

from conftest import REPO, GOLDEN, ASSETS, scene_path
import bvh_build_inputs as B

LIVE_JSON = os.path.join(GOLDEN, "bvh_build_live.json")


def test_entries_are_exported_and_declared(crt):
    L = crt.lib()
    abi = open(os.path.join(REPO, "include", "crt_abi.h")).read()
    host = open(os.path.join(REPO, "include", "crt_host.h")).read()
    for name in ("crt_build_bvh_device", "crt_get_bvh"):
        assert name in crt.ABI_SYMBOLS and getattr(L, name) is not None
        assert re.search(r"int\s+%s\s*\(\s*crt_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+bvh" % name, abi)
    for name in ("crt_host_bvh_build", "crt_host_scene_bvh_move_and_rebuild", "crt_host_scene_build_bvh_device"):
        assert name in crt.HOST_SYMBOLS and getattr(L, name) is not None and re.search(r"int\s+%s\s*\(" % name, host)
    assert re.search(r"#define\s+CRT_ABI_VERSION\s+3\b", abi) and L.crt_abi_version() == 3
    for method in (crt.Context.build_bvh_device, crt.Context.get_bvh, crt.HostScene.build_bvh_device, crt.HostScene.move_and_rebuild, crt.host_bvh_build):
        assert callable(method)
    pos = (C.c_float * 9)()
    assert L.crt_build_bvh_device(None, C.c_uint32(0), pos, C.c_uint32(1), None, None) == -1     # CRT_ERR_INVALID before anything touches a device
    assert L.crt_get_bvh(None, C.c_uint32(0), None, None, None, None, None) == -1
    assert L.crt_host_bvh_build(None, C.c_uint32(1), None, None, None) == -1
    assert L.crt_host_scene_bvh_move_and_rebuild(None, 0, pos, C.c_uint32(1)) == -1
    assert L.crt_host_scene_build_bvh_device(None, None, 0, pos, C.c_uint32(1), None) == -1


@pytest.fixture(scope="module")
def built(crt):
    """name -> (positions, host build), each computed once"""
    return {name: (B.mesh(crt, name), crt.host_bvh_build(B.mesh(crt, name))) for name in B.NAMES}


def test_host_build_equals_the_host_scenes_own(crt):
    """bare positions + recomputed centroids give the tree the loaded scene built, and move_and_rebuild gives the bare build of the moved positions"""
    hs = crt.HostScene(scene_path("bunny_scene.xml"), 0, ASSETS)
    b = hs.bvh(0)
    p = np.stack([b["tris"]["vertex0"], b["tris"]["vertex1"], b["tris"]["vertex2"]], axis=1)
    mine = crt.host_bvh_build(p)
    B.assert_bvh_equal(mine, dict(nodes=b["nodes"], indices=b["triIndices"], nodesUsed=b["nodesUsed"], maxDepth=b["maxDepth"]), "bunny")
    assert mine["height"] == B.depths(mine["nodes"]).max()
    moved = B.wobble(p)
    hs.move_and_rebuild(0, moved)
    b2 = hs.bvh(0)
    B.assert_bvh_equal(crt.host_bvh_build(moved), dict(nodes=b2["nodes"], indices=b2["triIndices"], nodesUsed=b2["nodesUsed"], maxDepth=b2["maxDepth"]), "moved bunny")
    assert np.array_equal(b2["tris"]["vertex1"], moved[:, 1]) and np.array_equal(b2["tris"]["centroid"], ((moved[:, 0] + moved[:, 1]) + moved[:, 2]) * np.float32(0.3333))
    assert b2["nodesUsed"] != b["nodesUsed"] or not np.array_equal(b2["triIndices"], b["triIndices"])       # a rebuild, not a refit


@pytest.mark.parametrize("name", B.NAMES)
def test_host_build_is_a_tree_over_every_triangle(built, name):
    p, t = built[name]
    n = t["nodes"]; leaf = n["triCount"] > 0
    assert t["nodesUsed"] == len(n) and len(n) % 2 == 1 and sorted(t["indices"]) == list(range(len(p)))
    assert n["triCount"][leaf].sum() == len(p)
    kids = n["leftFirst"][~leaf]
    assert sorted(np.concatenate([kids, kids + 1]).tolist()) == list(range(1, len(n))) and (kids % 2 == 1).all()
    d = B.depths(n)
    assert t["height"] == d.max() and t["maxDepth"] == (d[~leaf].max() if (~leaf).any() else 0)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


def summary(t, idx):
    return [int(t["nodesUsed"]), int(t["maxDepth"]), crc(t["nodes"]), crc(t[idx])]


@pytest.mark.parametrize("name", B.NAMES)
def test_host_build_equals_the_reference_live(orc, built, name):
    """The real infra/bvh.cpp where oracle/_ref is built, byte for byte; else its shape + CRC32 as recorded from it in tests/golden/bvh_build_live.json (which must
    not be stale where both exist).  The two zeros meshes are where the tie rule of the fold over a node's vertices shows: the reference build keeps the EARLIER of
    -0 and +0 (one triangle with x = (+0, -0, 5) has aabbMin.x = +0), and so does Builder::fit."""
    p, got = built[name]
    rec = json.load(open(LIVE_JSON)) if os.path.exists(LIVE_JSON) else {}
    try:
        ref = orc.Ref()
    except FileNotFoundError:
        ref = None
    if ref is not None:
        h, want = ref.bvh_build(B.tri_records(orc, p)); ref.bvh_free(h)
        if os.environ.get("CRT_RECORD_REF_LIVE") == "1":
            rec[name] = summary(want, "triIndices")
            with open(LIVE_JSON, "w") as f:
                json.dump(rec, f, indent=1, sort_keys=True)
        assert rec[name] == summary(want, "triIndices"), "%s: tests/golden/bvh_build_live.json is stale (re-record with CRT_RECORD_REF_LIVE=1)" % name
        B.assert_bvh_equal(got, dict(nodes=want["nodes"], indices=want["triIndices"], nodesUsed=want["nodesUsed"], maxDepth=want["maxDepth"]), name + " vs the reference")
    assert rec[name] == summary(got, "indices"), "%s: the host build differs from the reference's as recorded" % name


def test_each_mesh_has_its_shape(built):
    for name in ("single", "pair"):
        t = built[name][1]
        assert t["nodesUsed"] == 1 and t["nodes"]["triCount"][0] == len(built[name][0]) and t["height"] == 0
    # ulp: the plane rounds back to cmin, leftCount is 0: node 0 stays a leaf, its slots rotated by one by the partition loop that ran all the same
    t = built["ulp"][1]
    assert t["nodesUsed"] == 1 and t["nodes"]["triCount"][0] == 6 and list(t["indices"]) == [1, 2, 3, 4, 5, 0]
    assert B.partition_loop([False] * 6)[0] == [1, 2, 3, 4, 5, 0]
    # chain: one active node per level, numbering far from the level order
    t = built["chain"][1]
    assert t["height"] >= 16 and t["nodesUsed"] == 37
    d = B.depths(t["nodes"])
    assert all(((d == k) & (t["nodes"]["triCount"] == 0)).sum() <= 1 for k in range(d.max() + 1))
    # zeros: a box component of the two variants differs in its sign bit only
    a, b = built["zeros-neg"][1]["nodes"], built["zeros-pos"][1]["nodes"]
    assert len(a) == len(b)
    differs = False
    for k in ("aabbMin", "aabbMax"):
        assert np.array_equal(a[k], b[k])                                   # equal as values
        differs = differs or (np.signbit(a[k]) != np.signbit(b[k])).any()
    assert differs
    # the moved bunny: the root spans many workgroups of 256 slots, and some level has thousands of nodes
    p, t = built["bunny_moved"]
    assert len(p) == 4968 and t["nodesUsed"] > 4000 and np.bincount(B.depths(t["nodes"])).max() > 1000


def test_partition_closed_form_equals_the_loop(crt):
    """the kernel's own closed form (compiled for the host) against the loop: every pattern of up to 10 slots, and random ones of up to 300"""
    for n in range(1, 11):
        for left in itertools.product((False, True), repeat=n):
            assert B.partition_device_form(crt, left) == B.partition_loop(left), left
    rng = np.random.default_rng(3)
    for _ in range(300):
        left = (rng.random(int(rng.integers(11, 301))) < rng.random()).tolist()
        assert B.partition_device_form(crt, left) == B.partition_loop(left), left
