"""crt_build_kdtree_device / crt_get_kdtree — what runs without a GPU: the entries are exported and declared, and the HOST KDTree::Build that the device build is held
to equals the oracle's restatement of infra/kdtree.cpp byte for byte on every mesh of tests/kd_build_inputs.py (and the real kdtree.cpp where oracle/_ref is built,
else what it gave, recorded in tests/golden/kd_build_live.json), each of which is also asserted to have the shape it is there for."""
import ctypes as C
import json
import os
import re
import zlib

import numpy as np
import pytest

from conftest import REPO, GOLDEN
import kd_build_inputs as K

LIVE_JSON = os.path.join(GOLDEN, "kd_build_live.json")


def test_entries_are_exported_and_declared(crt):
    L = crt.lib()
    abi = open(os.path.join(REPO, "include", "crt_abi.h")).read()
    host = open(os.path.join(REPO, "include", "crt_host.h")).read()
    for name in ("crt_build_kdtree_device", "crt_get_kdtree"):
        assert name in crt.ABI_SYMBOLS and getattr(L, name) is not None
        assert re.search(r"int\s+%s\s*\(\s*crt_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+bvh" % name, abi)
    for name in ("crt_host_scene_build_kdtree_device", "crt_host_kd_build"):
        assert name in crt.HOST_SYMBOLS and getattr(L, name) is not None and re.search(r"int\s+%s\s*\(" % name, host)
    assert re.search(r"#define\s+CRT_ABI_VERSION\s+3\b", abi) and L.crt_abi_version() == 3
    for method in (crt.Context.build_kdtree_device, crt.Context.get_kdtree, crt.HostScene.build_kdtree_device, crt.host_kd_build):
        assert callable(method)
    pos = (C.c_float * 9)()
    assert L.crt_build_kdtree_device(None, C.c_uint32(0), pos, C.c_uint32(1), None) == -1        # CRT_ERR_INVALID before anything touches a device
    assert L.crt_get_kdtree(None, C.c_uint32(0), None, None, None, None, None) == -1


def tri_records(orc, p):
    tris = np.zeros(len(p), orc.TRI_DTYPE)
    tris["vertex0"], tris["vertex1"], tris["vertex2"] = p[:, 0], p[:, 1], p[:, 2]
    return tris


@pytest.fixture(scope="module")
def built(crt, orc):
    """name -> (positions, host build, oracle build), each computed once"""
    out = {}
    for name in K.NAMES:
        p = K.mesh(crt, name)
        a = orc.alt_accel("kd", tri_records(orc, p)); want = a.dump(); a.close()
        out[name] = (p, crt.host_kd_build(p), want)
    return out


@pytest.mark.parametrize("name", K.NAMES)
def test_host_build_equals_the_oracle(built, name):
    p, got, want = built[name]
    assert p.dtype == np.float32 and p.shape[1:] == (3, 3) and np.isfinite(p).all()
    K.assert_kd_equal(got, want, name)
    assert (got["maxDepth"], got["nodesUsed"]) == (want["maxDepth"], want["nodesUsed"])
    n = got["nodes"]; leaf = n["left"] < 0
    assert got["nodesUsed"] == len(n) and (n["right"][leaf] == -1).all() and (n["triCount"][~leaf] == 0).all()
    # firstTri of EVERY node counts the leaf references before it in pre-order
    before = np.concatenate([[0], np.cumsum(np.where(leaf, n["triCount"], 0))[:-1]])
    assert np.array_equal(n["firstTri"], before) and before[-1] + n["triCount"][-1] == len(got["refs"])
    d = K.depths(n)
    assert d.max() <= 20 and (n["triCount"][leaf & (d < 20)] <= 2).all()
    assert got["maxDepth"] == (d[~leaf].max() if (~leaf).any() else 0)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


@pytest.mark.parametrize("name", K.NAMES)
def test_host_build_equals_the_reference_live(orc, built, name):
    """the real infra/kdtree.cpp where oracle/_ref is built (and then the recording must not be stale), else its recorded shape + CRC32"""
    p, got, _ = built[name]
    mine = [len(got["nodes"]), len(got["refs"]), crc(got["nodes"]), crc(got["refs"]), int(got["maxDepth"]), int(got["nodesUsed"])]
    rec = json.load(open(LIVE_JSON)) if os.path.exists(LIVE_JSON) else {}
    try:
        ref = orc.Ref()
    except FileNotFoundError:
        ref = None
    if ref is not None:
        a = ref.alt_accel("kd", tri_records(orc, p)); want = a.dump(); a.close()
        K.assert_kd_equal(got, want, name + " vs the reference")
        assert (got["maxDepth"], got["nodesUsed"]) == (want["maxDepth"], want["nodesUsed"])
        if os.environ.get("CRT_RECORD_REF_LIVE") == "1":
            rec[name] = mine
            with open(LIVE_JSON, "w") as f:
                json.dump(rec, f, indent=1, sort_keys=True)
    assert rec[name] == mine, "%s: tests/golden/kd_build_live.json is stale (re-record with CRT_RECORD_REF_LIVE=1)" % name


def subtree_refs(t, node):
    """the leaf references below `node` of a pre-order tree (its subtree is the nodes up to the next sibling)"""
    n = t["nodes"]; end = node + 1; open_ = 2 if n["left"][node] >= 0 else 0
    while open_:                                                             # every interior node opens two more
        open_ += 1 if n["left"][end] >= 0 else -1
        end += 1
    last = end - 1
    return t["refs"][n["firstTri"][node]:n["firstTri"][last] + n["triCount"][last]]


def test_each_mesh_has_its_shape(built):
    for name in ("single", "pair"):
        n = built[name][1]["nodes"]
        assert len(n) == 1 and n["left"][0] == -1 and n["triCount"][0] == len(built[name][0])
    t = built["three"][1]
    assert len(t["nodes"]) == 3 and t["nodes"]["left"][0] == 1 and t["nodes"]["right"][0] == 2 and list(t["refs"]) == [0, 1, 2]
    for name in ("flat", "cluster"):                                         # triangles no plane separates: duplicated down to the depth limit
        n = built[name][1]["nodes"]; d = K.depths(n)
        assert ((n["left"] < 0) & (d == 20) & (n["triCount"] > 2)).any(), name
    t = built["coincident"][1]
    assert len(t["nodes"]) == 2 ** 21 - 1 and len(t["refs"]) == 3 * 2 ** 20 > 256 * 2048
    # margin: the 0.001 margin of the right-hand test, evaluated in double
    p, t, _ = built["margin"]
    n = t["nodes"]
    assert n["splitAxis"][0] == 0 and n["aabbMin"][0][0] == 0 and n["splitDistance"][0] == 1 and n["aabbMax"][n["left"][0]][0] == 1 and n["aabbMin"][n["right"][0]][0] == 1
    left, right = set(subtree_refs(t, n["left"][0])), set(subtree_refs(t, n["right"][0]))
    assert left == {0, 2, 4, 6, 7} and right == {1, 2, 3, 4, 5, 6}
    i = K.MARGIN_ROUNDED
    bmin, bmax, split = p[i, :, 0].min(), p[i, :, 0].max(), np.float32(1.0)
    assert bmin == np.float32(0.999) and not bmax < split
    assert float(bmin) > float(split) - 0.001                                # the reference's expression: right only
    assert not bmin > np.float32(split - np.float32(0.001))                  # a float32 evaluation: both
    # zeros: the root boxes of the two variants differ in their sign bits only
    a, b = built["zeros-neg"][1]["nodes"][0], built["zeros-pos"][1]["nodes"][0]
    for k in ("aabbMin", "aabbMax"):
        assert np.array_equal(a[k], b[k])
    assert np.signbit(a["aabbMin"][0]) and not np.signbit(b["aabbMin"][0]) and np.signbit(a["aabbMax"][2]) and not np.signbit(b["aabbMax"][2])
    # the moved bunny: a deep tree with duplicated references
    t = built["bunny_moved"][1]
    assert len(t["nodes"]) > 10000 and len(t["refs"]) > len(built["bunny_moved"][0]) and K.depths(t["nodes"]).max() == 20
