"""The meshes of the BVH build tests (tests/test_bvh_device_cpu.py, tests/test_gpu_bvh_device.py): those of tests/kd_build_inputs.py except `coincident` (a KD-tree
shape), and two more, each there for one shape of BVH::Build (infra/bvh.cpp:63-178, binned SAH) that a device build can get wrong.  (n, 3, 3) float32 arrays —
triangle, vertex, xyz.  Also here: the reference's partition loop, restated, and the closed form of it that the device build uses, called in the library."""
import numpy as np

import kd_build_inputs as K
from kd_build_inputs import wobble, bunny_moved, scene_positions   # noqa: F401  (re-exported)


def ulp():
    """6 triangles, each with all its vertices at one x: three at x = 2^20 near y = 0, three at the next float above it near y = 10.  The x centroids of the two
    groups are a few ulps apart near 1048471; the chosen plane is one of the x axis, and `cmin + scale * (i + 1)` rounds back to cmin: no centroid is below it,
    leftCount is 0 and node 0 stays a leaf — after the partition loop has rotated its slots by one (triangleIndices = 1 2 3 4 5 0)."""
    X = np.float32(2 ** 20); X1 = np.nextafter(X, np.float32(2 ** 21))
    t = []
    for k in range(6):
        x = X if k < 3 else X1; y = np.float32(0.0) if k < 3 else np.float32(10.0)
        t.append([[x, y, 0], [x, y + 1, 0], [x, y, 1]])
    return np.array(t, np.float32)


def chain(n=24):
    """24 triangles at x = 8^i: every split takes the one or two outermost triangles off, so one node is active per level, the tree is as tall as a tree of 24
    triangles gets here (height 18) and the depth-first numbering as far from the level order as it gets"""
    t = []
    for i in range(n):
        x = np.float32(8.0 ** i)
        t.append([[x, 0, 0], [x, 0, 0.5], [x, 1, 1]])
    return np.array(t, np.float32)


GENERATED = {k: v for k, v in K.GENERATED.items() if k != "coincident"}
GENERATED.update(ulp=ulp, chain=chain)
NAMES = list(GENERATED) + ["bunny_moved"]


def mesh(crt, name):
    return bunny_moved(crt) if name == "bunny_moved" else GENERATED[name]()


def assert_bvh_equal(a, b, what):
    """nodes and triangleIndices byte for byte (so -0.0 != +0.0), nodesUsed and maxDepth: the layout Context.get_bvh and crt.host_bvh_build share"""
    assert (a["nodesUsed"], a["maxDepth"]) == (b["nodesUsed"], b["maxDepth"]), (what, a["nodesUsed"], a["maxDepth"], b["nodesUsed"], b["maxDepth"])
    for k in ("nodes", "indices"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k, x.shape, y.shape)


def depths(nodes):
    """the depth of every node: children are numbered behind their parent"""
    d = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes)):
        if nodes["triCount"][i] == 0:
            d[nodes["leftFirst"][i]] = d[nodes["leftFirst"][i] + 1] = d[i] + 1
    return d


def tri_records(orc, p):
    """reference Tri records of bare positions, centroids as model.cpp:77 computes them"""
    tris = np.zeros(len(p), orc.TRI_DTYPE)
    tris["vertex0"], tris["vertex1"], tris["vertex2"] = p[:, 0], p[:, 1], p[:, 2]
    tris["centroid"] = ((p[:, 0] + p[:, 1]) + p[:, 2]) * np.float32(0.3333)
    return tris


# ---- the partition ----
def partition_loop(left):
    """bvh.cpp:96-103 over slots 0 .. n - 1 holding elements 0 .. n - 1; left[e]: element e's centroid is below the plane.  Returns (order, leftCount)."""
    a = list(range(len(left))); i = 0; j = len(a) - 1
    while i <= j:
        if left[a[i]]:
            i += 1
        else:
            a[i], a[j] = a[j], a[i]; j -= 1
    return a, i


def partition_device_form(crt, left):
    """the closed form of that loop as the device build scatters by it — bvh_partition_dest of csrc/device/build_common.h, the kernel's own lines compiled for the host
    (crt_debug_bvh_partition).  Returns (order, leftCount)."""
    import ctypes as C
    flags = np.array(left, np.uint8); out = np.zeros(len(flags), np.uint32)
    n_left = crt.lib().crt_debug_bvh_partition(flags.ctypes.data_as(C.c_void_p), C.c_uint32(len(flags)), out.ctypes.data_as(C.c_void_p))
    assert n_left >= 0, ("two slots mapped to one place, or a place outside the segment", left)
    return out.tolist(), n_left
