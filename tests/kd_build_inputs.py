"""The meshes of the KD-tree build tests (tests/test_kd_device_cpu.py, tests/test_gpu_kd_device.py): those of tests/grid_build_inputs.py, and three more, each there
for one shape of KDTree::Build (infra/kdtree.cpp:4-108) that a device build can get wrong.  (n, 3, 3) float32 arrays — triangle, vertex, xyz."""
import numpy as np

from grid_build_inputs import single, flat, sliver, cluster, spanner, zeros, wobble, bunny_moved, scene_positions   # noqa: F401  (re-exported)


def pair():
    """2 triangles: the root stays a leaf by the count rule (<= 2)"""
    return np.array([[[0, 0, 0], [1, 0, 0.5], [0, 1, 1]], [[2, 0, 0], [3, 0, 0.5], [2, 1, 1]]], np.float32)


def three():
    """3 triangles, two of them left of the first split plane (x = 3) and one right of it: exactly one split"""
    return np.array([[[0, 0, 0], [1, 0, 0.5], [0, 1, 1]], [[1.5, 0, 0], [2.5, 0, 0.5], [1.5, 1, 1]], [[5, 0, 0], [6, 0, 0.5], [5, 1, 1]]], np.float32)


def coincident():
    """3 coincident triangles: no plane separates them, so every split sends all three to both sides down to the depth limit — 2^21 - 1 nodes and a last level of
    3 * 2^20 references, more than 256 chunks of the build's prefix sums (the size at which the one-workgroup pass over the chunk sums takes several per lane)"""
    return np.repeat(np.array([[[0, 0, 0], [4, 0, 4], [0, 4, 4]]], np.float32), 3, axis=0)


MARGIN_X = ((0.0, 0.5),                   # 0 wholly left of the first split plane x = 1
            (1.5, 2.0),                   # 1 wholly right
            (0.3, 1.0),                   # 2 bmax == splitPos: not left (strict <), so both
            (0.9995, 1.6),                # 3 starts left of the plane but inside the 0.001 margin: right only
            (0.9985, 1.6),                # 4 outside the margin: both
            (np.float32(0.999), 1.6),     # 5 the double comparison 0.99900001287 > 0.999 sends it right only; float32(1 - 0.001f) == float32(0.999) would say both
            (0.5, 1.5),                   # 6 straddling
            (0.1, 0.6))                   # 7 wholly left (its y range reaches the box's top, 1.7)
MARGIN_ROUNDED = 5


def margin():
    """8 triangles in the box [0, 2] x [0, 1.7] x [0, 0.3], stacked 0.2 apart in y (later splits separate them), their x ranges MARGIN_X"""
    t = []
    for i, (x0, x1) in enumerate(MARGIN_X):
        y0 = 0.2 * i; th = 0.3 if i == 7 else 0.1
        t.append([[x0, y0, 0.0], [x1, y0, 0.3], [x0, y0 + th, 0.0]])
    return np.array(t, np.float32)


GENERATED = {"single": single, "pair": pair, "three": three, "flat": flat, "sliver": sliver, "cluster": cluster, "spanner": spanner, "margin": margin, "coincident": coincident,
             "zeros-neg": lambda: zeros(True), "zeros-pos": lambda: zeros(False)}
NAMES = list(GENERATED) + ["bunny_moved"]


def mesh(crt, name):
    return bunny_moved(crt) if name == "bunny_moved" else GENERATED[name]()


def assert_kd_equal(a, b, what):
    """nodes and refs byte for byte (so -0.0 != +0.0), in the layout HostScene.build_alt / Context.get_kdtree / crt.host_kd_build / the oracle's dump share"""
    for k in ("nodes", "refs"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k, x.shape, y.shape)


def depths(nodes):
    """the depth of every node of a pre-order tree"""
    d = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes)):
        if nodes["left"][i] >= 0:
            d[nodes["left"][i]] = d[nodes["right"][i]] = d[i] + 1
    return d
