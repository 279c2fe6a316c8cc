"""The generated meshes of the grid-build tests (tests/test_grid_device_cpu.py, tests/test_gpu_grid_device.py): each a (n, 3, 3) float32 array — triangle, vertex,
xyz — from a fixed formula or seed, and each there for one shape of Grid::Build (infra/grid.cpp:4-50) that a device build can get wrong."""
import numpy as np

from conftest import ASSETS, scene_path


def single():
    """1 triangle"""
    return np.array([[[0, 0, 0], [1, 0, 0.5], [0, 1, 1]]], np.float32)


def flat():
    """8 triangles, all with z = 0.5: a grid of volume 0 (the resolution lines meet inf and NaN, the z range 0 / 0)"""
    t = []
    for i in range(4):
        x, y = np.float32(i % 2), np.float32(i // 2)
        t.append([[x, y, 0.5], [x + 1, y, 0.5], [x + 1, y + 1, 0.5]])
        t.append([[x, y, 0.5], [x + 1, y + 1, 0.5], [x, y + 1, 0.5]])
    return np.array(t, np.float32)


def sliver():
    """64 triangles strung along x in [0, 100] with y, z extents of 0.01: the clamp of the resolution at 128"""
    i = np.arange(64, dtype=np.float64)
    x0, x1 = i * (100.0 / 64.0), (i + 1) * (100.0 / 64.0)
    z = np.zeros(64)
    return np.stack([np.stack([x0, z, z], 1), np.stack([x1, z + 0.01, z], 1), np.stack([(x0 + x1) / 2, z, z + 0.01], 1)], 1).astype(np.float32)


def cluster():
    """300 triangles of size <= 0.002 inside [0, 0.01]^3 plus one near (10, 10, 10): one cell with hundreds of references, most cells empty"""
    rng = np.random.default_rng(7)
    base = rng.uniform(0.0, 0.008, (300, 1, 3))
    small = base + rng.uniform(0.0, 0.002, (300, 3, 3))
    far = np.array([[[10, 10, 10], [9.9, 10, 10], [10, 9.9, 9.95]]])
    return np.concatenate([small, far]).astype(np.float32)


def spanner():
    """one triangle (0,0,0), (4,0,4), (0,4,4), whose box is the whole grid, plus 200 of size 0.1 scattered in [0, 4]^3"""
    rng = np.random.default_rng(11)
    base = rng.uniform(0.0, 3.9, (200, 1, 3))
    small = base + rng.uniform(0.0, 0.1, (200, 3, 3))
    big = np.array([[[0, 0, 0], [4, 0, 4], [0, 4, 4]]])
    return np.concatenate([big, small]).astype(np.float32)


def dense():
    """120 000 triangles of size <= 0.01 spread over [0, 1]^3: a grid of 84^3 = 592 704 cells, more than 256 x 2048 counters, so the one-block pass of the
    device's prefix sum over its chunk sums takes more than one chunk per thread"""
    rng = np.random.default_rng(13)
    base = rng.uniform(0.0, 0.99, (120000, 1, 3))
    return (base + rng.uniform(0.0, 0.01, (120000, 3, 3))).astype(np.float32)


def zeros(last_negative):
    """The minimum x of the mesh is 0 and the maximum z is 0; the vertices that tie there include some at -0.0 and some at +0.0 (two of them inside one triangle).
    The last tying vertex in (triangle, vertex) order is -0.0 (last_negative) or +0.0, for x and for z alike."""
    rng = np.random.default_rng(3)
    p = rng.uniform(0.25, 1.0, (8, 3, 3)).astype(np.float32)
    p[..., 2] = -p[..., 2]                                                  # z in [-1, -0.25]
    first, last = (np.float32(0.0), np.float32(-0.0)) if last_negative else (np.float32(-0.0), np.float32(0.0))
    for axis in (0, 2):
        p[1, 1, axis] = first
        p[3, 0, axis] = last; p[3, 2, axis] = first                         # inside one triangle: the later vertex wins the triangle's box
        p[5, 1, axis] = first
        p[6, 2, axis] = last                                                # the last one in the mesh
    return p


def scene_positions(crt, xml="bunny_scene.xml", kind=0, bvh=0):
    """the triangle positions of a scene's BVH in the reference's triangles[] order, (n, 3, 3) float32"""
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    t = hs.bvh(bvh)["tris"]
    hs.close()
    return np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1).astype(np.float32)


def wobble(p):
    """p += 0.15 * sin(3 * p.yzx): a deformation large enough to change the grid's resolution (float64 sine, rounded once)"""
    p = np.asarray(p, np.float32)
    return (p.astype(np.float64) + 0.15 * np.sin(3.0 * p[..., [1, 2, 0]].astype(np.float64))).astype(np.float32)


def bunny_moved(crt):
    """bunny.obj's triangles as the bunny scene holds them, wobbled"""
    return wobble(scene_positions(crt))


GENERATED = {"single": single, "flat": flat, "sliver": sliver, "cluster": cluster, "spanner": spanner, "dense": dense,
             "zeros-neg": lambda: zeros(True), "zeros-pos": lambda: zeros(False)}
NAMES = list(GENERATED) + ["bunny_moved"]


def mesh(crt, name):
    return bunny_moved(crt) if name == "bunny_moved" else GENERATED[name]()


GRID_KEYS = ("resolution", "cellSize", "boundsMin", "boundsMax", "cellStart", "refs")


def assert_grids_equal(a, b, what):
    """byte for byte (so -0.0 != +0.0), in the layout HostScene.build_alt / Context.get_grid / the oracle's dump share"""
    for k in GRID_KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)
