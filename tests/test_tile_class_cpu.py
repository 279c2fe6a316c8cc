"""The pool kernel's tile classes (device/tile_class.h classify_tiles) without a GPU: crt_debug_tile_classes_host classifies the tiles of a bare Scene block, and
for every tile with a bit set a float32 numpy restatement of the kernel's ray generation and of the skipped test — the light quad, the floor plane, the slab test
against rootPair, operand order as in dev_common.h — must report no hit for any ray of the tile: the 256 pixels x the jitters {0, 2^-32, 0.5, 1 - 2^-24, 1.0} on both
axes, and 2 000 random rays.  A set bit is a proof, so nothing here has a tolerance; the floors on the bit counts keep the proof from being vacuous."""
import ctypes as C
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from conftest import ASSETS, scene_path

f32 = np.float32
JITTERS = np.array([0.0, 2.0 ** -32, 0.5, 1.0 - 2.0 ** -24, 1.0], f32)
T_FAR = f32(1e34)                      # FindNearest's initial t: the loosest bound any of the tests sees


@pytest.fixture(scope="module")
def bunny(crt):
    """what an upload of the bunny scene puts into the Scene block: the light's offsets, its size, the floor's d, the BVH root's child pair"""
    xml = scene_path("bunny_scene.xml")
    lp = ET.parse(xml).getroot().find("light_position")
    pos = np.array([f32(lp.find(k).text) for k in "xyz"], f32)
    hs = crt.HostScene(xml, crt.SCENE_FILE, ASSETS)
    nodes = hs.bvh(0)["nodes"]
    left = int(nodes[0]["leftFirst"])
    pair = np.zeros(16, f32)
    for c in range(2):
        pair[8 * c:8 * c + 3] = nodes[left + c]["aabbMin"]; pair[8 * c + 4:8 * c + 7] = nodes[left + c]["aabbMax"]
    return dict(light=-pos, size=f32(0.5), floor_d=f32(1.0), pair=pair)      # Quad(0, 1) translated to the light position; Plane((0,1,0), 1)


def default_camera(W, H):
    a = f32(W) / f32(H)                                                   # crt_create: Camera() defaults
    return np.array([0, 0, -2, -a, 1, 0, a, 1, 0, -a, -1, 0], f32)


def camera_state(crt, W, H, pos, target):
    L = crt.lib()
    a = [(C.c_float * 3)() for _ in range(4)]
    assert L.crt_host_camera_state(W, H, (C.c_float * 3)(*pos), (C.c_float * 3)(*target), *a) == 0
    return np.array([list(x) for x in a], f32).reshape(12)


def min_std(a, b): return np.where(b < a, b, a)
def max_std(a, b): return np.where(a < b, b, a)


def rays_of_tile(cam, W, H, tx, ty, rng):
    """(x + jx, y + jy) of the test rays of a tile as the kernel forms them: float(x) + jitter in float32"""
    px, py = np.meshgrid(np.arange(16, dtype=np.int64) + 16 * tx, np.arange(16, dtype=np.int64) + 16 * ty)
    X = (px.reshape(-1, 1, 1).astype(f32) + JITTERS.reshape(1, -1, 1) + np.zeros((1, 1, 5), f32)).reshape(-1)
    Y = (py.reshape(-1, 1, 1).astype(f32) + JITTERS.reshape(1, 1, -1) + np.zeros((1, 5, 1), f32)).reshape(-1)
    rx = (rng.integers(0, 16, 2000) + 16 * tx).astype(f32) + (rng.integers(0, 2 ** 32, 2000, dtype=np.uint64).astype(f32) * f32(2.0 ** -32))
    ry = (rng.integers(0, 16, 2000) + 16 * ty).astype(f32) + (rng.integers(0, 2 ** 32, 2000, dtype=np.uint64).astype(f32) * f32(2.0 ** -32))
    return np.concatenate([X, rx]).astype(f32), np.concatenate([Y, ry]).astype(f32)


def hits_of(scene, cam, W, H, X, Y):
    """float32 restatement of the END pass's ray generation, hit_light_floor<true>'s two halves and box_exact_rel on both root children: which rays each test accepts"""
    O, TL = cam[0:3], cam[3:6]
    right, down = cam[6:9] - cam[3:6], cam[9:12] - cam[3:6]                # primRight, primDown
    invW, invH = f32(1.0) / f32(W), f32(1.0) / f32(H)
    u, vv = (X * invW).astype(f32), (Y * invH).astype(f32)
    with np.errstate(all="ignore"):
        P = [((TL[k] + u * right[k]).astype(f32) + vv * down[k]).astype(f32) for k in range(3)]
        v = [(P[k] - O[k]).astype(f32) for k in range(3)]
        dot = ((v[0] * v[0] + v[1] * v[1]).astype(f32) + v[2] * v[2]).astype(f32)
        inv = (f32(1.0) / np.sqrt(dot, dtype=f32)).astype(f32)
        D = [(v[k] * inv).astype(f32) for k in range(3)]
        rD = [(f32(1.0) / D[k]).astype(f32) for k in range(3)]
        # Quad::Intersect, the lightAxis form with the camera-relative sums
        Oy, Ox, Oz = f32(O[1] + scene["light"][1]), f32(O[0] + scene["light"][0]), f32(O[2] + scene["light"][2])
        t = (Oy / -D[1]).astype(f32)
        Ix, Iz = (Ox + t * D[0]).astype(f32), (Oz + t * D[2]).astype(f32)
        size = scene["size"]
        light = (t < T_FAR) & (t > 0) & (Ix > -size) & (Ix < size) & (Iz > -size) & (Iz < size)
        # Plane::Intersect, the floorAxisY form
        num = f32(O[1] + scene["floor_d"])
        tf = (-num / D[1]).astype(f32)
        floor = (tf < T_FAR) & (tf > 0)
        # the slab test of both root children on lo - camPos, hi - camPos (primRoot)
        tree = np.zeros(len(X), bool)
        for c in range(2):
            lo = (scene["pair"][8 * c:8 * c + 3] - O).astype(f32); hi = (scene["pair"][8 * c + 4:8 * c + 7] - O).astype(f32)
            t1, t2 = (lo[0] * rD[0]).astype(f32), (hi[0] * rD[0]).astype(f32)
            tmin, tmax = min_std(t1, t2), max_std(t1, t2)
            for k in (1, 2):
                t1, t2 = (lo[k] * rD[k]).astype(f32), (hi[k] * rD[k]).astype(f32)
                tmin = max_std(tmin, min_std(t1, t2)); tmax = min_std(tmax, max_std(t1, t2))
            tree |= (tmax >= tmin) & (tmin < T_FAR) & (tmax > 0)
    return light, floor, tree


def check_view(crt, scene, cam, W, H, part=None, max_tiles=400):
    """classify, then hold every set bit to the restated tests (all classified tiles of a small image; an even sample of a large one, every class present in it)"""
    tilesX, tiles = W // 16, (W // 16) * (H // 16)
    first, stride, count = part if part else (0, 1, tiles)
    cls = crt.tile_classes_host(cam, scene["light"], scene["size"], scene["floor_d"], scene["pair"], W, H, first, stride, count)
    assert cls.shape == (count,) and (cls & ~np.uint8(7)).max(initial=0) == 0
    rng = np.random.default_rng(7)
    marked = np.flatnonzero(cls)
    if len(marked) > max_tiles:
        marked = np.unique(np.concatenate([marked[::max(1, len(marked) // max_tiles)], marked[:8], marked[-8:]]))
    for i in marked:
        tile = first + int(i) * stride
        tx, ty = tile % tilesX, tile // tilesX
        X, Y = rays_of_tile(cam, W, H, tx, ty, rng)
        light, floor, tree = hits_of(scene, cam, W, H, X, Y)
        for bit, hit, what in ((crt.TILE_NO_LIGHT, light, "light quad"), (crt.TILE_NO_FLOOR, floor, "floor plane"), (crt.TILE_NO_TREE, tree, "root children")):
            if cls[i] & bit:
                assert not hit.any(), "tile (%d, %d) is marked as unable to hit the %s, but %d of its %d test rays pass that test" % (tx, ty, what, int(hit.sum()), len(hit))
    return cls


def test_library_exports_the_entries(crt):
    L = C.CDLL(crt.build())
    for name in ("crt_debug_tile_classes", "crt_debug_tile_classes_host"):
        assert hasattr(L, name), name


def test_default_view_of_the_benchmark(crt, bunny):
    cls = check_view(crt, bunny, default_camera(1280, 720), 1280, 720)
    counts = {b: int(((cls & b) == b).sum()) for b in (crt.TILE_SKY, crt.TILE_NO_TREE, crt.TILE_NO_LIGHT, crt.TILE_NO_FLOOR)}
    print("1280x720 default view: sky", counts[crt.TILE_SKY], "no tree", counts[crt.TILE_NO_TREE], "no light", counts[crt.TILE_NO_LIGHT], "no floor", counts[crt.TILE_NO_FLOOR])
    assert len(cls) == 3600
    assert counts[crt.TILE_SKY] >= 1400 and counts[crt.TILE_NO_TREE] >= 2900 and counts[crt.TILE_NO_LIGHT] == 3600
    # the horizon is the centre row: no tile below it may claim to miss the floor, and the tiles over the bunny see the tree
    assert not (cls.reshape(45, 80)[23:] & crt.TILE_NO_FLOOR).any()
    assert (cls & crt.TILE_NO_TREE).sum() // crt.TILE_NO_TREE < 3600


def test_default_view_small_image_every_tile(crt, bunny):
    cls = check_view(crt, bunny, default_camera(160, 96), 160, 96)
    assert len(cls) == 60 and (cls == crt.TILE_SKY).any() and (cls & crt.TILE_NO_TREE == 0).any()


CAMERAS = {
    "up_at_the_light": ((0.0, -0.5, -1.0), (0.0, 3.0, 1.0)),
    "below_the_floor": ((0.3, -3.0, -2.0), (0.0, -1.0, 2.0)),
    "beside_the_mesh": ((1.5, 0.7, -3.0), (0.2, -0.1, 2.0)),
}


@pytest.mark.parametrize("name", sorted(CAMERAS))
@pytest.mark.parametrize("W,H", [(160, 96), (1280, 720)])
def test_other_cameras(crt, bunny, name, W, H):
    cam = camera_state(crt, W, H, *CAMERAS[name])
    cls = check_view(crt, bunny, cam, W, H, max_tiles=120)
    if name == "up_at_the_light":
        assert (cls & crt.TILE_NO_LIGHT == 0).any(), "the camera looks at the light: some tile must be left able to hit it"
        assert (cls & crt.TILE_NO_LIGHT != 0).any()
    if name == "below_the_floor":
        assert (cls & crt.TILE_NO_FLOOR == 0).any()                         # looking up at the floor from underneath


def test_straight_down(crt, bunny):
    """a horizontal screen plane below the camera (which hangs between the mesh and the light): v.y is the same for every pixel"""
    for W, H in ((160, 96), (1280, 720)):
        a = f32(W) / f32(H)
        cam = np.array([0, 2.5, 2, -a, 1.5, 3, a, 1.5, 3, -a, 1.5, 1], f32)
        cls = check_view(crt, bunny, cam, W, H, max_tiles=120)
        assert not (cls & crt.TILE_NO_FLOOR).any() and (cls & crt.TILE_NO_LIGHT).all()       # every ray goes down: all can hit the floor, none the light above
        above = np.array([0, 4, 2, -a, 2, 3, a, 2, 3, -a, 2, 1], f32)                         # from above the light: the quad is hit from either side
        cls = check_view(crt, bunny, above, W, H, max_tiles=120)
        assert (cls & crt.TILE_NO_LIGHT == 0).any() and (cls & crt.TILE_NO_LIGHT != 0).any()


def test_inside_the_root_box(crt, bunny):
    pair = bunny["pair"]
    lo = np.minimum(pair[0:3], pair[8:11]); hi = np.maximum(pair[4:7], pair[12:15])
    mid = ((lo + hi) * f32(0.5)).astype(f32)
    for W, H in ((160, 96), (1280, 720)):
        cam = camera_state(crt, W, H, tuple(mid), (float(mid[0]), float(mid[1]), float(mid[2]) + 1.0))
        cls = check_view(crt, bunny, cam, W, H, max_tiles=120)
        assert not (cls & crt.TILE_NO_TREE).any()                           # corners behind the eye: the bit is cleared everywhere


def test_far_from_the_origin_sets_no_bit(crt, bunny):
    """1e6 away: one pixel's step is below 2^-16 of the coordinates, float rounding is no longer small against the guard band"""
    for W, H in ((160, 96), (1280, 720)):
        cam = camera_state(crt, W, H, (1e6, 0.0, -2.0), (1e6, 0.0, 0.0))
        cls = crt.tile_classes_host(cam, bunny["light"], bunny["size"], bunny["floor_d"], bunny["pair"], W, H)
        assert not cls.any()


def test_tile_partition(crt, bunny):
    """rank 1 of 8 of the 720p image: the partition's table is the whole image's, strided"""
    W, H = 1280, 720
    cam = default_camera(W, H)
    whole = crt.tile_classes_host(cam, bunny["light"], bunny["size"], bunny["floor_d"], bunny["pair"], W, H)
    part = crt.tile_partition(1, 8, len(whole))
    cls = check_view(crt, bunny, cam, W, H, part=part, max_tiles=60)
    assert len(cls) == part[2] and np.array_equal(cls, whole[part[0]::part[1]][:part[2]])


def test_flags_switch_the_bits_off(crt, bunny):
    """a general light / floor (lightAxis, floorAxisY clear) or a root that is a leaf (rootIsPair clear) leaves that bit clear everywhere"""
    W, H = 160, 96
    cam = default_camera(W, H)
    full = crt.tile_classes_host(cam, bunny["light"], bunny["size"], bunny["floor_d"], bunny["pair"], W, H)
    for flag, bit in ((1, crt.TILE_NO_LIGHT), (2, crt.TILE_NO_FLOOR), (4, crt.TILE_NO_TREE)):
        cls = crt.tile_classes_host(cam, bunny["light"], bunny["size"], bunny["floor_d"], bunny["pair"], W, H, flags=7 & ~flag)
        assert not (cls & bit).any() and np.array_equal(cls, full & ~np.uint8(bit))
