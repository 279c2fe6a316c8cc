"""The pool kernel's floor class (device/layout.h kTileFloorSure, device/tile_class.h classify_tiles) without a GPU: crt_debug_tile_classes_host_ex returns the whole
class byte of a bare Scene block, and for every tile with bit 3 set a float32 numpy restatement of the kernel's ray generation and of hit_light_floor<true>'s floor
half (operand order as in dev_common.h and in test_tile_class_cpu.py) must ACCEPT every ray of the tile, 0 < t < 1e34: the 256 pixels x the jitters
{0, 2^-32, 0.5, 1 - 2^-24, 1.0} on both axes, and 2 000 random rays.  A set bit is a proof, so nothing here has a tolerance; the floors on the counts keep the
proof from being vacuous.  The entries that predate the bit keep returning bits 0..2 for the same inputs."""
import ctypes as C

import numpy as np
import pytest

from test_tile_class_cpu import CAMERAS, bunny, camera_state, default_camera, hits_of, rays_of_tile       # noqa: F401  (bunny: the module's fixture)

f32 = np.float32


def classes(crt, scene, cam, W, H, part=None, flags=7):
    first, stride, count = part if part else (0, 1, (W // 16) * (H // 16))
    ex = crt.tile_classes_host(cam, scene["light"], scene["size"], scene["floor_d"], scene["pair"], W, H, first, stride, count, flags=flags, ex=True)
    old = crt.tile_classes_host(cam, scene["light"], scene["size"], scene["floor_d"], scene["pair"], W, H, first, stride, count, flags=flags)
    assert ex.shape == old.shape == (count,)
    assert (ex & ~np.uint8(15)).max(initial=0) == 0
    assert np.array_equal(old, ex & np.uint8(7)), "the old entry returns the three kTileNo* bits of the same table"
    assert not ((ex & crt.TILE_FLOOR_SURE != 0) & (ex & crt.TILE_NO_FLOOR != 0)).any(), "a tile cannot both always and never hit the floor"
    return ex


def check_view(crt, scene, cam, W, H, max_tiles=400):
    """every (of a large image: an even sample of the) tile with bit 3: all of its test rays pass the floor test; a kTileFloor tile carries kTileNoLight"""
    tilesX = W // 16
    cls = classes(crt, scene, cam, W, H)
    rng = np.random.default_rng(11)
    marked = np.flatnonzero(cls & crt.TILE_FLOOR_SURE)
    if len(marked) > max_tiles:
        marked = np.unique(np.concatenate([marked[::max(1, len(marked) // max_tiles)], marked[:8], marked[-8:]]))
    for i in marked:
        tx, ty = int(i) % tilesX, int(i) // tilesX
        X, Y = rays_of_tile(cam, W, H, tx, ty, rng)
        _, floor, _ = hits_of(scene, cam, W, H, X, Y)                       # (tf < 1e34) & (tf > 0)
        assert floor.all(), "tile (%d, %d) is marked as always hitting the floor, but %d of its %d test rays fail that test" % (tx, ty, int((~floor).sum()), len(floor))
        if (cls[i] & crt.TILE_FLOOR) == crt.TILE_FLOOR:
            assert cls[i] & crt.TILE_NO_LIGHT
    return cls


def test_library_exports_the_entries(crt):
    L = C.CDLL(crt.build())
    for name in ("crt_debug_tile_classes_ex", "crt_debug_tile_classes_host_ex", "crt_debug_tile_classes", "crt_debug_tile_classes_host"):
        assert hasattr(L, name), name
    assert crt.TILE_FLOOR_SURE == 8 and crt.TILE_FLOOR == 13


def test_default_view_of_the_benchmark(crt, bunny):
    cls = check_view(crt, bunny, default_camera(1280, 720), 1280, 720)
    assert len(cls) == 3600
    floor = (cls & crt.TILE_FLOOR) == crt.TILE_FLOOR
    print("1280x720 default view: kTileFloor tiles", int(floor.sum()), "kTileFloorSure", int((cls & crt.TILE_FLOOR_SURE != 0).sum()))
    # the 22 rows below the horizon hold 1 760 tiles, 441 tiles see the tree
    assert floor.sum() >= 1000
    assert not (cls.reshape(45, 80)[:22] & crt.TILE_FLOOR_SURE).any()


def test_default_view_small_image_every_tile(crt, bunny):
    cls = check_view(crt, bunny, default_camera(160, 96), 160, 96)
    assert len(cls) == 60 and ((cls & crt.TILE_FLOOR) == crt.TILE_FLOOR).sum() >= 1


@pytest.mark.parametrize("name", sorted(CAMERAS))
@pytest.mark.parametrize("W,H", [(160, 96), (1280, 720)])
def test_other_cameras(crt, bunny, name, W, H):
    cam = camera_state(crt, W, H, *CAMERAS[name])
    cls = check_view(crt, bunny, cam, W, H, max_tiles=120)
    if name == "below_the_floor":
        # the eye is under the plane (num < 0) and looks up at it: the rays that go up hit it from underneath
        assert (cls & crt.TILE_FLOOR_SURE).any()


def test_straight_down(crt, bunny):
    """a horizontal screen plane below the camera: every ray goes down, so every tile always hits the floor"""
    for W, H in ((160, 96), (1280, 720)):
        a = f32(W) / f32(H)
        cam = np.array([0, 2.5, 2, -a, 1.5, 3, a, 1.5, 3, -a, 1.5, 1], f32)
        cls = check_view(crt, bunny, cam, W, H, max_tiles=120)
        assert (cls & crt.TILE_FLOOR_SURE).all()


def test_far_from_the_origin_sets_no_bit(crt, bunny):
    for W, H in ((160, 96), (1280, 720)):
        cam = camera_state(crt, W, H, (1e6, 0.0, -2.0), (1e6, 0.0, 0.0))
        assert not classes(crt, bunny, cam, W, H).any()


def test_a_general_floor_sets_no_bit(crt, bunny):
    """floorAxisY clear (a plane that is not exactly (0, 1, 0)): the kernel evaluates the general expressions, the proof does not apply"""
    W, H = 160, 96
    cam = default_camera(W, H)
    full = classes(crt, bunny, cam, W, H)
    assert (full & crt.TILE_FLOOR_SURE).any()
    off = classes(crt, bunny, cam, W, H, flags=7 & ~2)
    assert not (off & (crt.TILE_FLOOR_SURE | crt.TILE_NO_FLOOR)).any()
    assert np.array_equal(off, full & ~np.uint8(crt.TILE_FLOOR_SURE | crt.TILE_NO_FLOOR))


def test_the_eye_on_the_plane_sets_no_bit(crt, bunny):
    """num == 0: t is 0 (or NaN) for every ray, never accepted"""
    W, H = 160, 96
    cam = camera_state(crt, W, H, (0.0, -1.0, -2.0), (0.0, -1.5, 2.0))
    assert f32(cam[1]) + bunny["floor_d"] == 0
    cls = classes(crt, bunny, cam, W, H)
    assert not (cls & crt.TILE_FLOOR_SURE).any()


def test_tile_partition(crt, bunny):
    W, H = 1280, 720
    cam = default_camera(W, H)
    whole = classes(crt, bunny, cam, W, H)
    part = crt.tile_partition(1, 8, len(whole))
    cls = classes(crt, bunny, cam, W, H, part=part)
    assert np.array_equal(cls, whole[part[0]::part[1]][:part[2]]) and (cls & crt.TILE_FLOOR_SURE).any()
