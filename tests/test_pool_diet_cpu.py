"""The Scene's camera-relative block (layout.h set_primary: what render_pool_kernel's END pass multiplies by a primary ray's reciprocal direction instead of
forming `lo - camPos` per lane) without a GPU: crt_debug_primary_block_host applies the block's writers to a bare Scene in the order of a session — the values an
upload sets, the camera setter's, a rebuilt root pair — and returns rootPair and the block.  Each value must be the ONE float32 operation the kernels perform, so
numpy's float32 arithmetic gives the same bits.  (On a context with a GPU the same is read back after a real upload, camera change and scene update:
tests/test_gpu_pool_diet.py.)"""
import ctypes as C

import numpy as np

from conftest import ASSETS, scene_path


def expected_block(pair, cam, light, floor_d):
    O = cam[0:3]
    root = np.concatenate([pair[0:3] - O, pair[4:7] - O, pair[8:11] - O, pair[12:15] - O])
    lf = np.array([O[1] + light[7], O[0] + light[3], O[2] + light[11], O[1] + floor_d], np.float32)
    return np.concatenate([root, lf, cam[6:9] - cam[3:6], cam[9:12] - cam[3:6]]).astype(np.float32)


def test_library_exports_the_entries(crt):
    L = C.CDLL(crt.build())
    for name in ("crt_debug_primary_block", "crt_debug_primary_block_host", "crt_debug_check_sqrt", "crt_debug_sky_probe"):
        assert hasattr(L, name), name


def test_block_follows_upload_camera_and_update(crt):
    L = crt.lib()
    L.crt_debug_primary_block_host.restype = C.c_int
    L.crt_debug_primary_block_host.argtypes = [C.c_int, C.c_void_p, C.c_void_p]

    def apply(op, values):
        v = np.ascontiguousarray(values, np.float32); out = np.zeros(16 + 22, np.float32)
        assert L.crt_debug_primary_block_host(op, v.ctypes.data, out.ctypes.data) == 0
        return out[:16].copy(), out[16:].copy()

    # the root pair of a real scene: the bunny's BVH root children, as the uploader lays them out (lo, ref, hi, ref16 per child)
    hs = crt.HostScene(scene_path("bunny_scene.xml"), crt.SCENE_FILE, ASSETS)
    nodes = hs.bvh(0)["nodes"]
    left = int(nodes[0]["leftFirst"])
    pair = np.zeros(16, np.float32)
    for c in range(2):
        pair[8 * c:8 * c + 3] = nodes[left + c]["aabbMin"]; pair[8 * c + 4:8 * c + 7] = nodes[left + c]["aabbMax"]
        pair[8 * c + 3] = np.float32(1e-40); pair[8 * c + 7] = np.float32(2e-40)     # the reference words: bit patterns, never operands
    light = np.eye(4, dtype=np.float32)[:3].reshape(12).copy(); light[[3, 7, 11]] = [-0.31, -2.97, 0.13]       # an unrotated quad: translation only
    floor_d = np.float32(1.0)
    cam0 = np.array([0, 0, -2, -1, 1, 0, 1, 1, 0, -1, -1, 0], np.float32)                                       # the defaults a new Scene starts with

    got_pair, block = apply(0, np.concatenate([light, [floor_d], pair]))                                        # upload
    assert got_pair.tobytes() == pair.tobytes()
    assert block.tobytes() == expected_block(pair, cam0, light, floor_d).tobytes()

    cam1 = np.array([1.5, 0.7, -3.0, -0.913, 1.31, -1.77, 1.02, 1.29, -2.21, -0.87, -0.69, -1.8], np.float32)
    _, block1 = apply(1, cam1)                                                                                  # camera change: root pair and light as uploaded
    assert block1.tobytes() == expected_block(pair, cam1, light, floor_d).tobytes()
    assert not np.array_equal(block1, block)

    pair2 = pair.copy(); pair2[[0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]] += np.float32(0.37)
    got_pair2, block2 = apply(2, pair2)                                                                         # host-side update: a refitted root pair, camera as set
    assert got_pair2.tobytes() == pair2.tobytes()
    assert block2.tobytes() == expected_block(pair2, cam1, light, floor_d).tobytes()
    assert not np.array_equal(block2[:12], block1[:12]) and np.array_equal(block2[12:], block1[12:])

    # values whose difference is not exactly representable: one rounding, to nearest
    cam3 = cam1.copy(); cam3[0:3] = [np.float32(1e-3), np.float32(3e7), np.float32(-1.0000001)]
    _, block3 = apply(1, cam3)
    assert block3.tobytes() == expected_block(pair2, cam3, light, floor_d).tobytes()
