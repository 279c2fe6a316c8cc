"""The compact sample slab's layout (device/sample_body.h) without a GPU: crt_debug_slab_layout evaluates, on the host, the position and
size functions the render kernels store through and accumulate_kernel / commit_frame_kernel load through.  A launch's slab is [64-frame window][local tile] tile
blocks; a tile holds 12-byte samples, or — a sky launch's tile whose accumulate follows at once — 4-byte texels in the first third of the same block.

Held here: every (frame, tile, pixel, pass) has a byte range of its own inside its tile's block of its window, texel rows lie in sky blocks only, and the bytes a
window's writers touch are the closed form the change was sized with (0.526 of the float4 slab for the default job's 3 600 tiles, 1 613 of them sky)."""
import ctypes as C
import itertools

import numpy as np
import pytest

SAMPLE, TEXEL, FLOAT4 = 12, 4, 16


def layout(crt, texel, frames, tiles, passes):
    """positions [frame][tile][pixel][pass], bytes per window of samples, bytes per tile block"""
    L = crt.lib()
    L.crt_debug_slab_layout.restype = C.c_int
    L.crt_debug_slab_layout.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    pos = np.zeros((frames, tiles, 256, passes), np.uint64); sizes = np.zeros(2, np.uint64)
    assert L.crt_debug_slab_layout(int(texel), frames, tiles, passes, pos.ctypes.data, sizes.ctypes.data) == 0
    return pos.astype(np.int64), int(sizes[0]), int(sizes[1])


def window_bytes_touched(tiles, sky, passes, frames=64):
    """what the writers of one window of `frames` frames store: 12 bytes per sample, 4 per sample of a sky tile"""
    return 256 * frames * passes * ((tiles - sky) * SAMPLE + sky * TEXEL)


@pytest.mark.parametrize("passes,tiles,frames", list(itertools.product([1, 2, 3, 4], [1, 3, 6], [1, 8, 64, 130])))
def test_every_sample_has_its_own_bytes_inside_its_block(crt, passes, tiles, frames):
    samp, win_bytes, tile_bytes = layout(crt, False, frames, tiles, passes)
    texl, win_bytes_t, tile_bytes_t = layout(crt, True, frames, tiles, passes)
    assert tile_bytes == tile_bytes_t == 256 * 64 * passes * SAMPLE and win_bytes == win_bytes_t == tiles * tile_bytes     # one block pitch for both forms
    assert (samp % 4 == 0).all() and (texl % 4 == 0).all() and win_bytes % 4 == 0                                          # (the factor scratch behind the samples stays aligned)
    fr = np.arange(frames)[:, None, None, None]; tl = np.arange(tiles)[None, :, None, None]
    block = (fr // 64) * win_bytes + tl * tile_bytes                                                                       # [window][local tile]
    windows = (frames + 63) // 64
    for sky in sorted({0, min(2, tiles), tiles}):                                                                          # the sky tail: the last `sky` tiles hold texels
        is_sky = (np.arange(tiles) >= tiles - sky)[None, :, None, None]
        start = np.where(is_sky, texl, samp); size = np.where(is_sky, TEXEL, SAMPLE) + np.zeros_like(start)
        assert (start >= block).all() and (start + size <= block + tile_bytes).all()                                       # inside its tile's block of its window
        assert (start + size <= windows * win_bytes).all()
        order = np.argsort(start, axis=None)
        s, e = start.ravel()[order], (start + size).ravel()[order]
        assert (s[1:] >= e[:-1]).all()                                                                                     # disjoint from every other
        if sky:
            t = texl[:, tiles - sky:]
            assert (t + TEXEL <= (block + tile_bytes // 3)[:, tiles - sky:]).all()                                         # a sky tile touches the first third of its block
            full = frames // 64 * 64                                                                                       # texel rows: the 64 frames of one (pixel, pass) are 256 contiguous bytes
            if full:
                rows = t[:64].transpose(1, 2, 3, 0)
                assert (np.diff(rows, axis=-1) == TEXEL).all()
        touched = int(size.sum())
        assert touched == sum(window_bytes_touched(tiles, sky, passes, min(64, frames - 64 * w)) for w in range(windows))
    # the sample form's rows: a pixel's samples in the order they are added — (frame-in-window, pass) — 12 bytes apart
    rows = samp[:min(frames, 64)].transpose(1, 2, 0, 3).reshape(tiles, 256, -1)
    assert (np.diff(rows, axis=-1) == SAMPLE).all()


def test_bytes_per_window_of_the_default_job(crt):
    """1280x720: 3 600 tiles, 1 613 of them sky, one pass — 943.7 MB as float4, 496.4 MB compact: the factor 0.526"""
    tiles, sky = 3600, 1613
    samp, win_bytes, tile_bytes = layout(crt, False, 1, tiles, 1)
    assert win_bytes == tiles * 256 * 64 * SAMPLE                                                # what the slab pool holds per window: 707.8 MB (float4: 943.7 MB)
    float4 = tiles * 256 * 64 * FLOAT4
    compact = window_bytes_touched(tiles, sky, 1)
    assert float4 == 943718400 and compact == 496369664
    assert round(compact / float4, 3) == 0.526
    # ... and at that size both forms start every tile's rows at its block (frame 0; the per-sample structure is the test above's)
    texl, _, _ = layout(crt, True, 1, tiles, 1)
    starts = np.arange(tiles) * tile_bytes
    assert np.array_equal(samp[0, :, 0, 0], starts) and np.array_equal(texl[0, :, 0, 0], starts)
    assert int(samp[0, :, 255, 0].max()) + 64 * SAMPLE == win_bytes and int(texl[0, :, 255, 0].max()) + 64 * TEXEL == win_bytes - 2 * (tile_bytes // 3)
