"""float32 restatement of the Whitted renderer's traversal inspection ("2. WhittedStyle/renderer.cpp":38-39, 147-152; infra/helper.h:104-120
GetTraverseCountColor), operation by operation in np.float32, and of the single-threaded pixel order that defines which peak a pixel is coloured with:

    peakIn(i) = max(peak carried into the Tick, max over pixels j < i of count(j))      i = x + y * W
    pixel(i)  = sky colour if the primary ray misses, GetTraverseCountColor(count(i), peakIn(i)) otherwise

Nothing here touches the library under test."""
import numpy as np

F = np.float32
INV_MAX = F(1) / F(255)                                              # const float invMax = 1 / 255.f
GREEN = (F(179) * INV_MAX, F(255) * INV_MAX, F(174) * INV_MAX)       # float3 green(179 * invMax, 255 * invMax, 174 * invMax)
RED = (F(255) * INV_MAX, F(50) * INV_MAX, F(50) * INV_MAX)


def traverse_count_color(traversed, peak):
    """GetTraverseCountColor(int traversed, int peak) for arrays of the same shape; returns float32 (..., 3)"""
    traversed = np.asarray(traversed, np.int64); peak = np.broadcast_to(np.asarray(peak, np.int64), traversed.shape)
    out = np.empty(traversed.shape + (3,), F)
    small = peak < 10
    t = np.clip(traversed, 0, np.maximum(peak, 0))                   # clamp(traversed, 0, peak)
    with np.errstate(divide="ignore", invalid="ignore"):
        blend = t.astype(F) / peak.astype(F)                         # traversed / (float)peak
    for k in range(3):
        d = F(RED[k] - GREEN[k])
        prod = (blend * d).astype(F)                                 # separate multiply ...
        out[..., k] = np.where(small, GREEN[k], (GREEN[k] + prod).astype(F))   # ... and add
    assert out.dtype == F and blend.dtype == F
    return out


def running_peak(count, peak_in):
    """exclusive prefix maximum of `count` (H, W) in row-major order, seeded with peak_in: the peak each pixel is coloured with"""
    flat = np.asarray(count, np.int64).ravel()
    incl = np.maximum.accumulate(np.concatenate([[int(peak_in)], flat]))
    return incl[:-1].reshape(np.shape(count)), int(incl[-1])


def rgb8(rgb):
    """RGBF32_to_RGB8 (template/precomp.h:336-340, scalar branch) of float32 (..., 3)"""
    c = (F(255) * np.minimum(F(1), rgb.astype(F))).astype(F).astype(np.uint32)
    return (c[..., 0] << 16) + (c[..., 1] << 8) + c[..., 2]


def heat_map(count, hit, sky_acc, peak_in):
    """one inspect Tick: count (H, W) int, hit (H, W) bool (objIdx != -1), sky_acc (H, W, 4) float32 giving the missed pixels' accumulator.
    Returns (accumulator (H, W, 4) float32, screen (H, W) uint32, peak carried out, peakIn per pixel)."""
    peaks, peak_out = running_peak(count, peak_in)
    acc = np.zeros(np.shape(count) + (4,), F)
    acc[..., :3] = traverse_count_color(count, peaks)
    acc[~hit] = sky_acc[~hit]
    return acc, rgb8(acc[..., :3]), peak_out, peaks


def metrics(traversed, tested, peak_traversal_in=0, peak_tests_in=0):
    """renderer.cpp:147-152 over the primary rays, totals as exact integers"""
    tr = np.asarray(traversed, np.int64); te = np.asarray(tested, np.int64)
    return dict(rayHitCount=int((tr > 0).sum()), totalTraversal=int(tr.sum()), totalTests=int(te.sum()),
                peakTraversal=max(int(peak_traversal_in), int(tr.max())), peakTests=max(int(peak_tests_in), int(te.max())))
