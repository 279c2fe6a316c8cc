"""The pool kernel's instruction diet ("instruction diet"): every item is an identity of IEEE or of address arithmetic, so nothing here has a
tolerance.  The short square root against the compiler's over all 2^32 inputs; the sky lookup behind its wave-uniform guard against the unguarded functions, with
the special operands alone in a wavefront and mixed into ordinary ones; the Scene's camera-relative block, formed on the host, after every kind of write that
makes it stale; the record pieces fetched at immediate offsets on the watch-tower scene.  The renders are held to the oracle bit for bit."""
import ctypes as C

import numpy as np
import pytest

import probe_inputs as pi
from conftest import ASSETS, scene_path

pytestmark = pytest.mark.gpu


def test_sqrt_exact_over_all_inputs(crt):
    ctx = crt.Context(64, 64)
    out = np.zeros(2, np.uint64)
    ctx.L.crt_debug_check_sqrt.restype = C.c_int
    ctx.L.crt_debug_check_sqrt.argtypes = [C.c_void_p, C.c_void_p]
    assert ctx.L.crt_debug_check_sqrt(ctx.h, out.ctypes.data) == 0
    print("sqrt_exact: inputs", int(out[0]), "differences", int(out[1]))
    assert out[0] == 1 << 32
    assert out[1] == 0, "sqrt_exact differs from __builtin_sqrtf for %d inputs" % out[1]


# ---- the guarded sky lookup (probe op 17 through crt_debug_sky_probe) against the unguarded functions (op 8) ----
def special_directions():
    """directions whose lookup takes a special case of crt_atan2f / crt_acosf, or sits next to one: along each axis, with +-0 components, |D.y| = 1 and just
    beyond, denormal, infinite and NaN components"""
    one, zero = np.float32(1), np.float32(0)
    den = [np.float32(1e-45), np.float32(-1e-45), pi.f32([0x007fffff])[0], pi.f32([0x807fffff])[0]]
    rows = []
    for s in (one, -one):
        rows += [[s, zero, zero], [zero, s, zero], [zero, zero, s], [s, -zero, -zero], [-zero, s, -zero], [-zero, -zero, s]]
        rows += [[zero, np.nextafter(s, 2 * s), zero], [zero, np.nextafter(s, zero), zero], [np.float32(0.6) * s, np.float32(0.8), zero], [zero, np.float32(0.8), np.float32(0.6) * s]]
        rows += [[np.float32(0.6) * s, np.float32(0.8), -zero], [-zero, np.float32(-0.8), np.float32(0.6) * s], [s, np.float32(1.5), s], [s, np.float32(-1.5), s]]
    for d in den:
        rows += [[d, np.float32(0.5), one], [one, np.float32(0.5), d], [one, d, one], [d, d, d], [d, np.float32(0.5), -d]]
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    for v in (inf, -inf, nan):
        rows += [[v, zero, one], [one, zero, v], [one, v, one], [v, np.float32(0.5), v], [v, np.float32(0.5), -v], [v, v, v]]
    return np.array(rows, np.float32)


def unit_directions(n=200000, seed=17):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    return (d / np.sqrt((d * d).sum(axis=1, keepdims=True), dtype=np.float32)).astype(np.float32)


def sky_records_of(D, w=4096, h=2048):
    r = np.zeros((len(D), 5), np.uint32); r[:, :3] = np.ascontiguousarray(D, np.float32).view(np.uint32); r[:, 3] = w; r[:, 4] = h
    return r


@pytest.fixture(scope="module")
def probes(crt):
    ctx = crt.Context(64, 64)
    ctx.L.crt_debug_device_probe.restype = C.c_int
    ctx.L.crt_debug_device_probe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32]
    ctx.L.crt_debug_sky_probe.restype = C.c_int
    ctx.L.crt_debug_sky_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]

    def run(records):
        r = np.ascontiguousarray(records, np.uint32)
        plain = np.zeros((len(r), 3), np.uint32); guarded = np.zeros((len(r), 3), np.uint32)
        assert ctx.L.crt_debug_device_probe(ctx.h, 8, r.ctypes.data, plain.ctypes.data, len(r)) == 0
        assert ctx.L.crt_debug_sky_probe(ctx.h, r.ctypes.data, guarded.ctypes.data, len(r)) == 0
        return plain, guarded
    return run


def assert_same_lookup(records, plain, guarded, what):
    """phi and theta as floats (any NaN equals any NaN, the suite's rule), the texel index exactly"""
    bad = np.union1d(pi.differing(guarded[:, :2].copy().view(np.float32), plain[:, :2].copy().view(np.float32)), np.flatnonzero(guarded[:, 2] != plain[:, 2]))
    assert len(bad) == 0, "%s: %d of %d lookups differ; first: D bits %s guarded %s unguarded %s" % (what, len(bad), len(records), records[bad[0], :3], guarded[bad[0]], plain[bad[0]])


def is_special(D):
    """what sky_angles' guard looks at: a zero, infinite or NaN x / z component, or |y| > 1 (NaN included)"""
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(D[:, 0]) | ~np.isfinite(D[:, 2]) | (D[:, 0] == 0) | (D[:, 2] == 0) | ~(np.abs(D[:, 1]) <= 1)


def test_sky_lookup_of_the_probe_inputs(probes):
    r = pi.sky_records()
    plain, guarded = probes(r)
    assert_same_lookup(r, plain, guarded, "probe_inputs.sky_records")


def test_sky_lookup_of_unit_directions(probes):
    D = unit_directions()
    whole = (~is_special(D))[:64 * (len(D) // 64)].reshape(-1, 64).all(axis=1)
    assert whole.sum() > 1000                                             # wavefronts without a special operand: the plain forms ran
    r = sky_records_of(D)
    plain, guarded = probes(r)
    assert_same_lookup(r, plain, guarded, "unit directions")
    assert (guarded[:, 2] < 4096 * 2048).all()


def test_sky_lookup_of_special_directions_alone_and_mixed(probes):
    S = special_directions()
    assert is_special(S).sum() > 40 and (~is_special(S)).sum() > 10       # the list holds both the specials and their ordinary neighbours (denormal components)
    # alone: whole wavefronts of one special direction each (the guard sends the wavefront to the general functions) ...
    alone = np.repeat(S, 64, axis=0)
    # ... and mixed: each special direction in one lane (a different one from wavefront to wavefront) of a wavefront of ordinary directions; and next to them the
    # same ordinary wavefronts without it, which take the plain forms
    U = unit_directions(64 * len(S), seed=23)
    U = U[~is_special(U)][:64 * (len(S) - 1)]
    U = np.concatenate([U, U[:64 * len(S) - len(U)]])
    mixed = U.copy()
    lanes = (np.arange(len(S)) * 7) % 64
    mixed[np.arange(len(S)) * 64 + lanes] = S
    for what, D in (("alone", alone), ("mixed", mixed), ("ordinary", U)):
        r = sky_records_of(D)
        plain, guarded = probes(r)
        assert_same_lookup(r, plain, guarded, what)
    groups = is_special(mixed).reshape(-1, 64).sum(axis=1)
    assert (groups <= 1).all() and (groups == 1).sum() == is_special(S).sum() and not is_special(U).any()


# ---- the camera-relative block of the Scene (layout.h set_primary) after every write that makes it stale ----
def primary_block(ctx):
    out = np.zeros(16 + 22, np.float32); cam = np.zeros(12, np.float32); lf = np.zeros(4, np.float32)
    ctx.L.crt_debug_primary_block.restype = C.c_int
    ctx.L.crt_debug_primary_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert ctx.L.crt_debug_primary_block(ctx.h, out.ctypes.data, cam.ctypes.data, lf.ctypes.data) == 0
    return out[:16], out[16:], cam, lf


def expected_block(pair, cam, lf):
    O = cam[0:3]
    root = np.concatenate([pair[0:3] - O, pair[4:7] - O, pair[8:11] - O, pair[12:15] - O])
    light = np.array([O[1] + lf[0], O[0] + lf[1], O[2] + lf[2], O[1] + lf[3]], np.float32)
    return np.concatenate([root, light, cam[6:9] - cam[3:6], cam[9:12] - cam[3:6]]).astype(np.float32)


CAMERA_2 = ((1.5, 0.7, -3.0), (0.2, -0.1, 2.0))


def rigid(angle_y, t):
    c, s = np.float32(np.cos(np.float32(angle_y))), np.float32(np.sin(np.float32(angle_y)))
    m = np.eye(4, dtype=np.float32)
    m[0, 0] = c; m[0, 2] = s; m[2, 0] = -s; m[2, 2] = c; m[:3, 3] = t
    return m


def three_steps(crt, orc, xml, kind, W, H, frames, stats):
    """upload, a camera change, a write of the root boxes (FileScene: a vertex refit; two-level: a transform update that rebuilds the TLAS) on ONE context; after each
    step the block is what numpy makes of the Scene's fields and the render is the oracle's, accumulator and counters"""
    from test_oracle_pinning import deform
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    o, _ = orc.load_scene(scene_path(xml), kind, ASSETS)
    o.renderer_init(W, H)
    ctx = crt.Context(W, H, collect_stats=stats, max_frames_per_launch=4096)
    blocks = []

    def check(step):
        pair, block, cam, lf = primary_block(ctx)
        assert block.tobytes() == expected_block(pair, cam, lf).tobytes(), step
        blocks.append((pair.copy(), block.copy()))
        ctx.clear(); ctx.reset_counters(); o.clear(); o.reset_counters()
        ctx.render(1, frames, 1); o.render(frames, 4)
        assert np.array_equal(ctx.accumulator(), o.accumulator()), step
        got, want = ctx.counters(), o.counters()
        if stats: assert got == want, step
        else: assert got["rays"] == want["rays"] and got["primary"] == want["primary"], step

    hs.upload(ctx)
    check("upload")
    ctx.set_camera_state(*CAMERA_2); o.set_camera_state(*CAMERA_2)
    check("camera")
    if kind == 0:
        t = hs.bvh(0)["tris"]
        moved = deform(np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1)) + np.float32(0.25)
        hs.move_and_refit(0, moved); o.move_and_refit(0, moved)
        hs.update(ctx, crt.UPDATE_BOUNDS)
    else:
        T0 = hs.blas_transform(1)[0].reshape(4, 4)
        T = rigid(0.4, T0[:3, 3] + np.array([0.9, 0.4, -0.6], np.float32))
        hs.set_transform(1, T); o.set_transform(1, T)
        hs.update(ctx, crt.UPDATE_TRANSFORMS)
    check("root boxes")
    assert not np.array_equal(blocks[0][1], blocks[1][1])                 # the camera moved: every camera-relative value with it
    assert not np.array_equal(blocks[1][0], blocks[2][0]) and not np.array_equal(blocks[1][1][:12], blocks[2][1][:12])      # the root pair moved, and its differences
    ctx.close()


@pytest.mark.parametrize("xml,kind,W,H", [("cube_scene.xml", 0, 32, 32), ("tlas_scene.xml", 1, 48, 32)])
def test_camera_relative_block_is_never_stale(crt, orc, monkeypatch, xml, kind, W, H):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")
    three_steps(crt, orc, xml, kind, W, H, 130, True)                     # 130 frames: 128 slots + the refill path


def test_camera_relative_block_with_the_tiles_kernel(crt, orc, monkeypatch):
    monkeypatch.setenv("CRT_RENDER_KERNEL", "tiles")
    three_steps(crt, orc, "cube_scene.xml", 0, 32, 32, 130, True)


def test_record_pieces_at_the_largest_offsets(crt, orc, monkeypatch):
    """the watch-tower scene (a textured multi-material mesh): node, triangle and shading records of another geometry buffer through the immediate-offset loads"""
    monkeypatch.setenv("CRT_RENDER_KERNEL", "pool_always")
    W, H, frames = 64, 48, 130
    xml = scene_path("tower_scene.xml")
    hs = crt.HostScene(xml, 0, ASSETS)
    ctx = crt.Context(W, H, max_frames_per_launch=4096)
    hs.upload(ctx)
    ctx.render(1, frames, 1)
    acc = ctx.accumulator()
    tm = ctx.timing()
    assert tm["pool_launches"] == 1
    o, _ = orc.load_scene(xml, 0, ASSETS)
    o.renderer_init(W, H)
    o.render(frames, 4)
    assert np.array_equal(acc, o.accumulator())
    got, want = ctx.counters(), o.counters()
    assert got["rays"] == want["rays"] and got["primary"] == want["primary"] and got["mesh_hits"] == want["mesh_hits"]
