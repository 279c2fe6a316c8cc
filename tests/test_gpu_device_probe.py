"""Every numeric building block of the device code, by itself, against the same formula evaluated on the CPU — bit for bit (any NaN equals any NaN).
dev_common.h promises "only IEEE + - * / sqrt, so results are bit-identical with a scalar CPU evaluation of the same expressions"; the renders check that through
whole paths, test_gpu_reciprocal.py checks the short reciprocals, and this file checks the rest through the probe the library ships (crt_debug_device_probe:
device/probe.hip for fp32, the end of device/render_prim.hip for the torus' fp64 chain) at the inputs where each block can go wrong.  The expectation is the
oracle's restatement (orc_probe_expected), plain numpy where the operation is IEEE arithmetic or the integer generator, and for normalize / cross / dot the
committed outputs of the real reference (tests/golden/ref_math.npz).  The float64 accuracy of the oracle's side is asserted in test_device_probe_cpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import probe_inputs as pi
from conftest import ASSETS, GOLDEN, scene_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(crt):
    c = crt.Context(64, 64)
    c.L.crt_debug_device_probe.restype = C.c_int
    c.L.crt_debug_device_probe.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32]
    return c


@pytest.fixture(scope="module")
def bunny(crt):
    return crt.HostScene(scene_path("bunny_scene.xml"), crt.SCENE_FILE, ASSETS).bvh(0)


def device(ctx, orc, op, inputs):
    """crt_debug_device_probe over [n, input words] records, in chunks of 2^25; returns [n, output words] uint32"""
    num, wi, wo = orc.PROBE_OPS[op]
    a = np.ascontiguousarray(inputs)
    a = a.reshape(len(a), -1)
    assert a.shape[1] * a.itemsize == wi * 4, (op, a.shape, a.dtype)
    out = np.zeros((len(a), wo), np.uint32)
    for s in range(0, len(a), pi.CHUNK):
        part, res = a[s:s + pi.CHUNK], out[s:s + pi.CHUNK]
        r = ctx.L.crt_debug_device_probe(ctx.h, num, part.ctypes.data, res.ctypes.data, len(part))
        assert r == 0, (op, r, ctx.L.crt_last_error(ctx.h))
    return out


def check(op, inputs, got, want, dtype=np.float32):
    """got == want by the shared rule; on failure the first differing records with both results in hex"""
    got = np.ascontiguousarray(got).view(dtype).reshape(len(got), -1); want = np.ascontiguousarray(want).view(dtype).reshape(len(want), -1)
    bad = pi.differing(got, want)
    if len(bad):
        raw = np.ascontiguousarray(inputs).reshape(len(got), -1)
        hexes = lambda v: " ".join("%0*x" % (2 * v.itemsize, int(w)) for w in v.view(np.uint64 if v.itemsize == 8 else np.uint32).ravel())
        lines = ["%s: %d of %d records differ" % (op, len(bad), len(got))]
        for i in bad[:8]:
            lines.append("  #%d in %s (%s)\n      device %s\n      expect %s" % (i, hexes(raw[i]), raw[i], hexes(got[i]), hexes(want[i])))
        pytest.fail("\n".join(lines))


def against_oracle(ctx, orc, op, inputs, dtype=np.float32):
    got = device(ctx, orc, op, inputs); want = orc.probe_expected(op, inputs)
    check(op, inputs, got, want, dtype)
    return got


def test_expf(ctx, orc):
    x = pi.l32(pi.EXPF_CONSTANTS)
    got = against_oracle(ctx, orc, "EXPF", x).view(np.float32)[:, 0]
    assert np.isinf(got).any() and (got == 0).any() and ((got > 0) & (got < 1e-38)).any()          # both guards and the denormal results were reached


def test_acosf(ctx, orc):
    against_oracle(ctx, orc, "ACOSF", pi.l32(pi.ACOSF_CONSTANTS))


def test_atan2f(ctx, orc):
    yx = np.concatenate([pi.a2_pairs(), pi.atan2_threshold_pairs()])
    with np.errstate(all="ignore"):
        q = np.abs(yx[::97, 0] / yx[::97, 1])
    assert ((q > 0) & (q < 1e-38)).any()                                  # denormal quotients ay / ax are in the grid
    against_oracle(ctx, orc, "ATAN2F", yx)


def test_sqrtf(ctx, orc):
    x = np.concatenate([pi.lattice32(), pi.f32(pi.SPECIALS32)])
    with np.errstate(all="ignore"):
        check("SQRTF", x, device(ctx, orc, "SQRTF", x), np.sqrt(x))


def test_divf(ctx, orc):
    x = np.concatenate([pi.lattice32(), pi.f32(pi.SPECIALS32)])
    ax = pi.a2_axis()[::3]
    ab = np.concatenate([np.stack([x[::4], np.roll(x, 4099)[::4]], 1), np.stack(np.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)]).astype(np.float32)
    with np.errstate(all="ignore"):
        check("DIVF", ab, device(ctx, orc, "DIVF", ab), ab[:, 0] / ab[:, 1])


def test_vec3_meets_the_reference_golden(ctx, orc):
    """the third `who` of test_tmplmath_inlines_match_reference_golden: the device, which alone computes normalize as rcp_exact(sqrtf(..))"""
    z = np.load(os.path.join(GOLDEN, "ref_math.npz"))
    rows = np.ascontiguousarray(z["inputs"][:, :6], np.float32)
    want = np.concatenate([z["outputs"][:, 0:3], z["outputs"][:, 6:9], z["outputs"][:, 9:10]], 1)         # normalize, cross, dot
    check("VEC3 (reference golden)", rows, device(ctx, orc, "VEC3", rows), want)
    against_oracle(ctx, orc, "VEC3", pi.vec3_edge_rows())


def test_rng(ctx, orc):
    bases = pi.rng_bases()
    check("RNG", bases, device(ctx, orc, "RNG", bases), pi.rng_expected(bases), np.uint32)


def test_tex_index(ctx, orc):
    r = pi.tex_records()
    got = against_oracle(ctx, orc, "TEX", r, np.uint32)[:, 0]
    assert (got < r[:, 2] * r[:, 3]).all()


def test_sky_lookup(ctx, orc):
    r = pi.sky_records()
    got = against_oracle(ctx, orc, "SKY", r)                             # phi, theta as floats (NaN rule); the index words are compared by the same view exactly
    assert (got[:, 2] < r[:, 3] * r[:, 4]).all()


def test_box_fast_and_box_exact(ctx, orc, bunny):
    r = pi.box_records(bunny["nodes"])
    first = orc.probe_expected("BOX", r).view(np.float32)[:, 0]
    hit = first != np.float32(1e30)
    again = r[hit].copy(); again[:, 12] = first[hit]                      # tray exactly the returned tmin: the strict `tmin < tray` rejects
    r = np.concatenate([r, again])
    got = device(ctx, orc, "BOX", r).view(np.float32); want = orc.probe_expected("BOX", r).view(np.float32)
    assert (want[len(r) - len(again):, 0] == np.float32(1e30)).all() and hit.sum() > 10000 and (~hit).sum() > 10000
    check("BOX box_exact", r, got[:, 0:1], want[:, 0:1])
    finite = np.isfinite(r[:, 9:12]).all(axis=1)
    assert finite.sum() > 10000 and (~finite).sum() > 10000
    gf, wf = got[finite], want[finite]
    bad = np.flatnonzero((gf[:, 1] != gf[:, 0]) | (gf[:, 1] != wf[:, 0]))           # as float values: zeros of either sign are equal; no result is a NaN
    assert not np.isnan(wf).any()
    assert len(bad) == 0, "box_fast differs from box_exact / the oracle where all reciprocals are finite: first records %s -> device %s, oracle %s" % (
        r[finite][bad[:4]].view(np.uint32), gf[bad[:4]].view(np.uint32), wf[bad[:4], 0].view(np.uint32))


def test_hit_tri(ctx, orc, bunny):
    """the device record holds e1 = v1 - v0 and e2 = v2 - v0, one float32 subtraction each: exactly what crt_upload_scene's flattening stores (abi.cpp,
    `lt.e1[k] = t.vertex1[k] - t.vertex0[k]`) and what the oracle's triangle test forms from the vertices"""
    tris = bunny["tris"][::5]
    r = pi.tri_records(tris)
    first = orc.probe_expected("TRI", r)
    acc = first[:, 3] == 1
    again = r[acc].copy(); again[:, 15] = first[acc, 0].view(np.float32)                # t_in exactly the t of the first pass: the strict `t < h.t` rejects
    above = r[acc].copy(); above[:, 15] = np.nextafter(first[acc, 0].view(np.float32), np.float32(np.inf))
    r = np.concatenate([r, again, above])
    want = orc.probe_expected("TRI", r)
    n1, n2 = len(first), len(first) + len(again)
    assert (want[n1:n2, 3] == 0).all() and (want[n2:, 3] == 1).all()
    u, v = want[:, 1].view(np.float32), want[:, 2].view(np.float32)
    a = want[:, 3] == 1
    assert a.sum() > 20000 and (~a).sum() > 20000
    assert (a & (u == 0)).sum() > 100 and (a & (v == 0)).sum() > 100 and (a & (u + v == 1)).sum() > 100      # hits exactly on the three edges
    check("TRI", r, device(ctx, orc, "TRI", pi.tri_device_records(r)), want)


@pytest.mark.parametrize("op", ["ACOS64", "COS64", "CBRT64"])
def test_torus_fp64_functions(ctx, orc, op):
    against_oracle(ctx, orc, op, pi.l64(op), np.float64)


def test_sqrt64(ctx, orc):
    d = pi.sqrt64_inputs()
    with np.errstate(all="ignore"):
        check("SQRT64", d, device(ctx, orc, "SQRT64", d), np.sqrt(d), np.float64)


def test_div64(ctx, orc):
    q = pi.div64_inputs()
    with np.errstate(all="ignore"):
        check("DIV64", q, device(ctx, orc, "DIV64", q), q[:, 0] / q[:, 1], np.float64)


def test_f64_to_f32(ctx, orc):
    c = pi.f64tof32_inputs()
    with np.errstate(all="ignore"):
        check("F64TOF32", c, device(ctx, orc, "F64TOF32", c), c.astype(np.float32))


def test_probe_refusals(ctx):
    x = np.zeros(16, np.float32); out = np.zeros(64, np.float32)
    probe = ctx.L.crt_debug_device_probe
    assert probe(ctx.h, 17, x.ctypes.data, out.ctypes.data, 1) == -1 and probe(ctx.h, -1, x.ctypes.data, out.ctypes.data, 1) == -1      # unknown op
    assert probe(ctx.h, 0, x.ctypes.data, out.ctypes.data, (1 << 25) + 1) == -1                                                          # before anything is allocated or read
    assert probe(ctx.h, 0, None, out.ctypes.data, 1) == -1 and probe(ctx.h, 0, x.ctypes.data, None, 1) == -1 and probe(None, 0, x.ctypes.data, out.ctypes.data, 1) == -1
    assert probe(ctx.h, 0, x.ctypes.data, out.ctypes.data, 0) == 0
    assert probe(ctx.h, 0, x.ctypes.data, out.ctypes.data, 16) == 0 and (out[:16] == 1.0).all() and (out[16:] == 0).all()
