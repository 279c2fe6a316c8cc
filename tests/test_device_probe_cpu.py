"""The CPU half of the device probe (tests/test_gpu_device_probe.py holds the device to these expectations bit for bit):
  1. orc_probe_expected is the oracle's own functions: it agrees with the scalar entries that exist, and with plain numpy where the operation is IEEE arithmetic;
  2. over the probe's inputs (L32, A2) the oracle's expf / acosf / atan2f stay within the bounds test_deterministic_math_accuracy sets against float64;
  3. the degenerate-ray families of the primitive scene take every listed branch of Cube / Torus / wall arithmetic at least 100 times, so the GPU comparison of
     test_degenerate_rays_through_identity_transforms cannot pass vacuously."""
import ctypes as C

import numpy as np

import probe_inputs as pi
from conftest import ASSETS


def test_probe_expected_is_the_scalar_entries(orc):
    L = orc.lib()
    acos64, cos64 = orc.det_acos_cos()
    x = np.concatenate([pi.lattice32()[::8192], pi.around32(pi.EXPF_CONSTANTS + pi.ACOSF_CONSTANTS, 8), pi.f32(pi.SPECIALS32)])
    assert 2000 < len(x) < 4000
    for op, fn in (("EXPF", L.orc_expf), ("ACOSF", L.orc_acosf)):
        got = orc.probe_expected(op, x).view(np.float32)[:, 0]
        assert pi.same_bits(got, np.array([fn(float(v)) for v in x], np.float32)), op
    ax = pi.a2_axis()[::71]
    yx = np.stack(np.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)
    yx = np.concatenate([yx, pi.atan2_threshold_pairs()[::9]]).astype(np.float32)
    got = orc.probe_expected("ATAN2F", yx).view(np.float32)[:, 0]
    assert pi.same_bits(got, np.array([L.orc_atan2f(float(p), float(q)) for p, q in yx], np.float32))
    for op, fn in (("ACOS64", acos64), ("COS64", cos64)):
        d = np.concatenate([pi.l64(op)[::2000], pi.high_word_neighbours()])
        got = orc.probe_expected(op, d).view(np.float64)[:, 0]
        assert pi.same_bits64(got, np.array([fn(float(v)) for v in d], np.float64)), op
    bases = pi.rng_bases()[::16]
    got = orc.probe_expected("RNG", bases)
    for b, row in zip(bases[:400], got[:400]):
        s = C.c_uint32(L.orc_init_seed(int(b)))
        assert s.value == row[0]
        draws = np.array([L.orc_random_uint(C.byref(s)) for _ in range(16)], np.uint32)
        f = draws.astype(np.float32) * np.float32(2.3283064365387e-10)
        f[8:] = f[8:] * np.float32(2) - np.float32(1)
        assert np.array_equal(f.view(np.uint32), row[1:17]) and s.value == row[17]
    assert np.array_equal(got, pi.rng_expected(bases))                      # the numpy statement the GPU test uses


def test_probe_expected_ieee_ops_are_numpy(orc):
    """SQRTF / DIVF / SQRT64 / DIV64 / F64TOF32: the device is held to numpy (correctly rounded IEEE); the oracle's C loop must say the same"""
    x = np.concatenate([pi.lattice32()[::64], pi.f32(pi.SPECIALS32)])
    with np.errstate(all="ignore"):
        assert pi.same_bits(orc.probe_expected("SQRTF", x).view(np.float32)[:, 0], np.sqrt(x))
        ab = np.stack([x, np.roll(x, 4099)], 1)
        assert pi.same_bits(orc.probe_expected("DIVF", ab).view(np.float32)[:, 0], ab[:, 0] / ab[:, 1])
        d = pi.sqrt64_inputs()
        assert pi.same_bits64(orc.probe_expected("SQRT64", d).view(np.float64)[:, 0], np.sqrt(d))
        q = pi.div64_inputs()
        assert pi.same_bits64(orc.probe_expected("DIV64", q).view(np.float64)[:, 0], q[:, 0] / q[:, 1])
        c = pi.f64tof32_inputs()
        assert pi.same_bits(orc.probe_expected("F64TOF32", c).view(np.float32)[:, 0], c.astype(np.float32))


def _ulps(got, want):
    want32 = want.astype(np.float32)
    sp = np.spacing(np.abs(want32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want) / np.maximum(sp, 1e-45)


def test_oracle_accuracy_over_the_probe_inputs(orc):
    """the bounds of test_deterministic_math_accuracy (2.0 ulp, 6e-7, 6e-7), over L32 and A2 instead of 6 000 random points.
    Measured maxima: expf 0.954 ulp, acosf 3.04e-7, atan2f 2.49e-7."""
    x = pi.l32(pi.EXPF_CONSTANTS)
    x = x[(x > np.float32(-103.9)) & (x < np.float32(88.7))]
    e = orc.probe_expected("EXPF", x).view(np.float32)[:, 0]
    with np.errstate(all="ignore"):
        worst = float(_ulps(e, np.exp(x.astype(np.float64))).max())
    print("expf: %d arguments, max error %.4f ulp" % (len(x), worst))
    assert worst <= 2.0
    x = pi.l32(pi.ACOSF_CONSTANTS)
    x = x[(x >= -1) & (x <= 1)]
    a = orc.probe_expected("ACOSF", x).view(np.float32)[:, 0]
    worst = float(np.abs(a.astype(np.float64) - np.arccos(x.astype(np.float64))).max())
    print("acosf: %d arguments, max error %.4g" % (len(x), worst))
    assert worst <= 6e-7
    yx = np.concatenate([pi.a2_pairs(), pi.atan2_threshold_pairs()])
    yx = yx[np.isfinite(yx).all(axis=1) & ((yx[:, 0] != 0) | (yx[:, 1] != 0))]
    a = orc.probe_expected("ATAN2F", yx).view(np.float32)[:, 0]
    worst = float(np.abs(a.astype(np.float64) - np.arctan2(yx[:, 0].astype(np.float64), yx[:, 1].astype(np.float64))).max())
    print("atan2f: %d pairs, max error %.4g" % (len(yx), worst))
    assert worst <= 6e-7


def test_degenerate_ray_families_take_every_branch(orc):
    o = orc.primitive_scene(ASSETS, 0.0)
    orc.prim_set_state(o, pi.identity_transforms(orc.prim_state(o)))
    assert np.array_equal(orc.prim_state(o)[32:96].reshape(4, 16), np.tile(np.eye(4, dtype=np.float32).reshape(16), (4, 1)))
    O, D = pi.prim_rays()
    total = {k: 0 for k in orc.PRIM_COVERAGE}
    for t in (0.0, 1.3):                                       # SetTime moves the light quad and the ball only: the cube / torus / wall counts are per pass
        orc.prim_set_time(o, t)
        orc.prim_set_state(o, pi.identity_transforms(orc.prim_state(o)))
        orc.prim_coverage(o, reset=True)
        g = o.find_nearest(O, D)
        cov = orc.prim_coverage(o)
        assert cov["t_nan"] == int(np.isnan(g["t"]).sum())
        assert cov["torus_nearest_po_pos"] + cov["torus_nearest_po_neg"] == int((g["objIdx"] == 10).sum())
        for k in total:
            total[k] += cov[k]
    print("branch counts over both times:", total)
    assert all(v >= 100 for v in total.values()), total
    # the existing test's kind of ray never gets there (the reason these families exist)
    rng = np.random.default_rng(11)
    Or = np.stack([rng.uniform(-2.8, 2.8, 2000), rng.uniform(-0.9, 1.9, 2000), rng.uniform(-2.8, 3.8, 2000)], 1).astype(np.float32)
    Dr = rng.normal(size=(2000, 3)).astype(np.float32)
    orc.prim_set_time(o, 0.0)
    orc.prim_coverage(o, reset=True); o.find_nearest(Or, Dr); cov = orc.prim_coverage(o, reset=True)
    assert cov["cube_nan"] == 0 and cov["t_nan"] == 0
