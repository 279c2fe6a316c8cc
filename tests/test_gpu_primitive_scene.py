"""SURVEY 8(f)4, second half: PrimitiveScene (infra/scene/primitive_scene.cpp + template/primitives.h Sphere / Cube / Quad / Torus) behind crt_find_nearest and
Renderer::Sample.  PARITY UNPINNED: the reference files need MSVC and the reference holds no fixture of this scene; the HIP kernels (render_prim.hip) are checked
bit for bit against the oracle's restatement (oracle/crt_oracle.cpp PrimScene), both using the same deterministic double-precision acos / cos for the torus."""
import numpy as np
import pytest

import probe_inputs as pi
from conftest import ASSETS

pytestmark = pytest.mark.gpu


def _rays(n, seed):
    rng = np.random.default_rng(seed)
    O = np.stack([rng.uniform(-2.8, 2.8, n), rng.uniform(-0.9, 1.9, n), rng.uniform(-2.8, 3.8, n)], axis=1).astype(np.float32)
    D = rng.normal(size=(n, 3)).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True).astype(np.float32)
    # a share aimed at the small objects (bouncing ball, cube, torus) so that every primitive is hit often
    targets = np.array([[-1.8, 0.2, 1.0], [1.8, 0.0, 2.5], [-0.25, 0.0, 2.0], [0.0, 1.7, 2.0]], np.float32)
    k = n // 2
    T = targets[rng.integers(0, len(targets), k)] + rng.normal(scale=0.4, size=(k, 3)).astype(np.float32)
    Dk = T - O[:k]; Dk /= np.linalg.norm(Dk, axis=1, keepdims=True)
    D[:k] = Dk.astype(np.float32)
    return O, D.astype(np.float32)


@pytest.mark.parametrize("t", [0.0, 1.3, 7.77])
def test_find_nearest_over_the_primitives_is_bit_exact(crt, orc, t):
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(t)
    o = orc.primitive_scene(ASSETS, t)
    assert np.array_equal(ps.state().view(np.uint32), orc.prim_state(o).view(np.uint32))     # constructor + SetTime: the same matrices to the bit
    ctx = crt.Context(64, 64); ps.upload(ctx)
    O, D = _rays(20000, 11)
    h = ctx.find_nearest(O, D); g = o.find_nearest(O, D)
    assert np.array_equal(h["objIdx"], g["objIdx"])
    assert np.array_equal(h["t"].view(np.uint32), g["t"].view(np.uint32))
    counts = np.bincount(h["objIdx"] + 1, minlength=12)
    assert (counts[1:] > 20).all(), counts                     # every one of the eleven primitives is the nearest hit of some rays (closed room: no misses)
    assert counts[0] == 0


@pytest.mark.parametrize("t,W,H,frames,passes", [(0.0, 96, 64, 3, 1), (1.3, 64, 48, 70, 1), (5.0, 64, 64, 2, 2)])
def test_path_tracer_over_the_primitive_scene_is_bit_exact(crt, orc, t, W, H, frames, passes):
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(t)
    o = orc.primitive_scene(ASSETS, t); o.renderer_init(W, H); o.set_params(5, passes)
    ctx = crt.Context(W, H); ps.upload(ctx)
    ctx.render(1, frames, passes); o.render(frames, 4)
    got, want = ctx.accumulator(), o.accumulator()
    assert np.isfinite(got).all() and got[..., :3].max() > 1.0
    assert np.abs(got - want).max() / (frames * passes) <= 1e-4      # north_star's tolerance ...
    assert np.array_equal(got, want)                                   # ... and exact: shared deterministic acos / cos, IEEE double otherwise
    assert ctx.counters()["rays"] == o.counters()["rays"]
    # the scene replaces a triangle scene, and a triangle scene replaces it
    with pytest.raises(crt.CrtError):
        ctx.whitted_tick()
    hs = crt.HostScene(ASSETS + "/scenes/cube_scene.xml", 0, ASSETS); hs.upload(ctx)
    ctx.clear(); ctx.render(1, 1, 1); ctx.sync()
    assert ctx.accumulator()[..., :3].max() > 0


@pytest.mark.parametrize("t", [0.0, 1.3])
def test_degenerate_rays_through_identity_transforms(crt, orc, t):
    """The scene as SetTime builds it rotates cube and torus, so no ray has an exact-zero direction component in object space and the edge inputs of the cube,
    the torus' quartic and the walls cannot occur.  Here oracle and device get the same edited description (identity cube / torus transforms) and the ray families
    of probe_inputs.prim_families; test_device_probe_cpu.py asserts that they take every branch (fabs(d1) < 1e-8, NaN slabs, NaN t, ...) at least 100 times."""
    ps = crt.HostPrimitiveScene(ASSETS); ps.set_time(t)
    o = orc.primitive_scene(ASSETS, t)
    state = pi.identity_transforms(ps.state())
    orc.prim_set_state(o, state)
    d = ps.desc_with_state(state)
    ctx = crt.Context(64, 64); ps.upload_desc(ctx, d)
    assert np.array_equal(orc.prim_state(o).view(np.uint32), state.view(np.uint32))
    O, D = pi.prim_rays()
    orc.prim_coverage(o, reset=True)
    h = ctx.find_nearest(O, D); g = o.find_nearest(O, D)
    cov = orc.prim_coverage(o)
    assert cov["d1_tiny"] > 100 and cov["cube_nan"] > 100 and cov["t_nan"] > 100 and cov["swapped"] > 100, cov
    tbad = np.zeros(len(O), bool); tbad[pi.differing(h["t"], g["t"])] = True          # bit equality, any NaN equals any NaN
    bad = np.flatnonzero((h["objIdx"] != g["objIdx"]) | tbad)
    assert len(bad) == 0, "first differing rays: %s" % [(int(i), O[i].tolist(), D[i].tolist(), int(h["objIdx"][i]), int(g["objIdx"][i]),
                                                        "%08x" % h["t"].view(np.uint32)[i], "%08x" % g["t"].view(np.uint32)[i]) for i in bad[:6]]
    assert np.isnan(g["t"]).sum() == cov["t_nan"] and np.array_equal(np.isnan(h["t"]), np.isnan(g["t"]))        # the NaN t of family (h), in the same rays
