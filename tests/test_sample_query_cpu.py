"""The premise of tests/test_gpu_sample_query.py, checked with the CPU oracle alone: the ray sets the GPU test feeds crt_sample reach every branch of
Renderer::Sample — per triangle-scene world at least 100 rays whose first hit is a mirror, the dielectric from outside, the dielectric from inside, a diffuse
surface (and the textured mesh), the light, and nothing; at least 100 paths that draw no random number and 100 that draw more than ten."""
import numpy as np
import pytest

import sample_query_inputs as si
from conftest import ASSETS


@pytest.mark.parametrize("world", ["bvh", "kd", "grid", "tlas", "tlas_kd", "tlas_grid"])
def test_triangle_ray_sets_reach_every_branch(orc, tmp_path, world):
    xml = si.scene_xml(tmp_path)
    o, _ = orc.load_scene(xml, 1 if world.startswith("tlas") else 0, ASSETS)
    acc = None
    if world in ("kd", "grid"):
        acc = orc.alt_accel(world, o.bvh(0)["tris"]); orc.set_render_accel(o, acc)
    if world in ("tlas_kd", "tlas_grid"):
        orc.set_blas_accel(o, orc.blas_accels(o, world[5:]))
        O, D, inside, seeds = si.two_level_rays(o, world[5:])
        assert len(O) == si.N_RAYS + 180
    else:
        O, D, inside, seeds = si.triangle_rays(o)
        assert len(O) == si.N_RAYS
    assert (seeds != 0).all() and (seeds >> 31).sum() > 100
    _, out, cnt = si.oracle_sample(o, O, D, inside, seeds)
    c, k = si.assert_branches(o, O, D, inside, seeds, out)
    assert cnt["rays"] > len(O) and cnt["primary"] == 0                                                   # paths longer than one ray
    if acc is not None:
        acc.close()


def test_primitive_ray_set_draws(orc):
    o = orc.primitive_scene(ASSETS, 1.3)
    O, D, inside, seeds = si.prim_rays()
    _, out, cnt = si.oracle_sample(o, O, D, inside, seeds)
    k = si.draws(seeds, out)
    assert (k >= 0).all() and (k == 0).sum() >= 100 and (k > 10).sum() >= 100           # the light quad ends a path at once; the walls are diffuse
    assert cnt["rays"] > len(O) and cnt["primary"] == 0


def test_seed_helpers_restate_the_generator(orc):
    """init_seed / rnd of the inputs module against the oracle's tile seed: one frame of one tile draws through them"""
    import probe_inputs as pi
    bases = np.array([0, 1, 1799, 64 + 1799, 0xffffffff], np.uint32)
    assert np.array_equal(si.init_seed(bases), pi.rng_expected(bases)[:, 0])
    s, r = si.rnd(si.init_seed(bases))
    assert np.array_equal(r.view(np.uint32), pi.rng_expected(bases)[:, 1])
