"""The CPU oracle against closed-form ground truth (tests/analytic_truth.py): the expectation of the reference's estimator on scenes small enough to have one, and
the PrimitiveScene's analytic nearest hit.  The GPU kernels return the oracle's bits (the rest of the suite), so what holds here holds there; the kernels are held
to the same truth directly in tests/test_gpu_analytic_truth.py.  Every statistical bound is analytic_truth's z criterion with sigma from the truth."""
import numpy as np
import pytest

import analytic_truth as at
import render_looks_inputs as li
from conftest import ASSETS
from test_gpu_golden_and_edges import write_scene
from test_gpu_primitive_scene import _rays


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    return at.write_scenes(tmp_path_factory.mktemp("truth"), write_scene)


@pytest.fixture(scope="module")
def sky(orc):
    return orc.read_image(ASSETS + "/sky_gradient.png")


@pytest.fixture(scope="module")
def flat_sky(orc, scenes):
    import os
    return orc.read_image(os.path.join(os.path.dirname(scenes["S0"]), "sky.tga"))


def oracle(orc, xml, kind, depth_limit=5):
    o, _ = orc.load_scene(xml, kind, ASSETS)
    o.renderer_init(at.W, at.H); o.set_params(depth_limit, 1)
    return o


def test_form_factor_equals_the_brute_force_quadrature():
    pts = list(at.FLOOR_POINTS) + [[1.2, 2.0, 0.5], [0.9, 1.5, 0.2], [-4.0, -1.0, 6.0]]           # h = 4, 1, 1.5, 4
    for P in pts:
        assert abs(float(at.form_factor(np.asarray(P), at.QUAD)) - at.form_factor_quadrature(P, at.QUAD)) <= 1e-6, P
    # and the second-moment integrand against the same kind of grid
    x = (np.arange(400) + 0.5) / 400 - 0.5
    for P in at.FLOOR_POINTS:
        dx, dz, h = at.QUAD[0][0] + x - P[0], at.QUAD[0][2] + x - P[2], at.QUAD[0][1] - P[1]
        brute = (h ** 3 / (dx[:, None] ** 2 + dz[None, :] ** 2 + h * h) ** 2.5).sum() / 400 ** 2
        assert abs(float(at.cos2_solid_angle(P, at.QUAD)) - brute) <= 1e-6


def test_constant_textures_come_back_as_one_colour(crt, orc, scenes, tmp_path):
    import os
    d = os.path.dirname(scenes["S0"])
    for name, rgb in (("floor.tga", at.FLOOR_RGB), ("sky.tga", at.SKY_RGB), ("mat.tga", at.MAT_RGB), ("mir.tga", at.MIRROR_RGB)):
        a = orc.read_image(os.path.join(d, name))
        assert a.shape[2] == 3 and (a == np.asarray(rgb, np.uint8)).all(), name
        b = crt.load_image(os.path.join(d, name))
        assert (b == (rgb[0] << 16) + (rgb[1] << 8) + rgb[2]).all(), name        # the host front's loader: packed 0x00RRGGBB
    for xml in scenes.values():
        crt.HostScene(xml, 0, ASSETS).close()                              # the host front reads every scene


@pytest.mark.parametrize("k", [0, 1, 2])
def test_floor_point(orc, scenes, k):
    o = oracle(orc, scenes["S0"], 0)
    O, D, mean, second, seeds = at.floor_case(k)
    h = o.find_nearest(O, D)
    assert h["objIdx"][0] == 1 and abs(float(h["t"][0]) - np.linalg.norm(at.FLOOR_POINTS[k] - at.EYE)) <= 1e-5
    check = at.check_mean(at.oracle_samples(o, O, D, seeds), mean, second, "floor point %d" % k)
    assert np.abs(check).max() <= at.Z


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("depth_limit", [1, 3, 5])
def test_slab(orc, scenes, depth_limit, kind):
    o = oracle(orc, scenes["S2"], kind, depth_limit)
    O, D, want, phys, seeds, thickness, t0 = at.slab_case(depth_limit)
    b = at.Box(**at.SLAB)
    assert np.abs(b.R.T[at.SLAB_AXIS] - b.R[at.SLAB_AXIS]).max() <= 1e-12          # a half turn: model.cpp:70's transposed normal is the face's own
    along = b.corners() @ b.R[:, at.SLAB_AXIS]                                      # cube.obj's eight corners, transformed here: two face planes
    assert abs((along.max() - along.min()) - thickness) <= 1e-6 and abs(thickness - 1.0) <= 1e-6       # the ray itself is float32
    h = o.find_nearest(O, D)
    assert h["objIdx"][0] == 2 and abs(float(h["t"][0]) - t0) <= 1e-5
    # what the recursion assumes about the ways out: backwards nothing, forwards the mirror's top face, whose reflection meets nothing
    n = b.R[:, at.SLAB_AXIS]
    far = b.c + (0.5 + at.EPSILON) * n
    assert o.find_nearest(b.c - (0.5 + at.EPSILON) * n, -n)["objIdx"][0] == -1
    hb = o.find_nearest(far, n)
    assert hb["objIdx"][0] == 3
    I = far + float(hb["t"][0]) * n
    assert abs(I[1] - (at.BEHIND["position"][1] + at.BEHIND["scale"][1])) <= 1e-5
    assert o.find_nearest(I + at.EPSILON * n * [1, -1, 1], n * [1, -1, 1])["objIdx"][0] == -1
    at.check_slab(at.oracle_samples(o, O, D, seeds), depth_limit, "slab, depth limit %d, kind %d" % (depth_limit, kind))


@pytest.mark.parametrize("kind", [0, 1])
def test_mirror(orc, scenes, sky, kind):
    o = oracle(orc, scenes["S1"], kind)
    O, D, want, axis, other = at.mirror_case(kind, sky)
    side = axis != 1
    assert (~side).sum() >= 100 and side.sum() >= 100, np.bincount(axis)       # the top face, and side faces (whose normal the scene kind decides)
    # the contrast: with the other kind's normal (model.cpp:70 against blas_bvh.cpp:397) these rays would show other texels, by a thousand tolerances
    differs = np.abs(other - want).max(axis=1) > 1e-3
    assert differs[side].sum() >= 50 and differs[~side].sum() >= 50, (differs[side].sum(), differs[~side].sum())
    got = np.stack([o.sample(O[i], D[i], 1 + i)[0] for i in range(len(O))])
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-3)
    print("mirror kind %d: %d rays, %d on side faces, largest relative error %.2e" % (kind, len(O), side.sum(), err.max()))
    assert err.max() <= 1e-6


def test_render_of_the_floor(orc, scenes, flat_sky):
    o = oracle(orc, scenes["S0"], 0)
    o.render(at.FRAMES, 8)
    at.check_render(o.accumulator(), at.FRAMES, flat_sky, "oracle")


def test_light_pixels(orc, scenes):
    o = oracle(orc, scenes["S0"], 0)
    o.set_camera_state(*at.LIGHT_CAMERA)
    cam = at.camera_state(at.LIGHT_CAMERA[0], at.LIGHT_CAMERA[1], at.W, at.H)
    for got, want in zip(o.camera(), cam):
        assert np.abs(got - want).max() <= 1e-5
    o.render(at.LIGHT_FRAMES, 8)
    at.check_light_pixels(o.accumulator(), at.LIGHT_FRAMES, "oracle")


@pytest.mark.parametrize("scene,kind", [("S0", 0), ("S1", 0), ("S1", 1)])
def test_whitted_floor(orc, scenes, scene, kind):
    o = oracle(orc, scenes[scene], kind)
    o.whitted(4)
    at.check_whitted(o.accumulator(), [at.Box(**at.MIRROR)] if scene == "S1" else [], "whitted %s kind %d" % (scene, kind), shadow=scene == "S1")


@pytest.mark.parametrize("t", [0.0, 1.3, 7.77])
def test_primitive_scene(orc, t):
    O, D = _rays(20000, 11)
    o = orc.primitive_scene(ASSETS, t)
    g = o.find_nearest(O, D)
    tw, iw, margin = at.prim_truth(O, D, t)
    seen = at.prim_check(g["t"], g["objIdx"], tw, iw, margin)
    print("t = %s: %d rays under the margin; observed |dt| %s" % (t, (margin < at.NEAR).sum(), {k: "%.3g" % v for k, v in seen.items()}))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the light quad of a look: turned, resized (analytic_truth.QUAD_LOOKS)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
RHO, L_SKY = at.texel_rgb(at.FLOOR_RGB), at.texel_rgb(at.SKY_RGB)


def look_oracle(orc, xml, name):
    o = oracle(orc, xml, 0)
    T, half = at.look_cells(name)
    o.set_light_quad(T, li.inverse_no_scale(T), half)
    return o


def test_quad_looks_are_the_look_tests_transforms():
    tr = li.transforms(np.asarray(at.LIGHT_POS, np.float32))
    for name, key in (("zyx", "zyx"), ("z25", "z25"), ("half_x", "half_x"), ("zyx_size_0.9", "zyx")):
        assert np.array_equal(at.look_cells(name)[0].reshape(4, 4), tr[key]), name
    assert np.array_equal(at.look_cells("size_0.9")[0].reshape(4, 4), li.translate(np.asarray(at.LIGHT_POS, np.float32)))


def test_general_quad_truth_checks_itself():
    """the general forms come to the parallel ones (1e-12), and Lambert's contour formula to the 400 x 400 midpoint quadrature (1e-6), for every look and point"""
    pts = list(at.QUAD_FLOOR_POINTS) + [[1.2, 2.0, 0.5], [-4.0, -1.0, 6.0]]
    same = (at.QUAD[0], np.eye(3), at.QUAD[1])
    for P in pts:
        P = np.asarray(P)
        assert abs(float(at.cos2_solid_angle(P, same)) - float(at.cos2_solid_angle_parallel(P, at.QUAD))) <= 1e-12
        assert abs(float(at.form_factor(P, same)) - float(at.form_factor(P, at.QUAD))) <= 1e-12
        m1, s1 = at.floor_radiance(P, RHO, L_SKY, same); m0, s0 = at.floor_radiance(P, RHO, L_SKY, at.QUAD)
        assert np.abs(m1 - m0).max() <= 1e-12 and np.abs(s1 - s0).max() <= 1e-12
    n = 400; u = ((np.arange(n) + 0.5) / n * 2 - 1)
    for name in at.QUAD_LOOKS:
        q = at.look_quad(name); c, R, h = q
        assert (at.quad_corners(q)[:, 1] > at.FLOOR_Y + 1.0).all()            # wholly above the floor
        for P in at.QUAD_FLOOR_POINTS:
            assert abs(float(at.form_factor(P, q)) - at.form_factor_quadrature(P, q)) <= 1e-6, (name, P)
            d = c + (u * h)[:, None, None] * R[:, 0] + (u * h)[None, :, None] * R[:, 2] - P
            r2 = (d * d).sum(-1)
            brute = (d[..., 1] ** 2 * np.abs(d @ R[:, 1]) / r2 ** 2.5).sum() * (2 * h / n) ** 2
            assert abs(float(at.cos2_solid_angle(P, q)) - brute) <= 1e-6, (name, P)
    # the figures the cases were chosen by: under zyx the two points either side of the centre tell R from its transpose, the point under it cannot
    m = [at.floor_radiance(P, RHO, L_SKY, at.look_quad("zyx"))[0][0] for P in at.QUAD_FLOOR_POINTS[[3, 4, 0]]]
    c, R, h = at.look_quad("zyx")
    mt = [at.floor_radiance(P, RHO, L_SKY, (c, R.T, h))[0][0] for P in at.QUAD_FLOOR_POINTS[[3, 4, 0]]]
    assert np.allclose(m, [0.5248, 0.4152, 0.5071], atol=5e-5) and np.allclose(mt, [0.4374, 0.5037, 0.5071], atol=5e-5), (m, mt)


def test_wrong_quad_models_lie_outside_the_band():
    """negative controls: each wrong model's truth lies beyond the right one's Z = 5 band by at least twice the band (three bands from the right mean), on some
    channel, at two or more floor points of a look that is tested; the Whitted control against check_whitted's bound in the same way"""
    def far_points(name, wrong):
        q = at.look_quad(name); k = 0
        for P in at.QUAD_FLOOR_POINTS:
            m, s2 = at.floor_radiance(P, RHO, L_SKY, q)
            band = at.Z * np.sqrt(s2 - m * m) / np.sqrt(at.N_FLOOR)
            assert (band <= 0.025 * m).all()                                  # 2.4 % of the mean at most
            k += bool((np.abs(wrong(P, q) - m) >= 3 * band).any())
        return k
    transposed = lambda P, q: at.floor_radiance(P, RHO, L_SKY, (q[0], q[1].T, q[2]))[0]      # noqa: E731
    no_size = lambda P, q: at.floor_radiance(P, RHO, L_SKY, (q[0], q[1], 0.5))[0]            # noqa: E731
    one_face = lambda P, q: at.floor_radiance(P, RHO, L_SKY, q, one_face=True)[0]            # noqa: E731
    assert far_points("zyx", transposed) >= 2 and far_points("z25", transposed) >= 2 and far_points("zyx_size_0.9", transposed) >= 2
    assert far_points("size_0.9", no_size) == 5 and far_points("zyx_size_0.9", no_size) == 5
    assert far_points("half_x", one_face) == 5
    for name in ("zyx", "z25", "half_x", "zyx_size_0.9"):
        q = at.look_quad(name)
        d = [np.abs(at.whitted_floor(P, RHO, q, along_normal=True)[0] - at.whitted_floor(P, RHO, q)[0]).max() for P in at.QUAD_FLOOR_POINTS]
        assert sum(x >= 3 * at.WHITTED_QUAD_TOL for x in d) >= 2, (name, d)


@pytest.mark.parametrize("name", sorted(at.QUAD_LOOKS))
def test_floor_points_and_whitted_under_a_quad_look(orc, scenes, name):
    """the oracle with set_light_quad against the expectation: Sample at the two floor points either side of the centre (the GPU module takes all five), and the
    Whitted image of the floor"""
    o = look_oracle(orc, scenes["S0"], name)
    q = at.look_quad(name)
    for k in (3, 4):
        O, D, mean, second, seeds = at.floor_case(k, q, salt=sorted(at.QUAD_LOOKS).index(name))
        assert o.find_nearest(O, D)["objIdx"][0] == 1
        at.check_mean(at.oracle_samples(o, O, D, seeds), mean, second, "%s, floor point %d" % (name, k))
    o.whitted(4)
    at.check_whitted(o.accumulator(), [], "whitted under %s" % name, shadow=name == "z25", quad=q, tol=at.WHITTED_QUAD_TOL)     # (z25: far floor lies behind the tilted quad's plane)


def test_render_and_light_pixels_under_quad_looks(orc, scenes, flat_sky):
    """ProcessTile's floor-tile means under every look, and the ring of pixels that see the 0.9 quad but not the 0.5 quad: exactly the light's colour"""
    for name in sorted(at.QUAD_LOOKS):
        o = look_oracle(orc, scenes["S0"], name)
        o.render(at.FRAMES, 8)
        at.check_render(o.accumulator(), at.FRAMES, flat_sky, "render under %s" % name, quad=at.look_quad(name), key=name)
    o = look_oracle(orc, scenes["S0"], "size_0.9")
    o.set_camera_state(*at.LIGHT_CAMERA); o.render(at.LIGHT_FRAMES, 8)
    ring = at.check_light_pixels(o.accumulator(), at.LIGHT_FRAMES, "ring", quad=(at.QUAD[0], 0.9), beyond=at.QUAD)
    assert ring >= 200
    plain = oracle(orc, scenes["S0"], 0)
    plain.set_camera_state(*at.LIGHT_CAMERA); plain.render(at.LIGHT_FRAMES, 8)
    with pytest.raises(AssertionError):                                     # the 0.5 quad leaves the ring to the sky
        at.check_light_pixels(plain.accumulator(), at.LIGHT_FRAMES, "ring without the size", quad=(at.QUAD[0], 0.9), beyond=at.QUAD)
