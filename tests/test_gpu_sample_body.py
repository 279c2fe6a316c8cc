"""The Sample body (csrc/device/sample_body.h) in the single-BVH instantiations of every render kernel.  No single-BVH scene of assets/scenes has a reflective or
refractive material or an absorbing medium, so the parity tests never run HandleMirror, HandleDielectric and the medium's absorption with KIND == 0.  This scene does:
cube_scene.xml with its material changed to reflectivity 0.3, refractivity 0.4, absorption (0.5, 0.2, 0.1).  32 x 32 pixels = 4 tiles, 130 frames = three windows of
render_tiles_kernel (the last one partial) and, in render_pool_kernel, 128 stream slots per tile and two frames more than slots."""
import numpy as np
import pytest

from conftest import ASSETS, scene_path

pytestmark = pytest.mark.gpu

W, H, FRAMES = 32, 32, 130
MATERIAL = ("<reflectivity>0.0</reflectivity>", "<refractivity>0.0</refractivity>", "<absorption><x>0.0</x><y>0.0</y><z>0.0</z></absorption>")
REFL, REFR, ABSORB = "<reflectivity>0.3</reflectivity>", "<refractivity>0.4</refractivity>", "<absorption><x>0.5</x><y>0.2</y><z>0.1</z></absorption>"


def write_variant(directory, name, refl=REFL, refr=REFR, absorb=ABSORB):
    text = open(scene_path("cube_scene.xml")).read()
    for old, new in zip(MATERIAL, (refl, refr, absorb)):
        assert text.count(old) == 1
        text = text.replace(old, new)
    p = directory / (name + ".xml")
    p.write_text(text)
    return str(p)


def oracle_render(orc, xml, kd=False):
    o, _ = orc.load_scene(xml, 0, ASSETS)
    o.renderer_init(W, H)
    acc = None
    if kd:
        acc = orc.alt_accel("kd", o.bvh(0)["tris"]); orc.set_render_accel(o, acc)
    o.render(FRAMES, 2)
    out = (o.accumulator().copy(), o.counters()["rays"])
    if kd:
        orc.set_render_accel(o, None); acc.close()
    return out


@pytest.fixture(scope="module")
def world(orc, tmp_path_factory):
    """the scene file and the oracle's renders of it, computed once: through the BVH, through its KD-tree, and with each of the three material edits taken back"""
    d = tmp_path_factory.mktemp("sample_body")
    xml = write_variant(d, "glass_cube")
    ref = {"bvh": oracle_render(orc, xml), "kd": oracle_render(orc, xml, kd=True)}
    ref["no_absorption"] = oracle_render(orc, write_variant(d, "no_absorption", absorb=MATERIAL[2]))
    ref["no_reflectivity"] = oracle_render(orc, write_variant(d, "no_reflectivity", refl=MATERIAL[0]))
    ref["no_refractivity"] = oracle_render(orc, write_variant(d, "no_refractivity", refr=MATERIAL[1]))
    return xml, ref


def test_scene_exercises_mirror_dielectric_and_medium(world):
    """on the oracle alone: the image depends on each of the three material edits, so every render below runs the mirror branch, the dielectric branch and the
    absorption inside the cube"""
    _, ref = world
    acc = ref["bvh"][0]
    assert np.isfinite(acc).all()
    for name in ("no_absorption", "no_reflectivity", "no_refractivity"):
        assert not np.array_equal(acc, ref[name][0]), name


@pytest.mark.parametrize("kernel,stats", [("tiles", False), ("tiles", True), ("pool_always", False)])
def test_hot_kernels_match_oracle(crt, monkeypatch, world, kernel, stats):
    xml, ref = world
    monkeypatch.setenv("CRT_RENDER_KERNEL", kernel)
    hs = crt.HostScene(xml, 0, ASSETS)
    ctx = crt.Context(W, H, collect_stats=stats, max_frames_per_launch=4096)
    hs.upload(ctx)
    ctx.render(1, FRAMES, 1)
    assert ctx.timing()["pool_launches"] == (1 if kernel == "pool_always" else 0)
    assert np.array_equal(ctx.accumulator().view(np.uint32), ref["bvh"][0].view(np.uint32))
    assert ctx.counters()["rays"] == ref["bvh"][1]
    ctx.close()


def test_sequential_kernel_through_kdtree_matches_oracle(crt, world):
    xml, ref = world
    hs = crt.HostScene(xml, 0, ASSETS)
    hs.build_alt(crt.ACCEL_KDTREE)
    ctx = crt.Context(W, H); hs.upload(ctx); hs.upload_alt(ctx, crt.ACCEL_KDTREE)
    ctx.set_render_accel(crt.ACCEL_KDTREE)
    ctx.render(1, FRAMES, 1)
    assert np.array_equal(ctx.accumulator().view(np.uint32), ref["kd"][0].view(np.uint32))
    assert ctx.counters()["rays"] == ref["kd"][1]
    ctx.close()
