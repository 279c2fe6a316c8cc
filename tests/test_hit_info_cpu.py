"""The shading queries (crt_get_hit_info / crt_get_sky_color / crt_get_light, crt_abi.h "scene queries") — what runs without a GPU.

tests/hit_info_restate.py restates GetHitInfo, GetAlbedo and GetSkyColor in numpy float32; it is the yardstick of tests/test_gpu_hit_info.py, and here it is
itself pinned to the oracle first:

  * the Whitted renderer's Trace, assembled from FindNearest, the restated hit info and IsOccluded, must give the oracle's Whitted image bit for bit;
  * the restated sky colour must be the oracle's Sample of a ray that misses, bit for bit.

Plus the header / export checks of the new entries."""
import os
import re

import numpy as np
import pytest

import hit_info_restate as hr
from conftest import ASSETS, REPO, scene_path
from test_gpu_golden_and_edges import write_scene
from test_gpu_scene_queries import quad_occluded

W, H = 160, 96
# Chosen with the oracle alone so that every image holds floor, mesh, sky and the light quad (the default camera sees neither the light, 45 degrees up, nor
# the floor): asserted below per scene.
CAMERA = ((0.0, 1.0, -4.0), (0.0, 1.0, -3.0))
ENTRIES = ("crt_get_hit_info", "crt_get_hit_info_device", "crt_get_sky_color", "crt_get_sky_color_device", "crt_get_light")


def whitted_xml(name, tmp_path):
    """the scenes of the Whitted assembly: every material diffuse, so that Trace never recurses"""
    if name == "tower_small":                                            # tower_scene.xml's tower at scale 0.3: all of it below the light's plane (see below)
        return write_scene(tmp_path, "watch-tower", pos=(0.0, -1.0, 3.5), rot=(0.0, 90.0, 0.0), scale=(0.3, 0.3, 0.3),
                           mats=[(0.0, 0.0, (0.0, 0.0, 0.0), "../assets/textures/Wood_Tower_Col.png")])
    return scene_path(name + "_scene.xml")


def load(orc, xml, kind=0):
    o, sc = orc.load_scene(xml, kind, ASSETS)
    return o, hr.SceneShading(orc, o, sc, kind, ASSETS)


def primary_rays(o):
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2).astype(np.float32)     # Trace(camera.GetPrimaryRay((float)x, (float)y)), row-major
    return o.primary_rays(xy)


def check_image_conditions(hits):
    obj = hits["objIdx"]; n = len(obj)
    assert (obj == 1).sum() >= 0.01 * n and (obj >= 2).sum() >= 0.01 * n and (obj == -1).sum() >= 0.01 * n and (obj == 0).sum() >= 1, \
        ("floor / mesh / sky / light pixels", (obj == 1).sum(), (obj >= 2).sum(), (obj == -1).sum(), (obj == 0).sum())


def assemble(sh, O, D, hits, info, occluded_fn):
    """the Whitted image (H, W, 4) from the primary rays' hit-info records; occluded_fn(origin, L, t) = IsOccluded of the shadow rays"""
    lp = sh.light_pos()
    org, L, t, _, _ = hr.shadow_rays(info, lp)
    return hr.whitted_diffuse(info, occluded_fn(org, L, t), lp).reshape(H, W, 4)


def oracle_occluded(o, sh):
    """IsOccluded (file_scene.cpp:177-187) from the oracle's exports: Quad::IsOccluded bounded by t, or a mesh as the nearest hit of the unbounded ray.  The
    reference intersects the structure over the WHOLE ray, so the two agree provided no mesh lies beyond the light's plane on a ray towards the light centre:
    every BVH root box must end below the light (asserted)."""
    for i in range(o.bvh_count()):
        assert o.bvh(i)["nodes"][0]["aabbMax"][1] < sh.light[1], "a mesh reaches above the light's plane"

    def fn(org, L, t):
        with np.errstate(all="ignore"):
            return quad_occluded(org, L, t, tuple(float(v) for v in sh.light))[0] | (o.find_nearest(org, L)["objIdx"] >= 2)
    return fn


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", ["bunny", "cube", "tower_small"])
def test_whitted_assembled_from_queries_equals_oracle(orc, tmp_path, name):
    o, sh = load(orc, whitted_xml(name, tmp_path))
    assert all(m["reflectivity"] == 0 and m["refractivity"] == 0 for m in sh.materials)
    o.renderer_init(W, H)
    o.set_camera_state(*CAMERA)
    O, D = primary_rays(o)
    hits = o.find_nearest(O, D)
    check_image_conditions(hits)
    info = sh.hit_info(O, D, hits)
    img = assemble(sh, O, D, hits, info, oracle_occluded(o, sh))
    o.whitted()
    want = o.accumulator()
    bad = (bits(img) != bits(want)).any(axis=2)
    assert not bad.any(), ("pixels that differ", int(bad.sum()), np.argwhere(bad)[:5].tolist())


def sky_directions():
    """20 000 random unit directions with a positive y, the +y axis, and directions with one or two zero components"""
    rng = np.random.default_rng(2024)
    v = rng.normal(size=(20000, 3)); v[:, 1] = np.abs(v[:, 1]) + 1e-3
    D = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    s = np.float32(np.sqrt(0.5))
    special = np.array([[0, 1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [s, s, 0], [-s, s, 0], [0, s, s], [0, s, -s], [s, 0, s], [-s, 0, s], [s, 0, -s], [-s, 0, -s],
                        [0.6, 0.8, 0], [0, 0.8, -0.6]], np.float32)
    D = np.concatenate([special, D])
    O = np.tile(np.array([[0.0, 10.0, 0.0]], np.float32), (len(D), 1))    # above every mesh, the light and the floor: nothing can be hit going up or level
    return O, D


def oracle_sky(o, O, D):
    return np.stack([o.sample(O[i], D[i], 1 + i)[0] for i in range(len(D))])


def test_sky_equals_oracle(orc):
    o, sh = load(orc, scene_path("bunny_scene.xml"))
    O, D = sky_directions()
    assert (o.find_nearest(O, D)["objIdx"] == -1).all()
    want = oracle_sky(o, O, D)                                           # Sample at depth 0: a miss returns GetSkyColor
    got = sh.sky(D)
    assert np.array_equal(bits(got), bits(want))
    assert len(np.unique(bits(got), axis=0)) > 50                        # the directions do sweep the texture


def test_light_restated(orc):
    o, sh = load(orc, scene_path("tlas_scene.xml"), 1)
    assert np.array_equal(sh.light_pos(), np.float32([0.0, 3.0, 1.5]) - np.float32([0, 0.01, 0]))
    assert np.array_equal(sh.light_normal(), np.float32([-0.0, -1.0, -0.0]))


def test_header_declares_the_entries():
    h = open(os.path.join(REPO, "include", "crt_abi.h")).read()
    for e in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % e, h), e
    assert "#define CRT_ABI_VERSION 3" in h
    assert re.search(r"#define\s+CRT_MATERIAL_MISS\s+\(-1\)", h) and re.search(r"#define\s+CRT_MATERIAL_INVALID\s+\(-2\)", h)
    assert "typedef struct crt_hit_info" in h


def test_library_exports_the_entries(crt):
    assert crt.HIT_INFO_DTYPE.itemsize == 48 and crt.HIT_INFO_DTYPE == hr.HIT_INFO_DTYPE
    assert [crt.HIT_INFO_DTYPE.fields[f][1] for f in ("I", "material", "N", "u", "albedo", "v")] == [0, 12, 16, 28, 32, 44]
    lib = crt.lib()
    for e in ENTRIES:
        assert e in crt.ABI_SYMBOLS
        getattr(lib, e)
    assert lib.crt_abi_version() == 3
    assert (crt.MATERIAL_MISS, crt.MATERIAL_INVALID) == (-1, -2)
