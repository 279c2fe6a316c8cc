"""crt_trace / crt_trace_device (the Whitted Renderer::Trace for ray arrays) — what runs without a GPU.

tests/trace_restate.py restates Trace's recursion in numpy float32 over the oracle's FindNearest / IsOccluded / expf and hit_info_restate's shading.  It is the
yardstick of tests/test_gpu_trace_query.py for rays no camera produces, so it is itself pinned to the oracle first: the restated Trace of the camera's pixel rays
must be orc_whitted_render's accumulator bit for bit, in a two-level scene with a dielectric and a half mirror (assets/scenes/tlas_scene.xml) and in a FileScene of
three cubes (full mirror, dielectric with absorption, half mirror), at depthLimit 5 and, for the cubes, 1.  The cameras were chosen with the oracle alone; each
image is asserted to hold sky, floor, light, mirror and dielectric pixels, and the oracle alone shows that the recursion reaches depthLimit.

Plus the header / export / binding checks of the new entries."""
import os
import re

import numpy as np
import pytest

import trace_restate as R
from conftest import ASSETS, REPO

ENTRIES = ("crt_trace", "crt_trace_device")
SCENES = os.path.join(ASSETS, "scenes")


def whitted_image(o, depth_limit):
    o.set_params(depth_limit=depth_limit, passes=1)
    o.whitted()
    return o.accumulator()


@pytest.mark.parametrize("name,depth_limit", [("tlas", 5), ("cubes", 5), ("cubes", 1)])
def test_restated_trace_equals_the_oracles_whitted_image(orc, tmp_path, name, depth_limit):
    xml, kind = R.scene_of(name, tmp_path, SCENES)
    o, sh, tr = R.load(orc, xml, kind, ASSETS, name, depth_limit)
    # what the image holds, by the oracle's FindNearest and the scene file's materials
    c = R.pixel_classes(tr, o)
    mirrors = c["mirror"] + c["half_mirror"]
    assert min(c["sky"], c["floor"]) >= 100 and min(c["light"], mirrors, c["dielectric"]) >= 5, c
    if name == "cubes":
        assert min(c["mirror"], c["half_mirror"]) >= 50, c
        mats = sh.materials
        assert [(m["reflectivity"], m["refractivity"]) for m in mats] == [(1.0, 0.0), (0.0, 1.0), (0.5, 0.0)] and max(mats[1]["absorption"]) > 0
    # the recursion reaches depthLimit, by the oracle alone: the rays traced AT depth depthLimit change pixels, and so would rays one level deeper
    want = whitted_image(o, depth_limit)
    shallower, deeper = whitted_image(o, depth_limit - 1), whitted_image(o, depth_limit + 1)
    assert (R.bits(want) != R.bits(shallower)).any() and (R.bits(want) != R.bits(deeper)).any()
    o.set_params(depth_limit=depth_limit, passes=1)
    # the restatement
    O, D = R.pixel_rays(o, R.W, R.H)
    counts = {}
    got = tr.trace(O, D, counts=counts)
    bad = R.differing(got, want.reshape(-1, 4)[:, :3])
    assert len(bad) == 0, ("pixels that differ", len(bad), bad[:5].tolist())
    assert (want[..., 3] == 0).all()
    # both children of a dielectric were followed somewhere (a tree of more nodes than a chain of depthLimit + 1), sky pixels are one FindNearest
    if depth_limit == 5:
        assert counts["cost"].max() > depth_limit + 1 and (counts["cost"] == 1).sum() >= c["sky"] + c["light"]
    hits = o.find_nearest(O, D)
    assert np.array_equal(counts["traversed"], hits["traversed"]) and np.array_equal(counts["tested"], hits["tested"])


def test_restated_trace_of_inside_rays_absorbs(orc, tmp_path):
    """rays that start inside the dielectric cube with inside = 1: the medium's absorption applies to the first segment (the result differs from the same ray with
    inside = 0, which also refracts with the indices swapped), and the restatement follows both; a depth above depthLimit returns black without tracing"""
    xml, kind = R.scene_of("cubes", tmp_path, SCENES)
    o, sh, tr = R.load(orc, xml, kind, ASSETS, "cubes")
    rng = np.random.default_rng(3)
    n = 64
    O = np.tile(np.float32(R.GLASS_C), (n, 1)) + rng.uniform(-0.1, 0.1, (n, 3)).astype(np.float32)
    D = rng.normal(size=(n, 3)); D[:, 1] = np.abs(D[:, 1])              # rising: the cube stands ON the floor, its bottom face lies in the floor's plane
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(np.float32)
    hit = o.find_nearest(O, D)
    assert (hit["objIdx"] == 3).all()                                         # the glass cube is object 1: every ray meets its inner wall first
    a, b = tr.trace(O, D, np.ones(n, np.int32)), tr.trace(O, D, np.zeros(n, np.int32))
    assert np.isfinite(a).all() and len(R.differing(a, b)) > n // 2
    assert not tr.trace(O, D, depth=6).any()


def test_header_declares_the_entries():
    h = open(os.path.join(REPO, "include", "crt_abi.h")).read()
    assert re.search(r"\bint\s+crt_trace\s*\(\s*crt_ctx\*\s*\w+,\s*int\s+accel,\s*const\s+crt_ray\*\s*\w+,\s*float\*\s*\w+[^,]*,\s*int32_t\*\s*\w+[^,]*,\s*int32_t\*\s*\w+[^,]*,\s*size_t\s+n\s*\)", h)
    assert re.search(r"\bint\s+crt_trace_device\s*\(\s*crt_ctx\*\s*\w+,\s*int\s+accel,\s*const\s+crt_ray\*\s*\w+,\s*float\*\s*\w+[^,]*,\s*int32_t\*\s*\w+[^,]*,\s*int32_t\*\s*\w+[^,]*,"
                     r"\s*size_t\s+n,\s*void\*\s*stream\s*\)", h)
    assert "#define CRT_ABI_VERSION 3" in h


def test_library_exports_the_entries_and_the_binding_has_them(crt):
    lib = crt.lib()
    for e in ENTRIES:
        assert e in crt.ABI_SYMBOLS
        getattr(lib, e)
    getattr(lib, "crt_debug_trace_resident_lanes")
    assert lib.crt_abi_version() == 3
    for m in ("trace", "trace_device", "trace_resident_lanes"):
        assert callable(getattr(crt.Context, m))
