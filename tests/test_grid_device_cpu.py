"""crt_build_grid_device / crt_get_grid — what runs without a GPU: the entries are exported and declared, and the HOST Grid::Build that the device build is held to
(through the resolution lines the two share) equals the oracle's restatement of infra/grid.cpp byte for byte on every mesh of tests/grid_build_inputs.py, each of
which is also asserted to have the shape it is there for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO
import grid_build_inputs as G


def test_entries_are_exported_and_declared(crt):
    L = crt.lib()
    abi = open(os.path.join(REPO, "include", "crt_abi.h")).read()
    host = open(os.path.join(REPO, "include", "crt_host.h")).read()
    for name in ("crt_build_grid_device", "crt_get_grid"):
        assert name in crt.ABI_SYMBOLS and getattr(L, name) is not None
        assert re.search(r"int\s+%s\s*\(\s*crt_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+bvh" % name, abi)
    for name in ("crt_host_scene_build_grid_device", "crt_host_grid_build"):
        assert name in crt.HOST_SYMBOLS and getattr(L, name) is not None and re.search(r"int\s+%s\s*\(" % name, host)
    assert re.search(r"#define\s+CRT_ABI_VERSION\s+3\b", abi) and L.crt_abi_version() == 3
    assert callable(crt.Context.build_grid_device) and callable(crt.Context.get_grid) and callable(crt.HostScene.build_grid_device)
    pos = (C.c_float * 9)()
    assert L.crt_build_grid_device(None, C.c_uint32(0), pos, C.c_uint32(1), None) == -1          # CRT_ERR_INVALID before anything touches a device
    assert L.crt_get_grid(None, C.c_uint32(0), None, None, None, None, None, None, None, None) == -1


@pytest.fixture(scope="module")
def built(crt, orc):
    """name -> (positions, host build, oracle build), each computed once"""
    out = {}
    for name in G.NAMES:
        p = G.mesh(crt, name)
        tris = np.zeros(len(p), orc.TRI_DTYPE)
        tris["vertex0"], tris["vertex1"], tris["vertex2"] = p[:, 0], p[:, 1], p[:, 2]
        a = orc.alt_accel("grid", tris); want = a.dump(); a.close()
        out[name] = (p, crt.host_grid_build(p), want)
    return out


@pytest.mark.parametrize("name", G.NAMES)
def test_host_build_equals_the_oracle(built, name):
    p, got, want = built[name]
    assert p.dtype == np.float32 and p.shape[1:] == (3, 3) and np.isfinite(p).all()
    G.assert_grids_equal(got, want, name)
    cells = int(got["resolution"].prod())
    assert len(got["cellStart"]) == cells + 1 and got["cellStart"][0] == 0 and got["cellStart"][-1] == len(got["refs"])
    for c in range(min(cells, 4096)):                                      # every cell ascending
        seg = got["refs"][got["cellStart"][c]:got["cellStart"][c + 1]]
        assert (np.diff(seg) > 0).all()


def per_cell(g):
    return np.diff(g["cellStart"].astype(np.int64))


def test_each_mesh_has_its_shape(crt, built):
    assert 128 in built["sliver"][1]["resolution"]                           # the clamp
    n = per_cell(built["cluster"][1])
    assert n.max() > 256 and (n == 0).sum() > 0                              # a long cell (the wavefront's sort), empty cells
    g = built["spanner"][1]
    starts, ends = g["cellStart"][:-1], g["cellStart"][1:]
    assert (ends > starts).all() and (g["refs"][starts] == 0).all()          # triangle 0 lies in every cell (ascending: it comes first)
    assert int(g["resolution"].prod()) > 64                                  # ... more cells than one lane takes on its own
    assert int(built["dense"][1]["resolution"].prod()) + 1 > 256 * 2048      # more chunk sums than the scan's one-block pass has threads
    for name, neg in (("zeros-neg", True), ("zeros-pos", False)):
        p, g, _ = built[name]
        assert p[..., 0].min() == 0 and p[..., 2].max() == 0
        tie = np.flatnonzero(p.reshape(-1, 3)[:, 0] == 0)
        assert len({bool(np.signbit(v)) for v in p.reshape(-1, 3)[tie, 0]}) == 2 and bool(np.signbit(p.reshape(-1, 3)[tie[-1], 0])) == neg
        assert g["boundsMin"][0] == 0 and bool(np.signbit(g["boundsMin"][0])) == neg, name
        assert g["boundsMax"][2] == 0 and bool(np.signbit(g["boundsMax"][2])) == neg, name
    assert tuple(built["flat"][1]["resolution"]) == (1, 1, 1) and built["flat"][1]["cellSize"][2] == 0
    g = built["bunny_moved"][1]
    still = crt.host_grid_build(G.scene_positions(crt))
    assert int(g["resolution"].prod()) > 1024 and tuple(g["resolution"]) != tuple(still["resolution"])
