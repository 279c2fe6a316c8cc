"""crt_update_transforms_device without a GPU: the library exports the entry, and the numpy restatement of the build as the kernel does it
(tests/tlas_device_inputs.py: the argmin rule, the fixed-size list) gives byte for byte the TLAS of the oracle and of the host front for every input set, while
the sets keep exercising what they were chosen for."""
import ctypes as C

import numpy as np
import pytest

from conftest import ASSETS
import tlas_device_inputs as inp

BUILDABLE = [s for s in inp.SETS if s != "nan"]


def test_library_exports_the_entries(crt):
    L = C.CDLL(crt.build())
    for name in ("crt_update_transforms_device", "crt_host_scene_update_transforms_device"):
        assert hasattr(L, name), name
        assert name in crt.ABI_SYMBOLS + crt.HOST_SYMBOLS


@pytest.fixture(scope="module")
def restated(crt, orc, tmp_path_factory):
    """per set: the restatement's result from the node-0 boxes of the loaded scene, next to the oracle and the host scene after set_transform for every instance"""
    out = {}
    tmp = tmp_path_factory.mktemp("tlas_device")
    for name in inp.SETS:
        xml = inp.scene_xml(tmp, name)
        T = inp.transforms(name)
        hs = crt.HostScene(xml, 1, ASSETS)
        assert hs.bvh_count() == inp.COUNT[name]
        boxes = np.stack([np.stack([hs.bvh(i)["nodes"][0]["aabbMin"], hs.bvh(i)["nodes"][0]["aabbMax"]]) for i in range(len(T))])
        r = inp.restate(boxes, T)
        if name != "nan":
            o, _ = orc.load_scene(xml, 1, ASSETS)
            for i in range(len(T)):
                o.set_transform(i, T[i]); hs.set_transform(i, T[i])
            r["oracle"], r["host"] = o, hs
        out[name] = r
    return out


@pytest.mark.parametrize("name", BUILDABLE)
def test_restatement_is_the_oracles_and_the_host_fronts_build(restated, name):
    r = restated[name]
    n = inp.COUNT[name]
    for who in ("oracle", "host"):
        nodes, used = r[who].tlas()
        assert used == 2 * n
        assert r["nodes"].tobytes() == nodes.tobytes(), who
        for i in range(n):
            T, invT, lo, hi = r[who].blas_transform(i)
            assert invT.tobytes() == r["invT"][i].tobytes() and lo.tobytes() == r["world"][i, 0].tobytes() and hi.tobytes() == r["world"][i, 1].tobytes(), (who, i)
    assert r["no_candidate"] is None
    print(name, "height", r["height"], "searches", r["searches"], "stale A", r["stale_a"], "ties", r["ties"])


def test_inputs_exercise_what_they_were_chosen_for(restated):
    for name in ("rand256", "line256"):
        assert restated[name]["stale_a"] >= 1, name                 # A, the last entry, outside the shortened list
        assert 3 * 256 < restated[name]["searches"] < 5 * 256
    for name in ("lattice64", "same8"):
        assert restated[name]["ties"] >= 1, name                    # equal areas: the lowest list index wins
    assert restated["one"]["searches"] == 1 and restated["one"]["height"] == 0 and restated["one"]["nodes"]["leftRight"][0] == 0
    assert restated["two"]["height"] == 1
    assert restated["nan"]["no_candidate"] is not None              # the reference's list[-1]
    assert len({restated[n]["height"] for n in BUILDABLE}) >= 5     # shallow and deep trees
