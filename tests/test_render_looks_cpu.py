"""What tests/test_gpu_update_look.py and tests/test_gpu_render_looks.py assume, held without a GPU: the look record's layout, the exported entries, and — on the
oracle — that every look of tests/render_looks_inputs.py changes the image at the tests' own cameras, seeds and frame counts, the light looks in a tile the move was
aimed at.  A kernel that ignores a field of a look therefore cannot pass the GPU comparisons.  The looks the oracle cannot express (render_looks_inputs.ORACLE_CANNOT:
a rotated quad, another quad size, another floor texture at the uploaded uv scale) are held to the fresh-upload comparison on the GPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import render_looks_inputs as li
from conftest import ASSETS, REPO, scene_path

F = np.float32


def test_entries_are_declared_and_exported(crt):
    L = crt.lib()
    abi = open(os.path.join(REPO, "include", "crt_abi.h")).read()
    for name in ("crt_update_look", "crt_render_looks", "crt_render_looks_device", "crt_look_words"):
        assert name in crt.ABI_SYMBOLS and getattr(L, name) is not None and re.search(r"\b%s\s*\(" % name, abi), name
    for name in ("crt_host_scene_look", "crt_host_scene_set_look"):
        assert name in crt.HOST_SYMBOLS and getattr(L, name) is not None
    for m in (0, 1, 3, 1000):
        assert L.crt_look_words(C.c_uint32(m)) == crt.look_words(m) == 36 + 6 * m
    assert C.sizeof(crt.MaterialS) == 4 * crt.LOOK_MATERIAL_WORDS


def test_packer_layout(crt):
    T = np.arange(16, dtype=F) + F(0.5); invT = -np.arange(16, dtype=F)
    look = dict(light_T=T, light_invT=invT, light_size=0.75, floor_texture=2, sky_texture=1,
                materials=[(0.25, 0.5, (0.1, 0.2, 0.3), -1), (1.0, 0.0, (0.0, 0.0, 0.0), 4)])
    rec = crt.look_records([look, look])
    assert rec.dtype == np.uint32 and rec.shape == (2, crt.look_words(2)) and rec[0].tobytes() == rec[1].tobytes()
    f, i = rec[0].view(F), rec[0].view(np.int32)
    assert np.array_equal(f[0:16], T) and np.array_equal(f[16:32], invT) and f[32] == F(0.75)
    assert (i[33], i[34], i[35]) == (2, 1, 0)                                  # floorTexture, skyTexture, the pad word
    assert np.array_equal(f[36:41], np.array([0.25, 0.5, 0.1, 0.2, 0.3], F)) and i[41] == -1
    assert np.array_equal(f[42:47], np.array([1.0, 0.0, 0.0, 0.0, 0.0], F)) and i[47] == 4
    back = crt.look_dicts(rec)[1]
    assert crt.look_records([back]).tobytes() == rec[1].tobytes()
    with pytest.raises(ValueError):
        crt.look_records([look, dict(look, materials=look["materials"][:1])])


@pytest.mark.parametrize("scene", sorted(li.SCENES))
def test_host_scene_look_round_trip(crt, scene):
    xml, kind = li.SCENES[scene]
    hs = crt.HostScene(scene_path(xml), kind, ASSETS)
    rec = hs.look()
    base = crt.look_dicts(rec)[0]
    assert rec.shape == (crt.look_words(len(base["materials"])),) and len(base["materials"]) == (1 if scene == "cube" else 3)
    assert (base["floor_texture"], base["sky_texture"], base["light_size"]) == (0, 1, 0.5)
    assert np.array_equal(base["light_invT"], li.inverse_no_scale(base["light_T"]).reshape(16))
    every = crt.look_records([li.looks(scene, base)["all"]])[0]
    hs.set_look(every)
    assert hs.look().tobytes() == every.tobytes()
    bad = crt.look_dicts(every)[0]; bad["sky_texture"] = 9
    with pytest.raises(crt.CrtError):
        hs.set_look(crt.look_records([bad])[0])
    assert hs.look().tobytes() == every.tobytes()                              # a refused look changes nothing
    names = set(li.looks(scene, base))
    for c in li.CASES.values():
        if c.scene == scene:
            assert set(c.names) <= names and c.K == (len(c.names) if c.view_look is None else len(c.view_look))


@pytest.fixture(scope="module")
def base_renders(crt, orc):
    """per scene: the file look as a dict, and the oracle's accumulator of it at the update-look tests' frames"""
    out = {}
    for scene, (xml, kind) in li.SCENES.items():
        base = crt.look_dicts(crt.HostScene(scene_path(xml), kind, ASSETS).look())[0]
        o = li.make_oracle(orc, scene, base)
        out[scene] = (base, li.oracle_render(o, li.CAMERAS[scene], 1, 3, 1), li.light_tiles(orc, o, li.CAMERAS[scene]))
    return out


@pytest.mark.parametrize("scene", sorted(li.SCENES))
def test_every_expressible_look_changes_the_image(crt, orc, base_renders, scene):
    base, want, base_light = base_renders[scene]
    assert np.isfinite(want).all() and base_light, "the camera sees the light quad"
    looks = li.looks(scene, base)
    for name, look in looks.items():
        if name == "base" or name in li.ORACLE_CANNOT:
            continue
        o = li.make_oracle(orc, scene, look)
        got = li.oracle_render(o, li.CAMERAS[scene], 1, 3, 1)
        assert not np.array_equal(got, want), (scene, name)
        if name == "light_move":
            now = li.light_tiles(orc, o, li.CAMERAS[scene])
            gained, lost = now - base_light, base_light - now
            assert gained and lost, (scene, sorted(base_light), sorted(now))
            for t in sorted(gained | lost):                                    # ... and the accumulator differs in every such tile
                assert not np.array_equal(got[li.tile_slice(t)], want[li.tile_slice(t)]), (scene, t)


def test_every_look_is_a_distinct_record(crt, base_renders):
    """the looks the oracle cannot express differ from the base at least as records, each in its own field"""
    for scene, (base, _, _) in base_renders.items():
        looks = li.looks(scene, base)
        recs = {n: crt.look_records([k])[0] for n, k in looks.items()}
        assert len({r.tobytes() for r in recs.values()}) == len(recs)
        b = recs["base"]
        changed = {n: set(np.nonzero(r != b)[0]) for n, r in recs.items()}
        assert changed["light_size"] == {32} and changed["floor"] == {33} and changed["sky"] == {34}
        assert changed["light_turn"] and changed["light_turn"] <= set(range(32)) and changed["light_move"] <= {3, 16 + 3}
        turned = np.asarray(looks["light_turn"]["light_invT"], F).reshape(4, 4)
        assert not np.array_equal(turned[:3, :3], np.eye(3, dtype=F))          # the quad's short (lightAxis) form does not apply
        assert all(min(c) >= 36 for n, c in changed.items() if n in ("mirror", "glass", "tex_other", "tex_none", "tex_floor"))
