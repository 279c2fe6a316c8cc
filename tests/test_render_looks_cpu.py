"""What tests/test_gpu_update_look.py and tests/test_gpu_render_looks.py assume, held without a GPU: the look record's layout, the exported entries, and — on the
oracle — that every look of tests/render_looks_inputs.py changes the image at the tests' own cameras, seeds and frame counts, the light looks in a tile the move was
aimed at.  A kernel that ignores a field of a look therefore cannot pass the GPU comparisons.  The rotated and resized quads and the other floor texture at the
uploaded uv scale are looks no scene file gives: the oracle takes them through set_light_quad / set_floor_uv_scale, held here to be kept across a rebuild and to
change nothing while unset."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hit_info_restate as hr
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
def test_every_look_changes_the_image(crt, orc, base_renders, scene):
    base, want, base_light = base_renders[scene]
    assert np.isfinite(want).all() and base_light, "the camera sees the light quad"
    looks = li.looks(scene, base)
    for name, look in looks.items():
        if name == "base":
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
    """the looks differ from the base as records, each in its own field"""
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


@pytest.mark.parametrize("scene", sorted(li.SCENES))
def test_oracle_setters_unset_kept_and_applied(crt, orc, base_renders, scene):
    """set_light_quad / set_floor_uv_scale: the file look through them is the scene file's own oracle bit for bit; they hold across a rebuild and reach a built
    scene at once; the built quad is the look's, cell for cell"""
    base, want, _ = base_renders[scene]
    xml, kind = li.SCENES[scene]
    plain, _ = orc.load_scene(scene_path(xml), kind, ASSETS)                   # no setter called: Translate(light position), Quad(0, 1), 1 / (width // 100)
    plain.renderer_init(li.W, li.H)
    assert np.array_equal(li.oracle_render(plain, li.CAMERAS[scene], 1, 3, 1).view(np.uint32), want.view(np.uint32))
    a, b = plain.light(), li.make_oracle(orc, scene, base).light()
    assert all(np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)) for k in a), (a, b)
    looks = li.looks(scene, base); looks.update(li.quad_looks(scene, base))
    for name in ("all", "zyx_size_0.9", "quarter_z"):
        look = looks[name]
        o = li.make_oracle(orc, scene, look)
        got = li.oracle_render(o, li.CAMERAS[scene], 1, 3, 1)
        q = o.light()
        T = np.asarray(look["light_T"], F).reshape(4, 4)
        assert np.array_equal(q["T"], T) and np.array_equal(q["invT"], li.inverse_no_scale(T)) and q["size"] == F(look["light_size"])
        assert np.array_equal(q["normal"], -T[:3, 1]) and q["floor_invto"] == b["floor_invto"]
        o.build()                                                              # a rebuild keeps both
        o.renderer_init(li.W, li.H)
        assert np.array_equal(li.oracle_render(o, li.CAMERAS[scene], 1, 3, 1).view(np.uint32), got.view(np.uint32)), name
        plain.set_light_quad(look["light_T"], look["light_invT"], look["light_size"])       # on a built scene: at once
        q2 = plain.light()
        assert np.array_equal(q2["T"], q["T"]) and np.array_equal(q2["invT"], q["invT"]) and q2["size"] == q["size"] and np.array_equal(q2["pos"], q["pos"])
    plain.set_floor_uv_scale(0.125)
    assert plain.light()["floor_invto"] == F(0.125)


@pytest.mark.parametrize("scene", sorted(li.SCENES))
def test_every_quad_look_changes_the_image_and_is_seen(crt, orc, base_renders, scene):
    """the transforms and sizes of render_looks_inputs.quad_looks: each but the half turn changes the oracle's image at the tests' camera; the quarter turn and the half turn leave
    the short (lightAxis) form; no cell of any invT is -0.0 (a quarter or half turn from cells 0 / +-1 has none), so the lightAxis comparison never meets one"""
    base, want, base_light = base_renders[scene]
    for name, look in li.quad_looks(scene, base).items():
        o = li.make_oracle(orc, scene, look)
        got = li.oracle_render(o, li.CAMERAS[scene], 1, 3, 1)
        # half_x turns the square onto itself: the path tracer, which returns the light's colour from either face, renders the file look's image to the bit
        # (what tells it apart is GetHitInfo's normal: test_gpu_light_quad.py)
        assert np.isfinite(got).all() and np.array_equal(got, want) == (name == "half_x"), (scene, name)
        inv = np.asarray(look["light_invT"], F).reshape(4, 4)[:3, :3]
        assert not (np.signbit(inv) & (inv == 0)).any(), name
        assert np.array_equal(inv, np.eye(3, dtype=F)) == name.startswith("size_"), name
        if name.startswith("size_"):                                           # at the close camera: tiles gained by the larger quads, a pixel centre on the smallest
            cam = li.QUAD_CAMERAS[scene]
            now, before = li.light_tiles(orc, o, cam), li.light_tiles(orc, li.make_oracle(orc, scene, base), cam)
            assert (now < before and len(now) == 1) if name == "size_0.03125" else (now > before), (name, sorted(before), sorted(now))
    q = li.transforms(li.light_position(base))
    assert np.array_equal(q["quarter_z"][:3, :3], np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], F)) and np.array_equal(-q["quarter_z"][:3, 1], np.array([-1, 0, 0], F))
    assert np.array_equal(-q["half_x"][:3, 1], np.array([0, 1, 0], F))
    R = q["zyx"][:3, :3]
    assert (R != 0).all() and np.abs(R - R.T)[np.triu_indices(3, 1)].min() > 0.05                # R and its transpose differ in every off-diagonal pair


@pytest.mark.parametrize("scene", sorted(li.SCENES))
def test_floor_records_tell_the_uploaded_scale_from_the_selected_textures(crt, orc, base_renders, scene):
    """the rays of render_looks_inputs.floor_rays under the looks that select another floor texture: hit_info_restate with the look (the uv scale kept from the
    uploaded floor texture) and its other reading (the scale taken from the selected texture's width) differ on at least a tenth of the records, in uv and in
    albedo, so test_gpu_light_quad.py's comparison can tell the two apart; the oracle with set_floor_uv_scale samples what the restatement's texel says"""
    base, _, _ = base_renders[scene]
    xml, kind = li.SCENES[scene]
    looks = li.looks(scene, base)
    o, sc = orc.load_scene(scene_path(xml), kind, ASSETS)
    sh = hr.SceneShading(orc, o, sc, kind, ASSETS)
    invto = sh.floor_invto
    O, D = li.floor_rays(invto)
    hits = o.find_nearest(O, D)
    floor = hits["objIdx"] == 1
    assert floor.sum() >= 0.8 * len(O)
    for name in ("floor", "all"):
        look = looks[name]
        sh.set_look(look)
        assert sh.floor_invto == invto and sh.floor_tex.shape[1] // 100 != int(round(1 / float(invto)))
        ol = li.make_oracle(orc, scene, look)
        hl = ol.find_nearest(O, D); fl = hl["objIdx"] == 1
        kept = sh.hit_info(O, D, hl)
        other = hr.SceneShading(orc, o, sc, kind, ASSETS); other.set_look(look)
        other.floor_invto = F(1) / F(other.floor_tex.shape[1] // 100)
        wrong = other.hit_info(O, D, hl)
        differ = fl & ((kept["u"] != wrong["u"]) | (kept["v"] != wrong["v"]))
        assert differ.sum() >= 0.1 * len(O) and (fl & (kept["albedo"] != wrong["albedo"]).any(1)).sum() >= 0.1 * len(O), (name, int(differ.sum()))
        u = kept["u"][fl]
        assert (u < 1e-3).sum() >= 20 and (u > 1 - 1e-3).sum() >= 20            # both sides of the wrap
        # the oracle's Sample of a floor hit whose bounce escapes to nothing brighter is hard to isolate; what it reads is held through its image instead:
        # with the other scale the oracle renders another image
        a = li.oracle_render(ol, li.CAMERAS[scene], 1, 2, 1)
        ol.set_floor_uv_scale(F(1) / F(sh.floor_tex.shape[1] // 100))
        assert not np.array_equal(a, li.oracle_render(ol, li.CAMERAS[scene], 1, 2, 1)), name
