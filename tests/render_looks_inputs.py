"""The scenes, looks, cameras and cases of the crt_update_look / crt_render_looks tests (test_gpu_update_look.py and test_gpu_render_looks.py on the GPU,
test_render_looks_cpu.py for what they assume of the oracle).  A look is a dict as cpu_ray_tracer_amd.look_dicts returns it; every named look differs from the scene
file's look (`base`) in exactly one thing, and "all" changes everything.  Texture indices are the host scene's: [0] the floor's, [1] the skydome, then the
materials' in file order.  The image is 64 x 48: twelve 16 x 16 tiles.

The oracle builds a scene per look through add_material / set_light_position / set_floor_texture / set_skydome.  It cannot express three of the looks, which are
held to the fresh-upload comparison only (ORACLE_CANNOT):
  light_turn   set_light_position is all the oracle has: its quad is never rotated;
  light_size   the oracle's quad is Quad(0, 1): size 0.5, always;
  floor        the oracle derives the floor plane's uv scale from the floor texture's width (file_scene.cpp:16), which is geometry, not part of a look: a look that
               selects another floor texture keeps the uploaded scene's scale.  (No two textures of the test scenes share width // 100.)
"""
import math
import os

import numpy as np

from conftest import ASSETS, scene_path

W, H = 64, 48
F = np.float32
SCENES = {"cube": ("cube_scene.xml", 0), "tlas": ("tlas_scene.xml", 1)}
# the camera looks up from below the light, so that the quad itself, the meshes, the floor and the sky are all in the image
CAMERAS = {"cube": ((0.0, 0.2, -2.5), (0.0, 1.3, 1.0)), "tlas": ((0.0, 0.4, -2.5), (0.0, 1.4, 1.5))}
ORACLE_CANNOT = ("light_turn", "light_size", "floor", "all")


def translate(p):
    T = np.eye(4, dtype=F); T[:3, 3] = np.asarray(p, F)
    return T


def inverse_no_scale(T):
    """mat4::FastInvertedTransformNoScale (template/tmplmath.h): the transposed rotation block and -(R^T t), summed in its order, in float32"""
    T = np.asarray(T, F).reshape(4, 4)
    inv = np.eye(4, dtype=F)
    inv[:3, :3] = T[:3, :3].T
    for i in range(3):
        inv[i, 3] = -F(F(F(T[0, i] * T[0, 3]) + F(T[1, i] * T[1, 3])) + F(T[2, i] * T[2, 3]))
    return inv


def with_light(look, T):
    out = dict(look); out["light_T"] = np.asarray(T, F).reshape(16).copy(); out["light_invT"] = inverse_no_scale(T).reshape(16)
    return out


def with_material(look, i, refl=None, refr=None, absorb=None, tex=None):
    m = list(look["materials"]); a, b, c, d = m[i]
    m[i] = (a if refl is None else refl, b if refr is None else refr, c if absorb is None else tuple(absorb), d if tex is None else tex)
    out = dict(look); out["materials"] = m
    return out


def light_position(look):
    return np.asarray(look["light_T"], F).reshape(4, 4)[:3, 3].copy()


def looks(scene, base):
    """{name: look} of `scene` ('cube' / 'tlas') round its file look `base`"""
    p = light_position(base)
    turn = np.eye(4, dtype=np.float64); a = math.radians(25.0)
    turn[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]                     # about z: the quad tilts, invT's rotation block is no identity
    out = {"base": base}
    if scene == "cube":                          # one material, untextured diffuse; textures: pavement 512 x 512, sky 1024 x 512
        out["mirror"] = with_material(base, 0, refl=1.0)
        out["glass"] = with_material(base, 0, refr=1.0, absorb=(0.3, 0.9, 0.1))
        out["tex_other"] = with_material(base, 0, tex=1)                                         # -1 -> the 1024 x 512 one
        out["tex_floor"] = with_material(base, 0, tex=0)                                         # ... and the 512 x 512 one
        out["floor"] = dict(base, floor_texture=1)
    else:                                        # wok: textured diffuse (4096 x 4096), torii: dielectric, teapot: half mirror
        out["mirror"] = with_material(base, 0, refl=1.0)
        out["glass"] = with_material(base, 2, refl=0.0, refr=1.0, absorb=(0.3, 0.9, 0.1))
        out["tex_other"] = with_material(base, 0, tex=1)                                         # 4096 x 4096 -> 1024 x 512
        out["tex_none"] = with_material(base, 0, tex=-1)
        out["floor"] = dict(base, floor_texture=2)
    out["sky"] = dict(base, sky_texture=0)
    out["light_move"] = with_light(base, translate(p + np.array([1.1, 0.0, 0.0], F)))          # sideways: tiles on the right gain the quad, tiles in the middle lose it
    out["light_turn"] = with_light(base, (translate(p).astype(np.float64) @ turn).astype(F))
    out["light_size"] = dict(base, light_size=0.9)
    every = with_light(out["glass"], (translate(p + np.array([-0.7, 0.2, 0.3], F)).astype(np.float64) @ turn).astype(F))
    every = dict(every, light_size=0.8, sky_texture=0, floor_texture=out["floor"]["floor_texture"])
    out["all"] = with_material(every, 0, tex=1)
    return out


# ---- the oracle's scene for a look ----
_images, _objs = {}, {}


def _rp(p):
    return p if os.path.isabs(p) else os.path.normpath(os.path.join(ASSETS, p))


def scene_textures(orc, sc):
    """the host scene's texture list as packed texel arrays: the floor's, the skydome, then the materials' in file order"""
    paths = [sc["plane_texture"], sc["skydome"]] + [m["texture"] for m in sc["materials"] if m["texture"]]
    for p in paths:
        if p not in _images:
            _images[p] = orc.pack_rgb(orc.read_image(_rp(p)))
    return [_images[p] for p in paths]


def make_oracle(orc, scene, look, width=W, height=H):
    """an oracle scene of `scene` with `look` (one of those the oracle can express), its renderer initialised"""
    xml, kind = SCENES[scene]
    sc = orc.read_scene_xml(scene_path(xml))
    tex = scene_textures(orc, sc)
    assert float(look["light_size"]) == 0.5 and np.array_equal(np.asarray(look["light_T"], F).reshape(4, 4)[:3, :3], np.eye(3, dtype=F))
    assert tex[look["floor_texture"]].shape[1] // 100 == tex[0].shape[1] // 100
    o = orc.Oracle(kind)
    o.set_light_position([float(x) for x in light_position(look)])
    o.set_floor_texture(tex[look["floor_texture"]])
    o.set_skydome(tex[look["sky_texture"]])
    for refl, refr, ab, t in look["materials"]:
        o.add_material(refl, refr, ab, tex[t] if t >= 0 else None)
    for ob in sc["objects"]:
        if ob["model"] not in _objs:
            _objs[ob["model"]] = orc.read_obj(_rp(ob["model"]))
        o.add_object(_objs[ob["model"]], ob["position"], ob["rotation"], ob["scale"], ob["material_idx"])
    o.build()
    o.renderer_init(width, height)
    return o


def oracle_render(o, camera, spp_first, frames, passes, threads=4):
    o.set_camera_state(*camera)
    o.clear(); o.set_spp(spp_first); o.set_params(5, passes)
    o.render(frames, threads)
    return o.accumulator().copy()


def light_tiles(orc, o, camera, width=W, height=H):
    """the tiles in which a primary ray through a pixel centre finds the light quad first (objIdx 0)"""
    o.set_camera_state(*camera)
    xs, ys = np.meshgrid(np.arange(width, dtype=F) + F(0.5), np.arange(height, dtype=F) + F(0.5))
    O, D = o.primary_rays(np.stack([xs.ravel(), ys.ravel()], axis=1))
    obj = o.find_nearest(O, D)["objIdx"].reshape(height, width)
    return {(y // 16) * (width // 16) + x // 16 for y, x in zip(*np.nonzero(obj == 0))}


def tile_slice(t, width=W):
    tx, ty = t % (width // 16), t // (width // 16)
    return slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16)


# ---- the jobs ----
class Case:
    def __init__(self, scene, names, view_look, spp_first, frames, passes):
        self.scene, self.names, self.view_look = scene, list(names), view_look
        self.spp_first, self.frames, self.passes = spp_first, frames, passes
        self.K = len(names) if view_look is None else len(view_look)

    def look_of(self, k):
        return self.names[k if self.view_look is None else int(self.view_look[k])]

    def camera(self, k):
        (px, py, pz), target = CAMERAS[self.scene]
        return ((px + 0.15 * k, py + 0.05 * k, pz), target)                                     # a camera of its own per view


CASES = {
    # 5 looks x 13 frames = 65 view-frames: a second window with one lane, lanes of different looks side by side in the first
    "cube_5x13": Case("cube", ["base", "mirror", "light_move", "sky", "all"], None, 1, 13, 1),
    "tlas_5x13": Case("tlas", ["glass", "tex_none", "light_turn", "floor", "all"], None, 1, 13, 1),
    # passes = 2, a start that is not 1
    "cube_passes2": Case("cube", ["glass", "tex_other", "light_size"], None, 5, 2, 2),
    "tlas_passes2": Case("tlas", ["mirror", "tex_other", "light_move"], None, 5, 2, 2),
    # K != L: six views over four looks, a look used twice, one order reversed
    "cube_permuted": Case("cube", ["base", "tex_floor", "floor", "light_turn"], [3, 1, 1, 0, 2, 3], 1, 1, 1),
    "tlas_permuted": Case("tlas", ["base", "sky", "light_size", "all"], [3, 1, 1, 0, 2, 3], 1, 1, 1),
}
