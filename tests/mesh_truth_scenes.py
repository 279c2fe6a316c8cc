"""What tests/test_mesh_truth_cpu.py and tests/test_gpu_mesh_truth.py share beside the truth itself (tests/mesh_truth.py, which stays free of the oracle and the
library): the scenes, how the oracle loads and walks them, and how a violating ray is reported.  Not collected by pytest."""
import os

import numpy as np

import mesh_truth as mt
from conftest import ASSETS, scene_path
from test_gpu_golden_and_edges import write_scene

SCENES = {"bunny": 0, "tlas": 1, "gen": 1}


def describe(orc, xml):
    """(scene description, light, material index per object, floor invto) read from the scene file by the oracle-side readers"""
    sc = orc.read_scene_xml(xml)
    tex = orc.read_image(os.path.normpath(os.path.join(ASSETS, sc["plane_texture"])))
    return sc, sc["light"], [ob["material_idx"] for ob in sc["objects"]], 1.0 / (tex.shape[1] // 100)


def scene_xml(name, tmp):
    return mt.write_generated(tmp, write_scene) if name == "gen" else scene_path(name + "_scene.xml")


def load(orc, name, tmp):
    """(oracle scene, description, world) of a scene; the generated one moved to its scaled transforms"""
    xml = scene_xml(name, tmp); kind = SCENES[name]
    o, _ = orc.load_scene(xml, kind, ASSETS)
    if name == "gen":
        for i, T in enumerate(mt.generated_transforms(o)):
            o.set_transform(i, T)
    sc, light, obj_mat, invto = describe(orc, xml)
    return o, sc, mt.world_of(o, kind, light, obj_mat, invto)


def through(orc, o, world_name):
    """walk the oracle scene through `world_name`'s structure from now on (built over the scene's CURRENT triangles)"""
    name = world_name.split("_")[-1]
    if name in ("kd", "grid"):
        if o.kind == 0:
            o._alt = orc.alt_accel(name, o.bvh(0)["tris"]); orc.set_render_accel(o, o._alt)
        else:
            orc.set_blas_accel(o, orc.blas_accels(o, name))
    elif o.kind == 0:
        orc.set_render_accel(o, None)
    else:
        orc.set_blas_accel(o, None)
    return o


def report(what, viol, O, D, hits, tr):
    rays = mt.rays_of(viol)[:6]
    return (what, {k: len(v) for k, v in viol.items()},
            [dict(ray=int(i), O=O[i].tolist(), D=D[i].tolist(), got=(float(hits["t"][i]), int(hits["objIdx"][i]), int(hits["triIdx"][i])),
                  t_lo=float(tr["t_lo"][i]), t_hi=float(tr["t_hi"][i]), want=(int(tr["obj"][i]), int(tr["tri"][i]))) for i in rays])


def moved_records(tris, p):
    t = np.array(tris)
    t["vertex0"], t["vertex1"], t["vertex2"] = p[:, 0], p[:, 1], p[:, 2]
    return t
