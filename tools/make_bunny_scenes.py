"""Writes the scenes that do not fit render_pool_kernel's 16-bit node references (assets/scenes/bunny4_scene.xml, bunny14_scene.xml,
bunny4_tlas_scene.xml): copies of assets/bunny.obj, placed so that the default camera sees every one of them.

    python tools/make_bunny_scenes.py            (rewrites the three files in place; deterministic)

The schema is LoadSceneFile's, as in bunny_scene.xml / tlas_scene.xml."""
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = """<?xml version="1.0" encoding="UTF-8"?>
<!-- %s
     Written by tools/make_bunny_scenes.py.  Schema = LoadSceneFile of the reference (infra/scene/file_scene.cpp:64-135); paths as in bunny_scene.xml. -->
<scene>
    <scene_name>%s</scene_name>
    <light_position><x>0.0</x><y>3.0</y><z>1.5</z></light_position>
    <plane_texture_location>../assets/textures/Stylized_Pavement_basecolor.png</plane_texture_location>
    <skydome_location>../assets/sky_gradient.png</skydome_location>
    <objects>
"""
OBJECT = """        <object>
            <model_location>../assets/bunny.obj</model_location>
            <material_idx>%d</material_idx>
            <position><x>%s</x><y>%s</y><z>%s</z></position>
            <rotation><x>0.0</x><y>%s</y><z>0.0</z></rotation>
            <scale><x>%s</x><y>%s</y><z>%s</z></scale>
        </object>
"""
MATERIAL = """        <material>
            <reflectivity>%s</reflectivity>
            <refractivity>%s</refractivity>
            <absorption><x>%s</x><y>%s</y><z>%s</z></absorption>
            <texture_location></texture_location>
        </material>
"""


def scene(name, note, objects, materials):
    s = HEAD % (note, name)
    for (mat, x, y, z, rot, sc) in objects:
        s += OBJECT % (mat, x, y, z, rot, sc, sc, sc)
    s += "    </objects>\n    <materials>\n"
    for m in materials:
        s += MATERIAL % m
    s += "    </materials>\n</scene>\n"
    return s


def grid(counts, depth, spread, y0, rise, scale, mats=1):
    """rows of bunnies above one another, all at one depth, so that none hides another: row r has counts[r] bunnies `spread` apart, centred on the view axis,
    standing at height y0 + r * rise (row 0 on the floor).  The default camera sits at (0, 0, -2) and sees |x| < 0.75 d, |y| < 0.5 d at distance d."""
    out, k = [], 0
    for r, n in enumerate(counts):
        for i in range(n):
            out.append((k % mats, round((i - (n - 1) / 2.0) * spread, 3), round(y0 + r * rise, 3), depth, 180.0 + 20.0 * ((k % 5) - 2), scale))
            k += 1
    return out


DIFFUSE = ("0.0", "0.0", "0.0", "0.0", "0.0")
SCENES = {
    "bunny4_scene.xml": ("bunny4 scene", "FileScene, 4 x bunny.obj = 19 872 triangles in one BVH: past the 14-bit index of the 16-bit node references",
                         grid([2, 2], 2.5, 2.6, -1.0, 1.6, 1.0), [DIFFUSE]),
    "bunny14_scene.xml": ("bunny14 scene", "FileScene, 14 x bunny.obj = 69 552 triangles in one BVH: leaf indices pass 65 535",
                          grid([4, 5, 5], 2.5, 1.3, -1.0, 1.08, 0.7), [DIFFUSE]),
    "bunny4_tlas_scene.xml": ("bunny4 tlas scene", "TLASFileScene, 4 bunny BLAS (4 x 4 968 triangles), each with its own transform and material: diffuse, mirror, dielectric, 50 % mirror",
                              grid([2, 2], 2.5, 2.6, -1.0, 1.6, 1.0, mats=4),
                              [DIFFUSE, ("1.0", "0.0", "0.0", "0.0", "0.0"), ("0.0", "1.0", "0.2", "0.0", "0.4"), ("0.5", "0.0", "0.0", "0.0", "0.0")]),
}

if __name__ == "__main__":
    for fn, (name, note, objects, materials) in SCENES.items():
        with open(os.path.join(REPO, "assets", "scenes", fn), "w") as f:
            f.write(scene(name, note, objects, materials))
        print(fn, len(objects), "objects")
