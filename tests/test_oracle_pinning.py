"""CPU tests that pin the oracle:
  * against the REAL reference compiled in place (oracle/_ref: infra/bvh.cpp, tinyobj, stb_image) where it can be built, and elsewhere
    against the outputs it gave for the same inputs (tests/golden/ref_live*);
  * against the committed golden vectors those runs produced (tests/golden/ref_*) — everywhere, including the GPU box;
  * regression vectors for the parts with no executable reference (tests/golden/orc_*, "parity unpinned")."""
import json
import os
import zlib

import numpy as np
import pytest

from conftest import ASSETS, GOLDEN, scene_path

G = json.load(open(os.path.join(GOLDEN, "golden.json")))
MESHES = sorted(G["ref_bvh"].keys())


def crc(a):
    return int(zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff)


def simple_scene(orc, mesh, kind=0):
    o = orc.Oracle(kind)
    o.set_light_position((0, 3, 1))
    o.set_floor_texture(np.full((512, 512), 0x808080, np.uint32))
    o.set_skydome(np.full((4, 8), 0x6080c0, np.uint32))
    o.add_material()
    o.add_object(orc.read_obj(os.path.join(ASSETS, mesh + ".obj")), (0, -1, 2), (0, 180, 0), (1, 1, 1), 0)
    o.build()
    return o


# ---------------------------------------------------------------------------------------------------------------
# golden vectors produced by the real reference
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", MESHES)
def test_obj_reader_matches_tinyobj_golden(orc, mesh):
    pos, nrm, uv = orc.read_obj(os.path.join(ASSETS, mesh + ".obj"))
    g = G["ref_obj"][mesh]
    assert pos.shape[0] == g["corners"]
    assert (crc(pos), crc(nrm), crc(uv)) == (g["pos"], g["nrm"], g["uv"])


@pytest.mark.parametrize("img", sorted(G["ref_img"].keys()))
def test_image_reader_matches_stb_golden(orc, img):
    a = orc.read_image(os.path.join(ASSETS, img))
    assert list(a.shape) == G["ref_img"][img]["shape"]
    assert crc(orc.pack_rgb(a)) == G["ref_img"][img]["packed"]


@pytest.mark.parametrize("mesh", MESHES)
def test_oracle_bvh_build_matches_reference_golden(orc, mesh):
    b = simple_scene(orc, mesh).bvh(0)
    g = G["ref_bvh"][mesh]
    assert crc(b["tris"]) == g["tris_crc"], "triangle soup differs: the build comparison would be meaningless"
    assert (b["nodesUsed"], b["maxDepth"]) == (g["nodesUsed"], g["maxDepth"])
    assert crc(b["nodes"]) == g["nodes"] and crc(b["triIndices"]) == g["triIndices"]


@pytest.mark.parametrize("mesh", ["bunny", "teapot", "cube"])
def test_oracle_traversal_matches_reference_golden(orc, mesh):
    """Rays against BVH::Intersect of the reference.  The oracle's FindNearest tests the light quad and the floor first;
    rays are compared where the mesh is (or is not) the nearest thing in both."""
    z = np.load(os.path.join(GOLDEN, "ref_bvh_rays.npz"))
    O, D = z[mesh + "_O"], z[mesh + "_D"]
    o = simple_scene(orc, mesh)
    h = o.find_nearest(O, D)
    rt, ro = z[mesh + "_t"], z[mesh + "_objIdx"]
    both = (h["objIdx"] >= 2) & (ro >= 2)
    assert both.sum() > 200
    for f in ("t", "u", "v"):
        assert np.array_equal(h[f][both].view(np.uint32), z[mesh + "_" + f][both].view(np.uint32)), f
    assert np.array_equal(h["triIdx"][both], z[mesh + "_triIdx"][both])
    other = (ro >= 2) & ~(h["objIdx"] >= 2)          # reference hit the mesh, oracle reports floor / light: must be nearer
    assert np.all(h["t"][other] < rt[other])
    assert not ((h["objIdx"] >= 2) & (ro < 2)).any()
    miss = (h["objIdx"] == -1) & (ro == -1)             # nothing shortened t before the traversal: loop-trip counters must agree
    assert np.array_equal(h["traversed"][miss], z[mesh + "_traversed"][miss])
    assert np.array_equal(h["tested"][miss], z[mesh + "_tested"][miss])


def camera_oracle(orc, pos_target):
    o = orc.Oracle(0)
    o.renderer_init(1024, 640)                       # the resolution template/camera.h is compiled for (SCRWIDTH x SCRHEIGHT)
    if pos_target is not None:
        o.set_camera_state(*pos_target)
    return o


@pytest.mark.parametrize("name", sorted(G["ref_camera"]["cams"].keys()))
def test_oracle_camera_matches_reference_golden(orc, name):
    """Camera(): default frustum, SetCameraState and GetPrimaryRay of the real reference (template/camera.h:14-30, 61-73)"""
    g = G["ref_camera"]["cams"][name]
    xy = np.load(os.path.join(GOLDEN, "ref_camera_xy.npy"))
    assert crc(xy) == G["ref_camera"]["xy"]
    o = camera_oracle(orc, g["pos_target"])
    assert crc(np.stack(o.camera())) == g["corners"]
    O, D = o.primary_rays(xy)
    assert (crc(O), crc(D)) == (g["O"], g["D"])


def test_oracle_texture_matches_reference_golden(orc):
    """Texture::LoadFromFile's packing, Texture::Sample and Material::GetAlbedo of the real reference (template/texture.h, material.h)"""
    g = G["ref_texture"]
    tex = orc.pack_rgb(orc.read_image(os.path.join(ASSETS, g["file"])))
    assert crc(tex) == g["texels"]
    assert crc(orc.pack_rgb(orc.read_image(os.path.join(ASSETS, "textures/Stylized_Wood_basecolor.tga")))) == g["tga"]
    uv = np.load(os.path.join(GOLDEN, "ref_texture_uv.npy"))
    assert crc(uv) == g["uv"]
    rgb = orc.texture_sample(tex, uv)
    assert crc(rgb) == g["rgb"] == g["albedo"]


def deform(p):
    """vertex animation stand-in (same as tests/golden/make_golden.py): p + 0.1 * (p.yzx * p.zxy), float32 products and sums only"""
    p = np.asarray(p, np.float32)
    return (p + np.float32(0.1) * (p[..., [1, 2, 0]] * p[..., [2, 0, 1]])).astype(np.float32)


@pytest.mark.parametrize("mesh", sorted(G["ref_refit"].keys()))
def test_oracle_refit_matches_reference_golden(orc, mesh):
    """BVH::Refit (infra/bvh.cpp:26-43) of the real reference after moving the vertices, incl. its skipped node 1"""
    o = simple_scene(orc, mesh)
    t = o.bvh(0)["tris"]
    moved = deform(np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1))
    assert crc(moved) == G["ref_refit"][mesh]["moved"]
    o.move_and_refit(0, moved)
    b = o.bvh(0)
    assert crc(b["nodes"]) == G["ref_refit"][mesh]["nodes"]
    assert np.array_equal(b["tris"]["vertex1"], moved[:, 1])


# ---------------------------------------------------------------------------------------------------------------
# live comparison with the real reference: oracle/_ref where it is built, elsewhere the outputs it gave for the same inputs
# (tests/golden/ref_live.json: shape + CRC32 per output; ref_live_masks.npz: the ray masks the comparisons are restricted to)
# ---------------------------------------------------------------------------------------------------------------
LIVE_JSON = os.path.join(GOLDEN, "ref_live.json")
LIVE_NPZ = os.path.join(GOLDEN, "ref_live_masks.npz")


def _canon(a, nan_any=False):
    """the bits an output is compared by: raw bytes of records, the bit patterns of floats (nan_any: every NaN as one pattern), the values of integers"""
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        return a.view(np.uint8)
    if a.dtype.kind == "f":
        a = a.view(np.uint32 if a.itemsize == 4 else np.uint64)
        return np.where((a & 0x7fffffff) > 0x7f800000, np.uint32(0x7fc00000), a) if nan_any else a
    return a.astype(np.int64)


class LiveRef:
    """`ref` is the real reference's library (oracle/_ref) where it is built, else None.  check() compares an output of the oracle with the
    reference's bit for bit: live when the library is there (and then also with the recording, which must not go stale), otherwise with the
    recorded shape + CRC32 of the reference's output for the same inputs.  CRT_RECORD_REF_LIVE=1 with oracle/_ref built re-records."""

    def __init__(self, ref, recording):
        self.ref, self.recording = ref, recording
        self.crcs = json.load(open(LIVE_JSON)) if os.path.exists(LIVE_JSON) or not recording else {}
        self.arrays = dict(np.load(LIVE_NPZ)) if os.path.exists(LIVE_NPZ) or not recording else {}

    def _keep(self, store, key, value, same):
        if self.recording:
            store[key] = value
        else:
            assert same(store[key], value), "%s: tests/golden/ref_live* is stale (re-record with CRT_RECORD_REF_LIVE=1)" % key

    def check(self, key, mine, theirs=None, nan_any=False):
        m = _canon(mine, nan_any)
        if self.ref is None:
            assert self.crcs[key] == [list(m.shape), crc(m)], key
            return
        t = _canon(theirs, nan_any)
        assert m.shape == t.shape and np.array_equal(m, t), key
        self._keep(self.crcs, key, [list(t.shape), crc(t)], lambda x, y: x == y)

    def mask(self, key, theirs=None):
        """a boolean ray mask of the reference's (which rays hit the mesh): live, or as recorded"""
        if self.ref is None:
            return self.arrays[key]
        self._keep(self.arrays, key, theirs, np.array_equal)
        return theirs


@pytest.fixture(scope="module")
def live(orc):
    try:
        ref = orc.Ref()
    except FileNotFoundError:
        ref = None
    lr = LiveRef(ref, ref is not None and os.environ.get("CRT_RECORD_REF_LIVE") == "1")
    yield lr
    if lr.recording:
        with open(LIVE_JSON, "w") as f:
            json.dump(lr.crcs, f, indent=1, sort_keys=True)
        np.savez_compressed(LIVE_NPZ, **lr.arrays)


def test_oracle_camera_and_texture_vs_reference_live(orc, live):
    ref = live.ref
    rng = np.random.default_rng(3)
    xy = rng.uniform(-2, [1026, 642], (4000, 2)).astype(np.float32)
    live.check("camera_xy", xy, xy)                 # (the inputs: the recorded outputs belong to these)
    for i, pt in enumerate((None, ((0.5, 1.25, -3.0), (0.0, 0.0, 2.0)), ((-2.0, 3.0, 1.0), (0.0, -1.0, 2.5)))):
        corners, O, D = ref.camera_rays(xy, pt) if ref else (None, None, None)
        o = camera_oracle(orc, pt)
        live.check("camera%d_corners" % i, np.stack(o.camera()), corners)
        oO, oD = o.primary_rays(xy)
        live.check("camera%d_O" % i, oO, O)
        live.check("camera%d_D" % i, oD, D)
    for f in ("textures/Stylized_Pavement_basecolor.png", "textures/Stylized_Wood_basecolor.tga", "textures/Defuse_wok.png"):
        live.check("texture_load " + f, orc.pack_rgb(orc.read_image(os.path.join(ASSETS, f))), ref.texture_load(os.path.join(ASSETS, f)) if ref else None)
    uv = rng.uniform(-0.5, 1.5, (20000, 2)).astype(np.float32)
    small = rng.integers(0, 1 << 24, (37, 53)).astype(np.uint32)
    live.check("texture_uv", uv, uv)
    live.check("texture_small", small, small)
    pavement = orc.pack_rgb(orc.read_image(os.path.join(ASSETS, "textures/Stylized_Pavement_basecolor.png")))     # = Texture::LoadFromFile's texels (checked above)
    for name, tex in (("pavement", pavement), ("small", small)):
        rgb, alb = ref.texture_sample(tex, uv) if ref else (None, None)
        mine = orc.texture_sample(tex, uv)
        live.check("texture_sample %s rgb" % name, mine, rgb)
        live.check("texture_sample %s albedo" % name, mine, alb)


@pytest.mark.parametrize("mesh", ["bunny", "wok"])
def test_oracle_refit_vs_reference_live(orc, live, mesh):
    ref = live.ref
    o = simple_scene(orc, mesh)
    t = o.bvh(0)["tris"]
    live.check("refit %s tris" % mesh, t, t)
    moved = deform(np.stack([t["vertex0"], t["vertex1"], t["vertex2"]], axis=1))
    rn = None
    if ref:
        h, _ = ref.bvh_build(t)
        try:
            rn = ref.bvh_move_and_refit(h, moved)
        finally:
            ref.bvh_free(h)
    o.move_and_refit(0, moved)
    live.check("refit %s nodes" % mesh, o.bvh(0)["nodes"], rn)


@pytest.mark.parametrize("mesh", ["bunny", "wok", "teapot"])
def test_oracle_vs_reference_live(orc, live, mesh):
    ref = live.ref
    o = simple_scene(orc, mesh)
    b = o.bvh(0)
    live.check("bvh %s tris" % mesh, b["tris"], b["tris"])
    rng = np.random.default_rng(99)
    n = 20000
    O = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    O[:, 1] = np.abs(O[:, 1]) + 0.2
    T = rng.uniform(-1, 1, (n, 3)).astype(np.float32) + np.array([0, -0.3, 2], np.float32)
    D = T - O
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(np.float32)
    live.check("bvh %s rays" % mesh, np.concatenate([O, D], axis=1), np.concatenate([O, D], axis=1))
    rb = rh = None
    if ref:
        h, rb = ref.bvh_build(b["tris"])
        try:
            rh = ref.bvh_intersect(h, O, D)
        finally:
            ref.bvh_free(h)
    live.check("bvh %s nodesUsed maxDepth" % mesh, np.array([b["nodesUsed"], b["maxDepth"]]), np.array([rb["nodesUsed"], rb["maxDepth"]]) if rb else None)
    live.check("bvh %s nodes" % mesh, b["nodes"], rb["nodes"] if rb else None)
    live.check("bvh %s triIndices" % mesh, b["triIndices"], rb["triIndices"] if rb else None)
    oh = o.find_nearest(O, D)
    both = (oh["objIdx"] >= 2) & live.mask("bvh_%s_mesh_hits" % mesh, None if rh is None else rh["objIdx"] >= 2)
    assert both.sum() > 1000
    for f in ("t", "u", "v", "triIdx"):
        live.check("bvh %s %s" % (mesh, f), oh[f][both], None if rh is None else rh[f][both])


def test_python_readers_vs_reference_live(orc, live):
    ref = live.ref
    for m in MESHES:
        p = os.path.join(ASSETS, m + ".obj")
        for name, a, b in zip(("pos", "nrm", "uv"), orc.read_obj(p), ref.obj_load(p) if ref else (None, None, None)):
            live.check("obj %s %s" % (m, name), a, b)
    for f in G["ref_img"]:
        live.check("image " + f, orc.read_image(os.path.join(ASSETS, f)), ref.image_load(os.path.join(ASSETS, f)) if ref else None)


# ---------------------------------------------------------------------------------------------------------------
# oracle regression vectors (integrator etc.: no executable reference exists — "parity unpinned")
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G["orc_render"].keys()))
def test_oracle_render_regression(orc, name):
    g = G["orc_render"][name]
    o, _ = orc.load_scene(scene_path(g["xml"]), g["kind"], ASSETS)
    o.renderer_init(g["W"], g["H"])
    o.render(g["frames"], 2)
    acc = o.accumulator()
    assert np.array_equal(acc, np.load(os.path.join(GOLDEN, "orc_render_%s.npy" % name)))
    assert crc(acc) == g["acc"] and crc(o.screen()) == g["screen"]
    assert o.counters() == g["counters"]
    assert float(np.float32(o.energy())) == g["energy"]
    seeds = [o.tile_seed(g["frames"], t) for t in range((g["W"] // 16) * (g["H"] // 16))]
    assert crc(np.array(seeds, np.uint32)) == g["last_frame_tile_seeds"]


def test_oracle_thread_count_invariance(orc):
    """renderer.cpp:120 seeds one stream per (tile, frame): the image cannot depend on the tile schedule."""
    res = []
    for threads in (1, 5):
        o, _ = orc.load_scene(scene_path("bunny_scene.xml"), 0, ASSETS)
        o.renderer_init(80, 64)
        o.render(3, threads)
        res.append(o.accumulator())
    assert np.array_equal(res[0], res[1])


def test_whitted_config1_regression(orc):
    """BASELINE config 1: cube.obj FileScene, Whitted-style, 640x360, CPU reference path (plumbing, no GPU)."""
    o, _ = orc.load_scene(scene_path("cube_scene.xml"), 0, ASSETS)
    o.renderer_init(640, 360)
    o.whitted(4)
    g = G["orc_whitted_cube_640x360"]
    acc = o.accumulator()
    assert np.isfinite(acc).all() and acc[..., :3].max() > 0.5
    assert crc(acc) == g["acc"] and crc(o.screen()) == g["screen"] and o.counters() == g["counters"]


# ---------------------------------------------------------------------------------------------------------------
# small known-answer checks of the restated primitives
# ---------------------------------------------------------------------------------------------------------------
def test_rng_known_answers(orc):
    L = orc.lib()

    def wang(s):
        s = ((s ^ 61) ^ (s >> 16)) & 0xffffffff
        s = (s * 9) & 0xffffffff
        s ^= s >> 4
        s = (s * 0x27d4eb2d) & 0xffffffff
        s ^= s >> 15
        return s
    for base in (0, 1, 1799, 123456789, 0xffffffff):
        assert L.orc_init_seed(base) == wang(((base + 1) * 17) & 0xffffffff)
    import ctypes as C
    s = C.c_uint32(0x12345678)
    x = 0x12345678
    for _ in range(100):
        x ^= (x << 13) & 0xffffffff
        x ^= x >> 17
        x ^= (x << 5) & 0xffffffff
        assert L.orc_random_uint(C.byref(s)) == x and s.value == x


def test_deterministic_math_accuracy(orc):
    """crt_expf / crt_atan2f / crt_acosf are the path's only transcendental functions (absorption, skydome lookup);
    they must stay within a few ulp of the correctly rounded result."""
    L = orc.lib()
    rng = np.random.default_rng(5)

    def ulps(got, want):
        got = np.asarray(got, np.float32)
        want32 = want.astype(np.float32)
        sp = np.spacing(np.abs(want32)).astype(np.float64)
        return np.abs(got.astype(np.float64) - want) / np.maximum(sp, 1e-45)
    x = np.concatenate([rng.uniform(-40, 0, 4000), rng.uniform(-90, 80, 2000), [0.0, -0.0, -1e-8]]).astype(np.float32)
    e = np.array([L.orc_expf(float(v)) for v in x], np.float32)
    assert ulps(e, np.exp(x.astype(np.float64))).max() <= 2.0
    assert L.orc_expf(0.0) == 1.0 and L.orc_expf(-0.0) == 1.0
    y = rng.uniform(-1, 1, 6000).astype(np.float32)
    xx = rng.uniform(-1, 1, 6000).astype(np.float32)
    a = np.array([L.orc_atan2f(float(p), float(q)) for p, q in zip(y, xx)], np.float32)
    assert np.abs(a.astype(np.float64) - np.arctan2(y.astype(np.float64), xx.astype(np.float64))).max() <= 6e-7
    c = np.concatenate([rng.uniform(-1, 1, 6000), [1.0, -1.0, 0.0, 0.5, -0.5]]).astype(np.float32)
    ac = np.array([L.orc_acosf(float(v)) for v in c], np.float32)
    assert np.abs(ac.astype(np.float64) - np.arccos(c.astype(np.float64))).max() <= 6e-7
    assert L.orc_atan2f(0.0, -1.0) == np.float32(np.pi) and L.orc_atan2f(0.0, 1.0) == 0.0


def test_reference_struct_sizes(orc):
    assert orc.TRI_DTYPE.itemsize == 112 and orc.NODE_DTYPE.itemsize == 32 and orc.TLAS_DTYPE.itemsize == 32


# ---------------------------------------------------------------------------------------------------------------
# template/tmplmath.h inline functions on the path + infra/helper.h's Vertex table: pinned to the
# real reference through oracle/_ref (ref_math_probe / ref_vertex_dedup) and its committed outputs tests/golden/ref_math.npz, ref_vertex.npz
# ---------------------------------------------------------------------------------------------------------------
MATH_FIELDS = [("normalize", 0, 3), ("reflect", 3, 6), ("cross", 6, 9), ("dot", 9, 10), ("mat4::Translate", 10, 26), ("mat4::RotateX", 26, 42),
               ("mat4::RotateY", 42, 58), ("mat4::RotateZ", 58, 74), ("mat4::Scale", 74, 90), ("FastInvertedTransformNoScale", 90, 106),
               ("aabb::Grow(float3) / Area", 106, 113), ("aabb::Grow(aabb) / Area", 113, 120)]


from probe_inputs import same_bits as _same_bits          # bit equality, any NaN matches any NaN: one definition for every bit-exact test


@pytest.mark.parametrize("who", ["oracle", "host_front"])
def test_tmplmath_inlines_match_reference_golden(orc, who):
    z = np.load(os.path.join(GOLDEN, "ref_math.npz"))
    assert crc(z["outputs"]) == G["ref_math"]["outputs"] and len(z["inputs"]) == G["ref_math"]["rows"]
    if who == "oracle":
        got = orc.math_probe(z["inputs"])
    else:
        from conftest import load_crt
        got = load_crt().host_math_probe(z["inputs"])
    for name, a, b in MATH_FIELDS:
        assert _same_bits(got[:, a:b], z["outputs"][:, a:b]), name


@pytest.mark.parametrize("who", ["oracle", "host_front"])
def test_vertex_table_matches_reference_golden(orc, who):
    """Vertex::operator== is float equality (+0 == -0: the first occurrence's bits are kept; a NaN vertex equals nothing and model.cpp:50's second
    lookup then yields index 0): corner indices and the unique-vertex array of the real std::unordered_map<Vertex, uint32_t>"""
    z = np.load(os.path.join(GOLDEN, "ref_vertex.npz"))
    assert crc(z["idx"]) == G["ref_math"]["vertex_idx"] and len(z["unique"]) == G["ref_math"]["vertex_unique"]
    if who == "oracle":
        idx, uniq = orc.vertex_dedup(z["corners"])
    else:
        from conftest import load_crt
        idx, uniq = load_crt().host_vertex_dedup(z["corners"])
    assert np.array_equal(idx, z["idx"])
    assert uniq.shape == z["unique"].shape and _same_bits(uniq, z["unique"])


def test_tmplmath_and_vertex_live(orc, live):
    """the same probes against oracle/_ref (or what it gave, recorded) on fresh random inputs"""
    ref = live.ref
    rng = np.random.default_rng(5)
    x = rng.uniform(-10, 10, (3000, 12)).astype(np.float32)
    live.check("math inputs", x, x)
    live.check("math_probe", orc.math_probe(x), ref.math_probe(x) if ref else None, nan_any=True)
    v = np.round(rng.uniform(-1, 1, (4000, 8)) * 4).astype(np.float32) / 4          # many exact duplicates, +0 and -0
    live.check("vertex inputs", v, v)
    i1, u1 = orc.vertex_dedup(v)
    i2, u2 = ref.vertex_dedup(v)[:2] if ref else (None, None)
    live.check("vertex_dedup idx", i1, i2)
    live.check("vertex_dedup unique", u1, u2, nan_any=True)


def test_sky_lookup_deviation_from_libm_is_bounded(orc):
    """GetSkyColor (file_scene.cpp:142-154) calls libm's atan2 / acos, the path here its own deterministic polynomials (so that x86 and gfx950
    agree bit for bit).  The two differ in the last ulp of phi / theta, which moves the nearest-texel index (int)(u * w) only when u * w lands within
    that ulp of an integer.  This test measures how often, on a 4096 x 2048 skydome: DESIGN.md quotes the bound."""
    L = orc.lib()
    rng = np.random.default_rng(11)
    n = 200000
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    PI, INV2PI, INVPI = np.float32(3.14159265358979323846264), np.float32(0.15915494309189533576888), np.float32(0.31830988618379067153777)
    phi_det = np.array([L.orc_atan2f(float(-z), float(x)) for x, z in zip(d[:, 0], d[:, 2])], np.float32) + PI
    th_det = np.array([L.orc_acosf(float(-y)) for y in d[:, 1]], np.float32)
    phi_lm = np.arctan2(-d[:, 2].astype(np.float64), d[:, 0].astype(np.float64)).astype(np.float32) + PI      # correctly rounded = what a good libm returns
    th_lm = np.arccos(-d[:, 1].astype(np.float64)).astype(np.float32)
    W, H = 4096, 2048

    def texel(phi, th):
        u = np.clip(phi * INV2PI, 0, 1); v = np.float32(1) - np.clip(th * INVPI, 0, 1)
        return np.clip((u * np.float32(W)).astype(np.int32), 0, W - 1), np.clip((v * np.float32(H)).astype(np.int32), 0, H - 1)
    xd, yd = texel(phi_det, th_det); xl, yl = texel(phi_lm, th_lm)
    flips = int(((xd != xl) | (yd != yl)).sum())
    assert np.abs(xd - xl).max() <= 1 and np.abs(yd - yl).max() <= 1          # never more than the neighbouring texel
    assert flips <= n * 5e-4, flips                                           # measured: 11 of 200 000 directions (1 in 18 000) at this resolution
    assert np.abs(phi_det.astype(np.float64) - phi_lm).max() <= 6e-7 and np.abs(th_det.astype(np.float64) - th_lm).max() <= 6e-7   # <= 2.5 ulp at pi
    print("sky texel flips vs libm: %d of %d (%.4f %%)" % (flips, n, 100.0 * flips / n))


# ---------------------------------------------------------------------------------------------------------------
# FileScene's alternative accelerators: KDTree (infra/kdtree.cpp) and Grid (infra/grid.cpp), pinned to the real reference
# (both files compile unmodified in oracle/_ref): structure CRCs in golden.json "ref_alt", the reference's own hits in ref_alt_rays.npz
# ---------------------------------------------------------------------------------------------------------------
def _alt_matches(d, g, kind):
    if kind == "kd":
        return (crc(d["nodes"]), crc(d["refs"]), len(d["nodes"]), len(d["refs"]), d["maxDepth"], d["nodesUsed"]) == (g["nodes"], g["refs"], g["nodeCount"], g["refCount"], g["maxDepth"], g["nodesUsed"])
    return ([int(x) for x in d["resolution"]], crc(d["cellSize"]), crc(d["boundsMin"]), crc(d["boundsMax"]), crc(d["cellStart"]), crc(d["refs"])) == \
           (g["resolution"], g["cellSize"], g["boundsMin"], g["boundsMax"], g["cellStart"], g["refs"])


@pytest.mark.parametrize("kind", ["kd", "grid"])
@pytest.mark.parametrize("mesh", ["bunny", "teapot", "cube"])
def test_oracle_alt_accel_matches_reference_golden(orc, mesh, kind):
    tris = simple_scene(orc, mesh).bvh(0)["tris"]
    a = orc.alt_accel(kind, tris)
    assert _alt_matches(a.dump(), G["ref_alt"][mesh][kind], kind)
    z = np.load(os.path.join(GOLDEN, "ref_bvh_rays.npz")); r = np.load(os.path.join(GOLDEN, "ref_alt_rays.npz"))
    h = a.intersect(z[mesh + "_O"], z[mesh + "_D"])
    a.close()
    for f in ("t", "u", "v"):
        assert np.array_equal(h[f].view(np.uint32), r["%s_%s_%s" % (mesh, kind, f)].view(np.uint32)), f
    for f in ("objIdx", "triIdx", "traversed", "tested"):
        assert np.array_equal(h[f], r["%s_%s_%s" % (mesh, kind, f)]), f


@pytest.mark.parametrize("kind,code", [("kd", 1), ("grid", 2)])
@pytest.mark.parametrize("mesh", ["bunny", "cube"])
def test_host_front_alt_accel_build_matches_reference_golden(tmp_path, mesh, kind, code):
    from conftest import load_crt
    from test_gpu_golden_and_edges import write_scene as write_simple_scene
    crt = load_crt()
    hs = crt.HostScene(write_simple_scene(tmp_path, mesh), 0, ASSETS)
    assert _alt_matches(hs.build_alt(code), G["ref_alt"][mesh][kind], kind)


def test_alt_accel_live(orc, live):
    """oracle vs the real kdtree.cpp / grid.cpp (or what they gave, recorded) on a mesh and rays the goldens do not cover"""
    ref = live.ref
    tris = simple_scene(orc, "log_fence").bvh(0)["tris"]
    live.check("alt tris", tris, tris)
    rng = np.random.default_rng(9)
    O = rng.uniform(-3, 3, (2000, 3)).astype(np.float32); O[:, 1] = np.abs(O[:, 1]) + 0.1
    D = (np.array([0, -0.5, 2], np.float32) + rng.uniform(-1, 1, (2000, 3)).astype(np.float32)) - O
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(np.float32)
    D[:20, 0] = 0; D[20:40, 1] = 0; D[40:60, 2] = 0                   # axis-parallel components: infinite reciprocal, NaN plane distances
    live.check("alt rays", np.concatenate([O, D], axis=1), np.concatenate([O, D], axis=1))
    for kind in ("kd", "grid"):
        b = orc.alt_accel(kind, tris)
        db, hb = b.dump(), b.intersect(O, D)
        b.close()
        da = ha = None
        if ref:
            a = ref.alt_accel(kind, tris)
            da, ha = a.dump(), a.intersect(O, D)
            a.close()
            assert sorted(da) == sorted(db)
        for k in sorted(db):
            live.check("alt %s %s" % (kind, k), np.asarray(db[k]), None if da is None else np.asarray(da[k]))
        for f in hb.dtype.names:
            live.check("alt %s hit %s" % (kind, f), hb[f], None if ha is None else ha[f])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the light quad and floor plane of a look (orc_set_light_quad / orc_set_floor_uv_scale) against the reference's own Quad and Plane
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["cube", "tlas"])
def test_oracle_quad_and_plane_vs_reference_classes(orc, scene):
    """Quad(0, 2 * size, T) and Plane(1, (0, 1, 0), 1, width / 100) of the reference, compiled in place, against the oracle's QuadPrim with the cells
    set_light_quad takes and its PlanePrim with set_floor_uv_scale's factor, bit for bit: Intersect, IsOccluded, GetNormal, GetUV, the constructor's invT and
    size, and GetLightPos's expression, for every transform and size of render_looks_inputs on the rays of light_quad_inputs (the exact ones included)"""
    import light_quad_inputs as lq
    import mesh_truth as mt
    import mesh_truth_scenes as MC
    import render_looks_inputs as li
    try:
        ref = orc.Ref()
    except FileNotFoundError:
        pytest.skip("oracle/_ref is not built (no reference tree on this machine)")
    if not (ref.has("ref_quad_probe") and ref.has("ref_plane_probe")):
        pytest.skip("oracle/_ref was built from an earlier harness and the reference tree is gone: nothing to rebuild it from")
    xml, kind = li.SCENES[scene]
    o, _ = orc.load_scene(li.scene_path(xml), kind, ASSETS)
    _, light, obj_mat, invto = MC.describe(orc, li.scene_path(xml))
    T0 = li.translate(np.asarray(light, np.float32))
    base = dict(light_T=T0.reshape(16), light_invT=li.inverse_no_scale(T0).reshape(16), light_size=0.5)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)                # noqa: E731
    looks = dict(li.quad_looks(scene, base), base=base)
    for name, look in looks.items():
        T = np.asarray(look["light_T"], np.float32).reshape(4, 4); size = look["light_size"]
        w = mt.world_of(o, kind, light, obj_mat, invto, light_T=T, light_half=size)
        O, D, given, cls = lq.make_rays(w, 1024, seed=7)
        tmax = np.where(np.isnan(given), np.float32(3.0), given).astype(np.float32)
        if name in ("quarter_z", "half_x"):
            eO, eD = lq.exact_rays(T, size, 5)
            O, D, tmax = np.concatenate([O, eO]), np.concatenate([D, eD]), np.concatenate([tmax, np.full(len(eO), 3.0, np.float32)])
        theirs = ref.quad_probe(T, size, O, D, tmax)
        assert np.array_equal(bits(theirs["invT"]), bits(li.inverse_no_scale(T))) and theirs["size"] == np.float32(size), name      # what a look's record carries
        mine = orc.quad_probe(T, look["light_invT"], size, O, D, tmax)
        for k in ("t", "objIdx", "occluded", "normal"):
            assert np.array_equal(bits(mine[k]), bits(theirs[k])), (scene, name, k)
        assert (theirs["objIdx"] == 0).sum() >= 300 and (theirs["objIdx"] == -1).sum() >= 200 and 100 <= theirs["occluded"].sum() <= len(O) - 100, name
        o.set_light_quad(T, look["light_invT"], size)                       # ... and the scene's own quad is that QuadPrim
        q = o.light()
        assert np.array_equal(bits(q["pos"]), bits(theirs["pos"])) and np.array_equal(bits(q["normal"]), bits(theirs["normal"])), (scene, name)
        lit = o.find_nearest(O, D)
        m = lit["objIdx"] == 0
        assert m.sum() >= 250 and (theirs["objIdx"][m] == 0).all() and np.array_equal(bits(lit["t"][m]), bits(theirs["t"][m])), (scene, name)
    # the floor: the file's own scale, another texture's, and one no texture width gives
    for offset in (5, 10, 40, 7.5):
        theirs = ref.plane_probe(offset, O, D)
        mine = orc.plane_probe(theirs["invto"], O, D)
        assert theirs["invto"] == np.float32(1.0) / np.float32(offset) and (theirs["objIdx"] == 1).sum() >= 200
        for k in ("t", "objIdx", "uv"):
            assert np.array_equal(bits(mine[k]), bits(theirs[k])), (offset, k)
    o.set_floor_uv_scale(np.float32(1.0) / np.float32(7.5))
    assert o.light()["floor_invto"] == ref.plane_probe(7.5, O[:1], D[:1])["invto"]
