"""
orc.py — Python (ctypes) binding of the CPU oracle + independent pure-Python asset readers.

TEST INFRASTRUCTURE ONLY: importable from tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg.
The product package (cpu-ray-tracer_amd/) never imports this module.

The readers here (OBJ, scene XML, PNG/TGA) are deliberately independent of the product's C++ loaders so
that a parsing bug cannot hide by being shared between the checker and the thing checked.
"""
import ctypes as C
import os
import struct
import subprocess
import xml.etree.ElementTree as ET
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libcrt_oracle.so")
REF_LIB_PATH = os.path.join(HERE, "_ref", "libcrt_ref.so")
# the entry point ref_harness.cpp gained last: whoever adds an export there names it here, or a library kept from before the addition is taken for current
REF_NEWEST_SYMBOL = b"ref_plane_probe"


def build(force=False):
    """Compile the oracle (g++) and, when /root/reference exists, oracle/_ref (the real reference, in place)."""
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < os.path.getmtime(os.path.join(HERE, "crt_oracle.cpp")):
        subprocess.check_call(["make", "-C", HERE, "libcrt_oracle.so"])
    ref_src = [os.path.join(HERE, "ref_build", "ref_harness.cpp"), os.path.join(HERE, "ref_build", "precomp.h"), os.path.join(HERE, "Makefile")]
    # (a library left by an earlier build of another harness lacks the entry points this one declares: rebuilt whenever a source of it is newer)
    def stale():
        if os.path.getmtime(REF_LIB_PATH) < max(os.path.getmtime(f) for f in ref_src):
            return True
        with open(REF_LIB_PATH, "rb") as f:                                 # (looked for in the file: a dlopen would pin the old image for this process)
            return REF_NEWEST_SYMBOL not in f.read()
    if os.path.isdir("/root/reference") and (force or not os.path.exists(REF_LIB_PATH) or stale()):
        subprocess.check_call(["make", "-B", "-C", HERE, "ref"])


class BvhNode(C.Structure):
    _fields_ = [("aabbMin", C.c_float * 3), ("aabbMax", C.c_float * 3), ("leftFirst", C.c_uint32), ("triCount", C.c_uint32)]


class TlasNode(C.Structure):
    _fields_ = [("aabbMin", C.c_float * 3), ("leftRight", C.c_uint32), ("aabbMax", C.c_float * 3), ("BLAS", C.c_uint32)]


class RayIn(C.Structure):
    _fields_ = [("O", C.c_float * 3), ("D", C.c_float * 3), ("inside", C.c_int32)]


class Hit(C.Structure):
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("objIdx", C.c_int32), ("triIdx", C.c_int32),
                ("traversed", C.c_int32), ("tested", C.c_int32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rays", "primary", "interior_iters", "leaf_iters", "tri_tests", "tlas_iters", "blas_visits", "mesh_hits")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


TRI_DTYPE = np.dtype([("vertex0", "<f4", 3), ("vertex1", "<f4", 3), ("vertex2", "<f4", 3),
                      ("normal0", "<f4", 3), ("normal1", "<f4", 3), ("normal2", "<f4", 3),
                      ("uv0", "<f4", 2), ("uv1", "<f4", 2), ("uv2", "<f4", 2),
                      ("centroid", "<f4", 3), ("objIdx", "<i4")])
NODE_DTYPE = np.dtype([("aabbMin", "<f4", 3), ("aabbMax", "<f4", 3), ("leftFirst", "<u4"), ("triCount", "<u4")])
TLAS_DTYPE = np.dtype([("aabbMin", "<f4", 3), ("leftRight", "<u4"), ("aabbMax", "<f4", 3), ("BLAS", "<u4")])
RAY_DTYPE = np.dtype([("O", "<f4", 3), ("D", "<f4", 3), ("inside", "<i4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("objIdx", "<i4"), ("triIdx", "<i4"), ("traversed", "<i4"), ("tested", "<i4")])
assert TRI_DTYPE.itemsize == 112 and NODE_DTYPE.itemsize == 32 and TLAS_DTYPE.itemsize == 32

_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB_PATH)
        L.orc_create.restype = C.c_void_p
        L.orc_create.argtypes = [C.c_int]
        L.orc_last_error.restype = C.c_char_p
        L.orc_accumulator.restype = C.POINTER(C.c_float)
        L.orc_screen.restype = C.POINTER(C.c_uint32)
        L.orc_energy.restype = C.c_float
        for n in ("orc_expf", "orc_acosf"):
            getattr(L, n).restype = C.c_float
            getattr(L, n).argtypes = [C.c_float]
        L.orc_atan2f.restype = C.c_float
        L.orc_atan2f.argtypes = [C.c_float, C.c_float]
        L.orc_init_seed.restype = C.c_uint32
        L.orc_init_seed.argtypes = [C.c_uint32]
        L.orc_random_uint.restype = C.c_uint32
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(C.c_void_p)


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


class Oracle:
    """One scene (FileScene kind=0 / TLASFileScene kind=1) + Renderer state."""

    def __init__(self, kind):
        self.L = lib()
        self.h = C.c_void_p(self.L.orc_create(int(kind)))
        self.kind = int(kind)
        self.W = self.H = 0

    def __del__(self):
        try:
            if self.h:
                self.L.orc_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _ck(self, r):
        if r != 0:
            raise RuntimeError("oracle: " + self.L.orc_last_error(self.h).decode())

    # --- scene description -------------------------------------------------------------------
    def set_light_position(self, p):
        self._ck(self.L.orc_set_light_position(self.h, _f3(p)))

    def set_light_quad(self, T, invT, size):
        """the light as Quad(0, 2 * size, T): both matrices cell for cell (16 float32 each, row-major), instead of Translate(light position) and size 0.5; kept across build()"""
        T = np.ascontiguousarray(T, np.float32).reshape(16); invT = np.ascontiguousarray(invT, np.float32).reshape(16)
        self._ck(self.L.orc_set_light_quad(self.h, _fp(T), _fp(invT), C.c_float(size)))

    def set_floor_uv_scale(self, invto):
        """the floor plane's uv scale (Plane::invto) instead of 1 / (floor texture width // 100); kept across build()"""
        self._ck(self.L.orc_set_floor_uv_scale(self.h, C.c_float(invto)))

    def light(self):
        """the built scene's quad and floor scale: dict(T, invT, size, normal = Quad::GetNormal, pos = GetLightPos(), floor_invto)"""
        T, invT, n, p = np.zeros(16, np.float32), np.zeros(16, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        size, invto = C.c_float(), C.c_float()
        self._ck(self.L.orc_get_light(self.h, _fp(T), _fp(invT), C.byref(size), _fp(n), _fp(p), C.byref(invto)))
        return dict(T=T.reshape(4, 4), invT=invT.reshape(4, 4), size=np.float32(size.value), normal=n, pos=p, floor_invto=np.float32(invto.value))

    def set_floor_texture(self, rgb):
        rgb = np.ascontiguousarray(rgb, dtype=np.uint32)
        self._ck(self.L.orc_set_floor_texture(self.h, _fp(rgb), rgb.shape[1], rgb.shape[0]))

    def set_skydome(self, rgb):
        rgb = np.ascontiguousarray(rgb, dtype=np.uint32)
        self._ck(self.L.orc_set_skydome(self.h, _fp(rgb), rgb.shape[1], rgb.shape[0]))

    def add_material(self, reflectivity=0.0, refractivity=0.0, absorption=(0, 0, 0), texture=None):
        if texture is not None:
            texture = np.ascontiguousarray(texture, dtype=np.uint32)
            return self.L.orc_add_material(self.h, C.c_float(reflectivity), C.c_float(refractivity), _f3(absorption),
                                           _fp(texture), texture.shape[1], texture.shape[0])
        return self.L.orc_add_material(self.h, C.c_float(reflectivity), C.c_float(refractivity), _f3(absorption), None, 0, 0)

    def add_object(self, corners, position=(0, 0, 0), rotation=(0, 0, 0), scale=(1, 1, 1), material_idx=0):
        pos, nrm, uv = [np.ascontiguousarray(a, dtype=np.float32) for a in corners]
        n = pos.shape[0]
        r = self.L.orc_add_object(self.h, _fp(pos), _fp(nrm), _fp(uv), n, _f3(position), _f3(rotation), _f3(scale), int(material_idx))
        if r < 0:
            self._ck(r)
        return r

    def build(self):
        self._ck(self.L.orc_build(self.h))

    # --- introspection -----------------------------------------------------------------------
    def bvh_count(self):
        return self.L.orc_bvh_count(self.h)

    def bvh(self, i=0):
        nu, tc, md = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(self.L.orc_bvh_info(self.h, i, C.byref(nu), C.byref(tc), C.byref(md)))
        nodes = np.zeros(nu.value, NODE_DTYPE)
        idx = np.zeros(tc.value, np.uint32)
        tris = np.zeros(tc.value, TRI_DTYPE)
        self._ck(self.L.orc_bvh_copy(self.h, i, _fp(nodes), _fp(idx), _fp(tris)))
        return dict(nodes=nodes, triIndices=idx, tris=tris, nodesUsed=nu.value, maxDepth=md.value)

    def blas_transform(self, i):
        T = np.zeros(16, np.float32)
        invT = np.zeros(16, np.float32)
        lo = np.zeros(3, np.float32)
        hi = np.zeros(3, np.float32)
        self._ck(self.L.orc_blas_transform(self.h, i, _fp(T), _fp(invT), _fp(lo), _fp(hi)))
        return T, invT, lo, hi

    def set_transform(self, i, T):
        """BLASBVH::SetTransform(T) of instance i + TLASBVH::Build"""
        T = np.ascontiguousarray(T, np.float32).reshape(16)
        self._ck(self.L.orc_set_blas_transform(self.h, int(i), _fp(T)))

    def move_and_refit(self, i, positions):
        positions = np.ascontiguousarray(positions, np.float32)
        self._ck(self.L.orc_bvh_move_and_refit(self.h, i, _fp(positions), C.c_uint32(positions.shape[0])))

    def tlas(self):
        n = self.bvh_count()
        nodes = np.zeros(2 * n, TLAS_DTYPE)
        nu = C.c_uint32()
        self._ck(self.L.orc_tlas_copy(self.h, _fp(nodes), C.byref(nu)))
        return nodes, nu.value

    # --- renderer ----------------------------------------------------------------------------
    def renderer_init(self, W, H):
        self._ck(self.L.orc_renderer_init(self.h, W, H))
        self.W, self.H = W, H

    def set_camera_state(self, pos, target):
        self._ck(self.L.orc_set_camera_state(self.h, _f3(pos), _f3(target)))

    def camera(self):
        a = [np.zeros(3, np.float32) for _ in range(4)]
        self._ck(self.L.orc_get_camera(self.h, *[_fp(x) for x in a]))
        return a

    def primary_rays(self, xy):
        """Camera::GetPrimaryRay of the oracle for pixel coordinates xy (n, 2)"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        O = np.zeros((xy.shape[0], 3), np.float32); D = np.zeros((xy.shape[0], 3), np.float32)
        self._ck(self.L.orc_primary_rays(self.h, _fp(xy), C.c_size_t(xy.shape[0]), _fp(O), _fp(D)))
        return O, D

    def set_params(self, depth_limit=5, passes=1):
        self._ck(self.L.orc_set_params(self.h, depth_limit, passes))

    def clear(self):
        self._ck(self.L.orc_clear(self.h))

    def set_spp(self, spp):
        self._ck(self.L.orc_set_spp(self.h, spp))

    def spp(self):
        return self.L.orc_get_spp(self.h)

    def set_tile_range(self, first, count):
        self._ck(self.L.orc_set_tile_range(self.h, first, count))

    def render(self, frames, threads=1):
        self._ck(self.L.orc_render(self.h, frames, threads))

    def whitted(self, threads=1):
        self._ck(self.L.orc_whitted_render(self.h, threads))

    def accumulator(self):
        p = self.L.orc_accumulator(self.h)
        return np.ctypeslib.as_array(p, shape=(self.H, self.W, 4)).copy()

    def screen(self):
        p = self.L.orc_screen(self.h)
        return np.ctypeslib.as_array(p, shape=(self.H, self.W)).copy()

    def energy(self):
        return float(self.L.orc_energy(self.h))

    def counters(self):
        c = Counters()
        self._ck(self.L.orc_get_counters(self.h, C.byref(c)))
        return c.as_dict()

    def reset_counters(self):
        self._ck(self.L.orc_reset_counters(self.h))

    def tile_seed(self, spp, tile):
        s = C.c_uint32()
        self._ck(self.L.orc_tile_seed_after_frame(self.h, spp, tile, C.byref(s)))
        return s.value

    def find_nearest(self, O, D, inside=None):
        O = np.asarray(O, np.float32).reshape(-1, 3)
        D = np.asarray(D, np.float32).reshape(-1, 3)
        rays = np.zeros(O.shape[0], RAY_DTYPE)
        rays["O"], rays["D"] = O, D
        if inside is not None:
            rays["inside"] = inside
        hits = np.zeros(O.shape[0], HIT_DTYPE)
        self._ck(self.L.orc_find_nearest(self.h, _fp(rays), _fp(hits), C.c_size_t(O.shape[0])))
        return hits

    def is_occluded(self, O, D, t):
        """scene.IsOccluded(Ray(O, D, t)) per ray: the light quad bounded by t, then the structure with shadow.t = 1e34f (through the set of set_blas_accel, if any)"""
        O = np.ascontiguousarray(O, np.float32).reshape(-1, 3); D = np.ascontiguousarray(D, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, np.float32), (O.shape[0],)))
        out = np.zeros(O.shape[0], np.int32)
        self._ck(self.L.orc_is_occluded(self.h, _fp(O), _fp(D), _fp(t), _fp(out), C.c_size_t(O.shape[0])))
        return out

    def sample(self, O, D, seed, inside=0):
        r = np.zeros(1, RAY_DTYPE)
        r["O"], r["D"], r["inside"] = O, D, inside
        s = C.c_uint32(seed)
        rgb = np.zeros(3, np.float32)
        self._ck(self.L.orc_sample(self.h, _fp(r), C.byref(s), _fp(rgb)))
        return rgb, s.value


# ================================================================================================
# independent asset readers (pure Python / numpy)
# ================================================================================================
def texture_sample(texels, uv):
    """Texture::Sample of the oracle on (h, w) uint32 texels"""
    texels = np.ascontiguousarray(texels, np.uint32); uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    rgb = np.zeros((uv.shape[0], 3), np.float32)
    lib().orc_texture_sample(_fp(texels), texels.shape[1], texels.shape[0], _fp(uv), C.c_size_t(uv.shape[0]), _fp(rgb))
    return rgb


def read_obj(path):
    """OBJ -> (pos[n,3], nrm[n,3], uv[n,2]) per triangle corner, triangulated with tinyobjloader v2.0's rules
    (reference lib/tiny_obj_loader.h:1480-1700): triangles pass through, quads split along the shorter diagonal
    (strict <, float32 arithmetic), larger polygons are ear-clipped (see _earclip).  Missing vn / vt -> zeros."""
    V, VN, VT = [], [], []
    corners = []  # (vi, ti, ni) zero-based or -1
    with open(path, "r", errors="replace") as f:
        for line in f:
            s = line.split()
            if not s:
                continue
            k = s[0]
            if k == "v":
                V.append([float(s[1]), float(s[2]), float(s[3])])
            elif k == "vn":
                VN.append([float(s[1]), float(s[2]), float(s[3])])
            elif k == "vt":
                VT.append([float(s[1]), float(s[2]) if len(s) > 2 else 0.0])
            elif k == "f":
                face = []
                for tok in s[1:]:
                    parts = tok.split("/")

                    def fix(i, n):
                        i = int(i)
                        return i - 1 if i > 0 else n + i
                    vi = fix(parts[0], len(V))
                    ti = fix(parts[1], len(VT)) if len(parts) > 1 and parts[1] != "" else -1
                    ni = fix(parts[2], len(VN)) if len(parts) > 2 and parts[2] != "" else -1
                    face.append((vi, ti, ni))
                if len(face) < 3:
                    continue
                corners.append(face)
    V32 = np.asarray(V, np.float64).astype(np.float32).reshape(-1, 3)
    out = []
    for face in corners:
        n = len(face)
        if n == 3:
            out.extend(face)
        elif n == 4:
            p = [V32[c[0]] for c in face]
            e02 = p[2] - p[0]
            e13 = p[3] - p[1]
            s02 = np.float32(np.float32(e02[0] * e02[0] + e02[1] * e02[1]) + e02[2] * e02[2])
            s13 = np.float32(np.float32(e13[0] * e13[0] + e13[1] * e13[1]) + e13[2] * e13[2])
            if s02 < s13:
                out.extend([face[0], face[1], face[2], face[0], face[2], face[3]])
            else:
                out.extend([face[0], face[1], face[3], face[1], face[2], face[3]])
        else:
            for tri in _earclip(face, V32):
                out.extend(tri)
    n = len(out)
    VN32 = np.asarray(VN, np.float64).astype(np.float32).reshape(-1, 3)
    VT32 = np.asarray(VT, np.float64).astype(np.float32).reshape(-1, 2)
    pos = np.zeros((n, 3), np.float32)
    nrm = np.zeros((n, 3), np.float32)
    uv = np.zeros((n, 2), np.float32)
    vi = np.array([c[0] for c in out])
    ti = np.array([c[1] for c in out])
    ni = np.array([c[2] for c in out])
    pos[:] = V32[vi]
    m = ni >= 0
    nrm[m] = VN32[ni[m]]
    m = ti >= 0
    uv[m] = VT32[ti[m]]
    return pos, nrm, uv


def _earclip(face, V32):
    """tinyobjloader v2.0 built-in ear clipping for polygons with > 4 vertices
    (reference lib/tiny_obj_loader.h:1714-1935, the non-earcut path the reference compiles)."""
    f32 = np.float32
    npolys = len(face)
    axes = [1, 2]
    eps = np.finfo(np.float32).eps
    for k in range(npolys):
        v0 = V32[face[(k + 0) % npolys][0]]
        v1 = V32[face[(k + 1) % npolys][0]]
        v2 = V32[face[(k + 2) % npolys][0]]
        e0 = v1 - v0
        e1 = v2 - v1
        cx = abs(f32(f32(e0[1] * e1[2]) - f32(e0[2] * e1[1])))
        cy = abs(f32(f32(e0[2] * e1[0]) - f32(e0[0] * e1[2])))
        cz = abs(f32(f32(e0[0] * e1[1]) - f32(e0[1] * e1[0])))
        if cx > eps or cy > eps or cz > eps:
            if cx > cy and cx > cz:
                pass
            else:
                axes[0] = 0
                if cz > cx and cz > cy:
                    axes[1] = 1
            break
    a0, a1 = axes
    rem = list(face)
    tris = []
    guess = 0
    remaining_iter = len(face)
    prev_n = len(rem)
    while len(rem) > 3 and remaining_iter > 0:
        n = len(rem)
        if guess >= n:
            guess -= n
        if prev_n != n:
            prev_n = n
            remaining_iter = n
        else:
            remaining_iter -= 1
        ind = [rem[(guess + k) % n] for k in range(3)]
        vx = [V32[i[0]][a0] for i in ind]
        vy = [V32[i[0]][a1] for i in ind]
        e0x = f32(vx[1] - vx[0])
        e0y = f32(vy[1] - vy[0])
        e1x = f32(vx[2] - vx[1])
        e1y = f32(vy[2] - vy[1])
        cross = f32(f32(e0x * e1y) - f32(e0y * e1x))
        area = f32(f32(f32(vx[0] * vy[1]) - f32(vy[0] * vx[1])) * f32(0.5))
        if f32(cross * area) < 0:
            guess += 1
            continue
        overlap = False
        for other in range(3, n):
            idx = (guess + other) % n
            ov = V32[rem[idx][0]]
            if _pnpoly(vx, vy, ov[a0], ov[a1]):
                overlap = True
                break
        if overlap:
            guess += 1
            continue
        tris.append((ind[0], ind[1], ind[2]))
        del rem[(guess + 1) % n]
    if len(rem) == 3:
        tris.append((rem[0], rem[1], rem[2]))
    return tris


def _pnpoly(vx, vy, tx, ty):
    f32 = np.float32
    c = False
    j = 2
    for i in range(3):
        if (vy[i] > ty) != (vy[j] > ty):
            with np.errstate(divide="ignore", invalid="ignore"):
                x = f32(f32(f32(f32(vx[j] - vx[i]) * f32(ty - vy[i])) / f32(vy[j] - vy[i])) + vx[i])
            if tx < x:
                c = not c
        j = i
    return c


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def read_png(path):
    """Minimal PNG reader (8-bit gray / gray+alpha / RGB / RGBA / palette, non-interlaced) -> (h, w, n) uint8."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG"
    p = 8
    idat = b""
    plte = None
    while p < len(data):
        ln, typ = struct.unpack(">I4s", data[p:p + 8])
        body = data[p + 8:p + 8 + ln]
        p += 12 + ln
        if typ == b"IHDR":
            w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat += body
        elif typ == b"PLTE":
            plte = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif typ == b"IEND":
            break
    assert depth == 8 and interlace == 0, "unsupported PNG (depth %d, interlace %d)" % (depth, interlace)
    ch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    raw = np.frombuffer(zlib.decompress(idat), np.uint8)
    assert raw.size == h * (1 + w * ch), "PNG size mismatch"
    out = np.zeros(h * w * ch, np.uint8)
    rc = lib().orc_png_unfilter(_fp(np.ascontiguousarray(raw)), _fp(out), w * ch, h, ch)
    assert rc == 0, "bad PNG filter type"
    img = out.reshape(h, w, ch)
    if ctype == 3:
        img = plte[img[:, :, 0]]
    return img


def read_tga(path):
    """Uncompressed / RLE true-colour TGA (types 2, 10; 24/32 bpp) -> (h, w, n) uint8 RGB(A), top row first."""
    d = open(path, "rb").read()
    idlen, cmap, typ = d[0], d[1], d[2]
    w, h, bpp, desc = struct.unpack("<HHBB", d[12:18])
    assert cmap == 0 and typ in (2, 10) and bpp in (24, 32), "unsupported TGA"
    n = bpp // 8
    p = 18 + idlen
    if typ == 2:
        px = np.frombuffer(d, np.uint8, w * h * n, p).reshape(h, w, n)
    else:
        buf = bytearray()
        total = w * h * n
        while len(buf) < total:
            c = d[p]
            p += 1
            cnt = (c & 127) + 1
            if c & 128:
                buf += d[p:p + n] * cnt
                p += n
            else:
                buf += d[p:p + n * cnt]
                p += n * cnt
        px = np.frombuffer(bytes(buf[:total]), np.uint8).reshape(h, w, n)
    px = px[:, :, [2, 1, 0] + ([3] if n == 4 else [])]
    if not (desc & 0x20):
        px = px[::-1]
    return np.ascontiguousarray(px)


def read_image(path):
    ext = os.path.splitext(path)[1].lower()
    if ext == ".png":
        return read_png(path)
    if ext == ".tga":
        return read_tga(path)
    raise NotImplementedError("image format %s (oracle-side reader)" % ext)


def pack_rgb(img):
    """Texture::LoadFromFile packing (template/texture.h:24-38): greyscale replicated, else 0xRRGGBB from the first 3 channels."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    n = img.shape[2]
    a = img.astype(np.uint32)
    if n == 1:
        p = a[:, :, 0]
        return p + (p << 8) + (p << 16)
    return (a[:, :, 0] << 16) + (a[:, :, 1] << 8) + a[:, :, 2]


def read_scene_xml(path):
    """Scene file schema of LoadSceneFile (infra/scene/file_scene.cpp:64-135)."""
    root = ET.parse(path).getroot()

    def xyz(node, default=0.0):
        v = [default] * 3
        for ch in node:
            v[ord(ch.tag[0]) - ord("x")] = float(np.float32(float(ch.text)))
        return v
    sc = dict(name=root.find("scene_name").text, light=xyz(root.find("light_position")),
              plane_texture=root.find("plane_texture_location").text, skydome=root.find("skydome_location").text,
              objects=[], materials=[])
    for o in root.find("objects").findall("object"):
        sc["objects"].append(dict(model=o.find("model_location").text, material_idx=int(o.find("material_idx").text),
                                  position=xyz(o.find("position")), rotation=xyz(o.find("rotation")), scale=xyz(o.find("scale"))))
    for m in root.find("materials").findall("material"):
        t = m.find("texture_location").text
        sc["materials"].append(dict(reflectivity=float(m.find("reflectivity").text), refractivity=float(m.find("refractivity").text),
                                    absorption=xyz(m.find("absorption")), texture=(t or "").strip()))
    return sc


def load_scene(xml_path, kind, base_dir=None):
    """Build an Oracle from a scene XML.  Paths inside the XML are relative to `base_dir`
    (the reference resolves them against the executable's working directory)."""
    sc = read_scene_xml(xml_path)
    base = base_dir if base_dir is not None else os.path.dirname(os.path.abspath(xml_path))

    def rp(p):
        return p if os.path.isabs(p) else os.path.normpath(os.path.join(base, p))
    o = Oracle(kind)
    o.set_light_position(sc["light"])
    o.set_floor_texture(pack_rgb(read_image(rp(sc["plane_texture"]))))
    o.set_skydome(pack_rgb(read_image(rp(sc["skydome"]))))
    for m in sc["materials"]:
        tex = pack_rgb(read_image(rp(m["texture"]))) if m["texture"] else None
        o.add_material(m["reflectivity"], m["refractivity"], m["absorption"], tex)
    for ob in sc["objects"]:
        o.add_object(read_obj(rp(ob["model"])), ob["position"], ob["rotation"], ob["scale"], ob["material_idx"])
    o.build()
    return o, sc


KD_NODE_DTYPE = np.dtype([("aabbMin", "<f4", 3), ("left", "<i4"), ("aabbMax", "<f4", 3), ("right", "<i4"), ("splitDistance", "<f4"), ("splitAxis", "<i4"),
                          ("firstTri", "<u4"), ("triCount", "<u4")])      # flat pre-order KDTreeNode (left < 0: leaf), 48 bytes
assert KD_NODE_DTYPE.itemsize == 48


class AltAccel:
    """KDTree (infra/kdtree.cpp) or Grid (infra/grid.cpp) over a triangle array: `L`/prefix select the oracle's restatement (orc_) or the real
    reference compiled in place (ref_, oracle/_ref); same entry points, same flat layouts."""

    def __init__(self, L, prefix, kind, tris):
        self.L, self.p, self.kind = L, prefix + ("kd" if kind == "kd" else "grid"), kind
        tris = np.ascontiguousarray(tris); assert tris.dtype.itemsize == 112
        f = getattr(L, self.p + "_build"); f.restype = C.c_void_p
        self.h = C.c_void_p(f(_fp(tris), C.c_uint32(len(tris))))

    def dump(self):
        if self.kind == "kd":
            n, r, md, nu = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
            getattr(self.L, self.p + "_info")(self.h, C.byref(n), C.byref(r), C.byref(md), C.byref(nu))
            nodes = np.zeros(n.value, KD_NODE_DTYPE); refs = np.zeros(max(r.value, 1), np.uint32)
            getattr(self.L, self.p + "_dump")(self.h, _fp(nodes), _fp(refs))
            return dict(nodes=nodes, refs=refs[:r.value], maxDepth=md.value, nodesUsed=nu.value)
        res = np.zeros(3, np.int32); cell = np.zeros(3, np.float32); lo = np.zeros(3, np.float32); hi = np.zeros(3, np.float32); r = C.c_uint32()
        getattr(self.L, self.p + "_info")(self.h, _fp(res), _fp(cell), _fp(lo), _fp(hi), C.byref(r))
        start = np.zeros(int(res.prod()) + 1, np.uint32); refs = np.zeros(max(r.value, 1), np.int32)
        getattr(self.L, self.p + "_dump")(self.h, _fp(start), _fp(refs))
        return dict(resolution=res, cellSize=cell, boundsMin=lo, boundsMax=hi, cellStart=start, refs=refs[:r.value])

    def intersect(self, O, D):
        O = np.ascontiguousarray(O, np.float32).reshape(-1, 3); D = np.ascontiguousarray(D, np.float32).reshape(-1, 3)
        hits = np.zeros(O.shape[0], HIT_DTYPE)
        getattr(self.L, self.p + "_intersect")(self.h, _fp(O), _fp(D), C.c_uint32(O.shape[0]), _fp(hits))
        return hits

    def close(self):
        if self.h:
            getattr(self.L, self.p + "_free")(self.h); self.h = None


def primitive_scene(assets_dir=None, t=0.0):
    """the oracle's PrimitiveScene (infra/scene/primitive_scene.cpp): orc_create(2) + the wall images (red.png / blue.png read by the oracle-side PNG reader) + SetTime(t)"""
    o = Oracle(2)
    red = blue = None
    if assets_dir:
        red = np.ascontiguousarray(pack_rgb(read_image(os.path.join(assets_dir, "red.png"))), np.uint32)
        blue = np.ascontiguousarray(pack_rgb(read_image(os.path.join(assets_dir, "blue.png"))), np.uint32)
        assert red.shape == (512, 512) and blue.shape == (512, 512)
    if o.L.orc_prim_setup(o.h, None if red is None else _fp(red), None if blue is None else _fp(blue)) != 0:
        raise RuntimeError("orc_prim_setup refused")
    o._prim_keep = (red, blue)
    o.L.orc_prim_set_time(o.h, C.c_float(t))
    return o


def prim_set_time(o, t):
    if o.L.orc_prim_set_time(o.h, C.c_float(t)) != 0:
        raise RuntimeError("orc_prim_set_time refused")


def prim_state(o):
    out = np.zeros(108, np.float32)
    if o.L.orc_prim_state(o.h, _fp(out)) != 0:
        raise RuntimeError("orc_prim_state refused")
    return out


def prim_set_state(o, state):
    """the inverse of prim_state: the 108 floats, e.g. with identity cube / torus transforms"""
    st = np.ascontiguousarray(state, np.float32).reshape(108)
    if o.L.orc_prim_set_state(o.h, _fp(st)) != 0:
        raise RuntimeError("orc_prim_set_state refused")


PRIM_COVERAGE = ("v_neg", "swapped", "acos_small", "acos_neg", "acos_pos", "cos_kernel", "cos_reduced", "cbrt", "d1_tiny", "d1_neg", "pair1_po_pos", "pair1_po_neg",
                 "pair2_po_pos", "pair2_po_neg", "torus_nearest_po_pos", "torus_nearest_po_neg", "cube_entered", "cube_left", "cube_nan", "t_nan")


def prim_coverage(o, reset=False):
    """exact branch counts of PrimScene::find_nearest / Torus::Intersect since the last reset (process-wide): {name: count}"""
    out = np.zeros(len(PRIM_COVERAGE), np.uint64)
    if o.L.orc_prim_coverage(o.h, _fp(out), C.c_int(1 if reset else 0)) != 0:
        raise RuntimeError("orc_prim_coverage refused")
    return {k: int(v) for k, v in zip(PRIM_COVERAGE, out)}


# ops of the device probe (crt_debug_device_probe; layouts in cpu-ray-tracer_amd/csrc/device/probe.hip): name -> (number, input words, output words)
PROBE_OPS = {"EXPF": (0, 1, 1), "ACOSF": (1, 1, 1), "ATAN2F": (2, 2, 1), "SQRTF": (3, 1, 1), "DIVF": (4, 2, 1), "VEC3": (5, 6, 7), "RNG": (6, 1, 18), "TEX": (7, 4, 1),
             "SKY": (8, 5, 3), "BOX": (9, 13, 2), "TRI": (10, 16, 4), "ACOS64": (11, 2, 2), "COS64": (12, 2, 2), "CBRT64": (13, 2, 2), "SQRT64": (14, 2, 2),
             "DIV64": (15, 4, 2), "F64TOF32": (16, 2, 1)}


def probe_expected(op, inputs):
    """orc_probe_expected: `inputs` = [n, input words] of a 4-byte type (or [n, words / 2] float64); returns [n, output words] uint32 (view it as the op's type).
    TRI takes v0, v1, v2 where the device record holds v0, e1, e2."""
    num, wi, wo = PROBE_OPS[op]
    a = np.ascontiguousarray(inputs)
    n = a.shape[0] if a.ndim > 1 else (len(a) if wi * 4 == a.itemsize else len(a) * a.itemsize // (4 * wi))
    assert a.nbytes == n * wi * 4, (op, a.shape, a.dtype)
    out = np.zeros((n, wo), np.uint32)
    L = lib()
    L.orc_probe_expected.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    if L.orc_probe_expected(num, _fp(a), _fp(out), n) != 0:
        raise RuntimeError("orc_probe_expected refused")
    return out


def det_acos_cos():
    L = lib()
    L.orc_det_acos.restype = C.c_double; L.orc_det_acos.argtypes = [C.c_double]
    L.orc_det_cos.restype = C.c_double; L.orc_det_cos.argtypes = [C.c_double]
    return L.orc_det_acos, L.orc_det_cos


def set_render_accel(scene, accel):
    """scene: an oracle scene (load_scene); accel: None (BVH again) or an AltAccel of the oracle built over scene.bvh(0)["tris"] — Sample / Trace then go through it"""
    L = lib()
    r = L.orc_set_render_accel(scene.h, C.c_int(0 if accel is None else (1 if accel.kind == "kd" else 2)), None if accel is None else accel.h)
    if r != 0:
        raise RuntimeError("orc_set_render_accel refused")


def set_blas_accel(scene, accels):
    """scene: an oracle TLAS scene (load_scene(.., 1)); accels: None (the TLAS-BVH again) or one AltAccel of the oracle per BLAS, built over scene.bvh(i)["tris"] —
    FindNearest / IsOccluded / Sample / Tick / Whitted then walk TLASKDTree / TLASGrid.  The scene keeps the list alive."""
    L = lib()
    if accels is None:
        r = L.orc_set_blas_accel(scene.h, C.c_int(0), None, C.c_int(0))
    else:
        accels = list(accels)
        kinds = {a.kind for a in accels}
        if len(kinds) != 1 or any(not a.p.startswith("orc_") for a in accels):
            raise ValueError("set_blas_accel: oracle structures of one kind")
        arr = (C.c_void_p * len(accels))(*[a.h for a in accels])
        r = L.orc_set_blas_accel(scene.h, C.c_int(1 if kinds.pop() == "kd" else 2), arr, C.c_int(len(accels)))
    if r != 0:
        raise RuntimeError("orc_set_blas_accel refused: " + L.orc_last_error(scene.h).decode())
    scene._blas_accels = accels


def blas_accels(scene, kind):
    """one oracle KDTree ("kd") / Grid ("grid") per BLAS of `scene`, over its object-space triangles in reference order"""
    return [alt_accel(kind, scene.bvh(i)["tris"]) for i in range(scene.bvh_count())]


def alt_accel(kind, tris):
    """the oracle's KDTree ("kd") / Grid ("grid") over `tris`"""
    return AltAccel(lib(), "orc_", kind, tris)


def _math_probe(fn, inputs):
    inputs = np.ascontiguousarray(inputs, np.float32).reshape(-1, 12)
    out = np.zeros((len(inputs), 120), np.float32)
    fn(_fp(inputs), C.c_uint32(len(inputs)), _fp(out))
    return out


def math_probe(inputs):
    """the oracle's restatement of the same functions, same layout as Ref.math_probe"""
    return _math_probe(lib().orc_math_probe, inputs)


def vertex_dedup(v8):
    v8 = np.ascontiguousarray(v8, np.float32).reshape(-1, 8)
    idx = np.zeros(len(v8), np.uint32); uniq = np.zeros((len(v8), 8), np.float32)
    L = lib(); L.orc_vertex_dedup.restype = C.c_uint32
    n = L.orc_vertex_dedup(_fp(v8), C.c_uint32(len(v8)), _fp(idx), _fp(uniq))
    return idx, uniq[:n].copy()


def _ray_arrays(O, D, tmax):
    O = np.ascontiguousarray(O, np.float32).reshape(-1, 3); D = np.ascontiguousarray(D, np.float32).reshape(-1, 3)
    return O, D, np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (O.shape[0],))), O.shape[0]


def quad_probe(T, invT, size, O, D, tmax):
    """the oracle's QuadPrim alone (orc_quad_probe): dict(t, objIdx, occluded, normal), as Ref.quad_probe"""
    T = np.ascontiguousarray(T, np.float32).reshape(16); invT = np.ascontiguousarray(invT, np.float32).reshape(16); O, D, tmax, n = _ray_arrays(O, D, tmax)
    t, obj, occ, nrm = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(3, np.float32)
    lib().orc_quad_probe(_fp(T), _fp(invT), C.c_float(size), _fp(O), _fp(D), _fp(tmax), C.c_size_t(n), _fp(t), _fp(obj), _fp(occ), _fp(nrm))
    return dict(t=t, objIdx=obj, occluded=occ, normal=nrm)


def plane_probe(invto, O, D):
    """the oracle's PlanePrim alone (orc_plane_probe): dict(t, objIdx, uv), as Ref.plane_probe"""
    O, D, _, n = _ray_arrays(O, D, 0.0)
    t, obj, uv = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32)
    lib().orc_plane_probe(C.c_float(invto), _fp(O), _fp(D), C.c_size_t(n), _fp(t), _fp(obj), _fp(uv))
    return dict(t=t, objIdx=obj, uv=uv)


class Ref:
    """oracle/_ref: the reference's own bvh.cpp / tinyobj / stb_image compiled in place (authoring container only)."""

    def __init__(self):
        if not os.path.exists(REF_LIB_PATH):
            raise FileNotFoundError(REF_LIB_PATH)
        L = C.CDLL(REF_LIB_PATH)
        L.ref_bvh_build.restype = C.c_void_p
        L.ref_obj_load.restype = C.c_void_p
        L.ref_image_load.restype = C.POINTER(C.c_ubyte)
        L.ref_texture_load.restype = C.POINTER(C.c_uint32)
        self.L = L

    def has(self, symbol):
        """whether this build of oracle/_ref exports `symbol` (one kept from an earlier harness, where the reference tree is gone, does not have the later ones)"""
        return hasattr(self.L, symbol)

    def bvh_build(self, tris):
        tris = np.ascontiguousarray(tris)
        assert tris.dtype == TRI_DTYPE
        h = C.c_void_p(self.L.ref_bvh_build(_fp(tris), C.c_uint32(len(tris))))
        nu, md = C.c_uint32(), C.c_uint32()
        self.L.ref_bvh_info(h, C.byref(nu), C.byref(md))
        nodes = np.zeros(nu.value, NODE_DTYPE)
        idx = np.zeros(len(tris), np.uint32)
        self.L.ref_bvh_copy(h, _fp(nodes), _fp(idx))
        return h, dict(nodes=nodes, triIndices=idx, nodesUsed=nu.value, maxDepth=md.value)

    def bvh_move_and_refit(self, h, positions):
        """the reference's BVH::Refit after replacing the vertex positions ((n, 3, 3) floats); returns the node array"""
        positions = np.ascontiguousarray(positions, np.float32)
        self.L.ref_bvh_move_and_refit(h, _fp(positions), C.c_uint32(positions.shape[0]))
        nu, md = C.c_uint32(), C.c_uint32()
        self.L.ref_bvh_info(h, C.byref(nu), C.byref(md))
        nodes = np.zeros(nu.value, NODE_DTYPE)
        idx = np.zeros(positions.shape[0], np.uint32)
        self.L.ref_bvh_copy(h, _fp(nodes), _fp(idx))
        return nodes

    def bvh_intersect(self, h, O, D):
        O = np.ascontiguousarray(O, np.float32).reshape(-1, 3)
        D = np.ascontiguousarray(D, np.float32).reshape(-1, 3)
        hits = np.zeros(O.shape[0], HIT_DTYPE)
        self.L.ref_bvh_intersect(h, _fp(O), _fp(D), C.c_uint32(O.shape[0]), _fp(hits))
        return hits

    def bvh_free(self, h):
        self.L.ref_bvh_free(h)

    def alt_accel(self, kind, tris):
        """the reference's own KDTree ("kd", infra/kdtree.cpp) / Grid ("grid", infra/grid.cpp), compiled in place"""
        return AltAccel(self.L, "ref_", kind, tris)

    def math_probe(self, inputs):
        """the reference's inline tmplmath.h functions (normalize, reflect, cross, dot, mat4 factories, FastInvertedTransformNoScale, aabb): (n, 12) -> (n, 120)"""
        return _math_probe(self.L.ref_math_probe, inputs)

    def vertex_dedup(self, v8):
        """real Vertex::operator== / std::hash<Vertex> in a real std::unordered_map (infra/helper.h:28-86, model.cpp:44-50): (idx, unique vertices, hashes)"""
        v8 = np.ascontiguousarray(v8, np.float32).reshape(-1, 8)
        idx = np.zeros(len(v8), np.uint32); uniq = np.zeros((len(v8), 8), np.float32); hsh = np.zeros(len(v8), np.uint64)
        self.L.ref_vertex_dedup.restype = C.c_uint32
        n = self.L.ref_vertex_dedup(_fp(v8), C.c_uint32(len(v8)), _fp(idx), _fp(uniq), _fp(hsh))
        return idx, uniq[:n].copy(), hsh

    def obj_load(self, path):
        n = C.c_uint32()
        h = self.L.ref_obj_load(path.encode(), C.byref(n))
        if not h:
            raise RuntimeError("tinyobj failed on " + path)
        h = C.c_void_p(h)
        pos = np.zeros((n.value, 3), np.float32)
        nrm = np.zeros((n.value, 3), np.float32)
        uv = np.zeros((n.value, 2), np.float32)
        self.L.ref_obj_copy(h, _fp(pos), _fp(nrm), _fp(uv))
        self.L.ref_obj_free(h)
        return pos, nrm, uv

    def camera_rays(self, xy, pos_target=None):
        """the reference's Camera (1024 x 640): default frustum or SetCameraState(pos, target); returns (corners[4,3], O, D)"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        pt = None if pos_target is None else np.ascontiguousarray(np.concatenate([np.asarray(pos_target[0], np.float32), np.asarray(pos_target[1], np.float32)]), np.float32)
        corners = np.zeros((4, 3), np.float32); O = np.zeros((xy.shape[0], 3), np.float32); D = np.zeros((xy.shape[0], 3), np.float32)
        self.L.ref_camera_rays(None if pt is None else _fp(pt), _fp(xy), C.c_uint32(xy.shape[0]), _fp(corners), _fp(O), _fp(D))
        return corners, O, D

    def texture_load(self, path):
        """Texture::LoadFromFile's own packing: (h, w) uint32 0x00RRGGBB"""
        w, h = C.c_int(), C.c_int()
        p = self.L.ref_texture_load(path.encode(), C.byref(w), C.byref(h))
        if not p:
            raise RuntimeError("Texture::LoadFromFile failed on " + path)
        a = np.ctypeslib.as_array(p, shape=(h.value, w.value)).copy()
        self.L.ref_free(p)
        return a

    def texture_sample(self, texels, uv):
        """Texture::Sample and Material::GetAlbedo of the reference on (h, w) uint32 texels; returns (rgb, albedo)"""
        texels = np.ascontiguousarray(texels, np.uint32); uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        rgb = np.zeros((uv.shape[0], 3), np.float32); alb = np.zeros((uv.shape[0], 3), np.float32)
        self.L.ref_texture_sample(_fp(texels), texels.shape[1], texels.shape[0], _fp(uv), C.c_uint32(uv.shape[0]), _fp(rgb), _fp(alb))
        return rgb, alb

    def quad_probe(self, T, size, O, D, tmax):
        """the reference's own Quad(0, 2 * size, T): dict(t, objIdx of Intersect on Ray(O, D); occluded = IsOccluded(Ray(O, D, tmax)); invT, size as its constructor
        left them; normal = GetNormal; pos = FileScene::GetLightPos's expression on its T)"""
        T = np.ascontiguousarray(T, np.float32).reshape(16); O, D, tmax, n = _ray_arrays(O, D, tmax)
        t, obj, occ, out = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(23, np.float32)
        self.L.ref_quad_probe(_fp(T), C.c_float(size), _fp(O), _fp(D), _fp(tmax), C.c_uint32(n), _fp(t), _fp(obj), _fp(occ), _fp(out))
        return dict(t=t, objIdx=obj, occluded=occ, invT=out[:16].reshape(4, 4).copy(), size=out[16], normal=out[17:20].copy(), pos=out[20:23].copy())

    def plane_probe(self, texture_offset, O, D):
        """the reference's own Plane(1, (0, 1, 0), 1, texture_offset): dict(t, objIdx of Intersect; uv = GetUV(O + t D) where it is hit; invto)"""
        O, D, _, n = _ray_arrays(O, D, 0.0)
        t, obj, uv, invto = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32), C.c_float()
        self.L.ref_plane_probe(C.c_float(texture_offset), _fp(O), _fp(D), C.c_uint32(n), _fp(t), _fp(obj), _fp(uv), C.byref(invto))
        return dict(t=t, objIdx=obj, uv=uv, invto=np.float32(invto.value))

    def image_load(self, path):
        w, h, n = C.c_int(), C.c_int(), C.c_int()
        p = self.L.ref_image_load(path.encode(), C.byref(w), C.byref(h), C.byref(n))
        if not p:
            raise RuntimeError("stbi_load failed on " + path)
        a = np.ctypeslib.as_array(p, shape=(h.value, w.value, n.value)).copy()
        self.L.ref_image_free(p)
        return a
