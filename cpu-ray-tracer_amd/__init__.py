"""
cpu_ray_tracer_amd — ctypes binding of libcrt_amd.so (the MI355X path-tracing back end).

This module is plumbing only: every call goes straight to the C ABI declared in include/crt_abi.h and
include/crt_host.h.  There is no Python or CPU implementation of the path behind it — if the shared library is
missing, or no HIP device is visible, the calls raise.

The directory is named `cpu-ray-tracer_amd` (not an importable identifier); load it with
    importlib.util.spec_from_file_location("cpu_ray_tracer_amd", ".../cpu-ray-tracer_amd/__init__.py")
as __graft_entry__.py, bench.py and tests/conftest.py do.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIB_PATH = os.environ.get("CRT_LIB_PATH") or os.path.join(HERE, "libcrt_amd.so")   # CRT_LIB_PATH: A/B builds of the same library (tools/ab_bench.py)

SCENE_FILE, SCENE_TLAS = 0, 1
UPDATE_TRANSFORMS, UPDATE_BOUNDS = 1, 2        # crt_update_scene flags
ACCEL_KDTREE, ACCEL_GRID = 1, 2                 # FileScene's alternative accelerators (crt_upload_alt_accel / crt_find_nearest_alt)
KD_NODE_DTYPE = np.dtype([("aabbMin", "<f4", 3), ("left", "<i4"), ("aabbMax", "<f4", 3), ("right", "<i4"), ("splitDistance", "<f4"), ("splitAxis", "<i4"),
                          ("firstTri", "<u4"), ("triCount", "<u4")])      # crt_kd_node


class CrtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("crt error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("depthLimit", C.c_int32), ("device", C.c_int32),
                ("tileFirst", C.c_int32), ("tileStride", C.c_int32), ("tileCount", C.c_int32),
                ("maxFramesPerLaunch", C.c_int32), ("collectStats", C.c_int32), ("renderStreams", C.c_int32)]


# ---- reference record layouts of include/crt_abi.h (ctypes mirrors; used by Context.upload_desc = INTEGRATION.md path A from Python) ----
class BvhS(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("nodesUsed", C.c_uint32), ("triangles", C.c_void_p), ("triCount", C.c_uint32), ("triangleIndices", C.c_void_p),
                ("objIdx", C.c_int32), ("matIdx", C.c_int32), ("T", C.c_float * 16), ("invT", C.c_float * 16)]


class TextureS(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


class MaterialS(C.Structure):
    _fields_ = [("reflectivity", C.c_float), ("refractivity", C.c_float), ("absorption", C.c_float * 3), ("texture", C.c_int32)]


class SceneDescS(C.Structure):
    _fields_ = [("kind", C.c_int32), ("bvhs", C.POINTER(BvhS)), ("bvhCount", C.c_uint32), ("tlasNodes", C.c_void_p), ("tlasNodeCount", C.c_uint32),
                ("objMatIdx", C.c_void_p), ("objCount", C.c_uint32), ("materials", C.POINTER(MaterialS)), ("materialCount", C.c_uint32),
                ("textures", C.POINTER(TextureS)), ("textureCount", C.c_uint32), ("floorTexture", C.c_int32), ("skyTexture", C.c_int32),
                ("lightT", C.c_float * 16), ("lightInvT", C.c_float * 16), ("lightSize", C.c_float),
                ("floorN", C.c_float * 3), ("floorD", C.c_float), ("floorInvto", C.c_float)]


class AltAccelS(C.Structure):
    """crt_alt_accel: one KD-tree / grid description (pointers into numpy arrays the caller keeps alive)"""
    _fields_ = [("kind", C.c_int32), ("triangles", C.c_void_p), ("triCount", C.c_uint32), ("kdNodes", C.c_void_p), ("kdNodeCount", C.c_uint32),
                ("kdTriIndices", C.c_void_p), ("kdTriIndexCount", C.c_uint32), ("gridResolution", C.c_int32 * 3), ("gridCellSize", C.c_float * 3),
                ("gridMin", C.c_float * 3), ("gridMax", C.c_float * 3), ("gridCellStart", C.c_void_p), ("gridCellTris", C.c_void_p), ("gridCellTriCount", C.c_uint32)]


def alt_desc(kind, tris, s):
    """AltAccelS for a structure `s` in the layout HostScene.build_alt / blas_alt return (kind = ACCEL_KDTREE / ACCEL_GRID, tris = its TRI_DTYPE array)"""
    a = AltAccelS(); a.kind = int(kind); a.triangles = tris.ctypes.data; a.triCount = len(tris)
    if kind == ACCEL_KDTREE:
        a.kdNodes = s["nodes"].ctypes.data; a.kdNodeCount = len(s["nodes"]); a.kdTriIndices = s["refs"].ctypes.data if len(s["refs"]) else None; a.kdTriIndexCount = len(s["refs"])
    else:
        for k in range(3):
            a.gridResolution[k] = int(s["resolution"][k]); a.gridCellSize[k] = float(s["cellSize"][k]); a.gridMin[k] = float(s["boundsMin"][k]); a.gridMax[k] = float(s["boundsMax"][k])
        a.gridCellStart = s["cellStart"].ctypes.data; a.gridCellTris = s["refs"].ctypes.data if len(s["refs"]) else None; a.gridCellTriCount = len(s["refs"])
    return a


class CountersS(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rays", "primary", "interior_iters", "leaf_iters", "tri_tests", "tlas_iters", "blas_visits", "mesh_hits")]


class WhittedMetricsS(C.Structure):
    """crt_whitted_metrics"""
    _fields_ = [("rayHitCount", C.c_uint64), ("totalTraversal", C.c_uint64), ("totalTests", C.c_uint64), ("peakTraversal", C.c_int32), ("peakTests", C.c_int32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


INSPECT_NONE, INSPECT_TRAVERSAL, INSPECT_TESTS = 0, 1, 2      # crt_whitted_tick_inspect modes


class TimingS(C.Structure):
    _fields_ = [("render_kernel_ms", C.c_float), ("resolve_kernel_ms", C.c_float), ("render_launches", C.c_uint32), ("pool_launches", C.c_uint32), ("split_launches", C.c_uint32), ("reserved", C.c_uint32)]


TRI_DTYPE = np.dtype([("vertex0", "<f4", 3), ("vertex1", "<f4", 3), ("vertex2", "<f4", 3),
                      ("normal0", "<f4", 3), ("normal1", "<f4", 3), ("normal2", "<f4", 3),
                      ("uv0", "<f4", 2), ("uv1", "<f4", 2), ("uv2", "<f4", 2), ("centroid", "<f4", 3), ("objIdx", "<i4")])
NODE_DTYPE = np.dtype([("aabbMin", "<f4", 3), ("aabbMax", "<f4", 3), ("leftFirst", "<u4"), ("triCount", "<u4")])
TLAS_DTYPE = np.dtype([("aabbMin", "<f4", 3), ("leftRight", "<u4"), ("aabbMax", "<f4", 3), ("BLAS", "<u4")])
RAY_DTYPE = np.dtype([("O", "<f4", 3), ("D", "<f4", 3), ("inside", "<i4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("objIdx", "<i4"), ("triIdx", "<i4"), ("traversed", "<i4"), ("tested", "<i4")])
SHADOW_RAY_DTYPE = np.dtype([("O", "<f4", 3), ("D", "<f4", 3), ("t", "<f4")])     # crt_shadow_ray: the argument of IsOccluded
HIT_INFO_DTYPE = np.dtype([("I", "<f4", 3), ("material", "<i4"), ("N", "<f4", 3), ("u", "<f4"), ("albedo", "<f4", 3), ("v", "<f4")])   # crt_hit_info (48 bytes)
MATERIAL_MISS, MATERIAL_INVALID = -1, -2       # crt_hit_info.material of a miss / of a record whose objIdx or triIdx the scene does not have

# every symbol include/crt_abi.h and include/crt_host.h declare (tests check the library exports all of them)
ABI_SYMBOLS = ["crt_look_words", "crt_update_look", "crt_render_looks", "crt_render_looks_device", "crt_render_shapes", "crt_render_shapes_device", "crt_render_shape_sets", "crt_render_shape_sets_device", "crt_render_poses", "crt_render_poses_device", "crt_render_views", "crt_render_views_device", "crt_trace","crt_trace_device", "crt_build_bvh_device", "crt_get_bvh", "crt_build_kdtree_device", "crt_get_kdtree", "crt_build_grid_device", "crt_get_grid", "crt_update_transforms_device", "crt_sample", "crt_sample_device", "crt_refit_device", "crt_get_hit_info", "crt_get_hit_info_device", "crt_get_sky_color", "crt_get_sky_color_device", "crt_get_light", "crt_upload_blas_accel", "crt_is_occluded", "crt_find_nearest_device", "crt_is_occluded_device", "crt_upload_primitive_scene", "crt_set_render_accel", "crt_upload_alt_accel", "crt_find_nearest_alt", "crt_update_scene", "crt_abi_version", "crt_device_count", "crt_create", "crt_destroy", "crt_last_error", "crt_upload_scene", "crt_set_camera",
               "crt_render", "crt_tick", "crt_reserve", "crt_whitted_tick", "crt_whitted_tick_inspect", "crt_sync", "crt_clear", "crt_read_accumulator", "crt_resolve_screen", "crt_find_nearest", "crt_get_counters",
               "crt_reset_counters", "crt_get_timing", "crt_get_tile_clocks", "crt_bind_accumulator", "crt_accumulator_device_ptr"]
HOST_SYMBOLS = ["crt_host_scene_look", "crt_host_scene_set_look", "crt_host_bvh_build", "crt_host_scene_bvh_move_and_rebuild", "crt_host_scene_build_bvh_device", "crt_host_scene_build_kdtree_device", "crt_host_kd_build", "crt_host_scene_build_grid_device", "crt_host_grid_build", "crt_host_scene_update_transforms_device", "crt_host_scene_bvh_refit_device", "crt_host_scene_blas_alt_info", "crt_host_scene_blas_alt_copy", "crt_host_primitive_scene_create", "crt_host_primitive_scene_free", "crt_host_primitive_scene_set_time", "crt_host_primitive_scene_desc", "crt_host_primitive_scene_upload", "crt_host_scene_build_alt", "crt_host_scene_upload_alt", "crt_host_scene_alt_info", "crt_host_scene_alt_copy", "crt_host_scene_set_transform", "crt_host_scene_update", "crt_host_math_probe", "crt_host_vertex_dedup", "crt_host_last_error", "crt_host_scene_load", "crt_host_scene_free", "crt_host_scene_upload", "crt_host_scene_kind",
                "crt_host_scene_triangle_count", "crt_host_scene_bvh_count", "crt_host_scene_bvh_info", "crt_host_scene_bvh_copy",
                "crt_host_scene_bvh_move_and_refit", "crt_host_scene_blas_transform", "crt_host_scene_tlas_copy", "crt_host_camera_state", "crt_host_renderer_create",
                "crt_host_renderer_destroy", "crt_host_renderer_init", "crt_host_renderer_set_camera", "crt_host_renderer_set_passes",
                "crt_host_renderer_clear", "crt_host_renderer_tick", "crt_host_renderer_render", "crt_host_renderer_tick_whitted", "crt_host_renderer_set_inspect", "crt_host_renderer_whitted_metrics", "crt_host_renderer_spp",
                "crt_host_renderer_energy", "crt_host_renderer_accumulator", "crt_host_renderer_screen", "crt_host_renderer_ctx",
                "crt_host_obj_load", "crt_host_image_load", "crt_host_free"]


def build(force=False):
    """Compile libcrt_amd.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    srcs = [os.path.join(HERE, "Makefile")]
    for root, _, files in os.walk(os.path.join(HERE, "csrc")):
        srcs += [os.path.join(root, f) for f in files]
    srcs += [os.path.join(REPO, "include", f) for f in ("crt_abi.h", "crt_host.h")]
    stale = force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if stale:
        subprocess.check_call(["make", "-C", HERE] + (["-B"] if force else []))
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (there is no fallback path)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        # the library's test / diagnostic environment switches (CRT_RENDER_KERNEL, CRT_LAT_*, ...) are dead unless the process opts in; the test suite and the
        # tools do (tests/conftest.py, tools/*.py set CRT_ENABLE_DEBUG_HOOKS=1 for themselves), bench.py and a host application do not
        if os.environ.get("CRT_ENABLE_DEBUG_HOOKS") == "1":
            L.crt_debug_enable_hooks(1)
        L.crt_last_error.restype = C.c_char_p
        L.crt_last_error.argtypes = [C.c_void_p]
        L.crt_host_last_error.restype = C.c_char_p
        L.crt_host_renderer_energy.restype = C.c_float
        L.crt_host_renderer_accumulator.restype = C.POINTER(C.c_float)
        L.crt_host_renderer_screen.restype = C.POINTER(C.c_uint32)
        L.crt_host_renderer_ctx.restype = C.c_void_p
        L.crt_destroy.argtypes = [C.c_void_p]
        L.crt_host_scene_free.argtypes = [C.c_void_p]
        L.crt_host_renderer_destroy.argtypes = [C.c_void_p]
        L.crt_host_free.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def camera_records(width, height, pairs):
    """[K, 12] float32 camera records (camPos, topLeft, topRight, bottomLeft: crt_set_camera's arguments, crt_render_views' `cams`) of the reference Camera of a
    width x height image for each (position, target) pair — crt_host_camera_state, what Context.set_camera_state hands to crt_set_camera."""
    out = np.zeros((len(pairs), 12), np.float32)
    for k, (position, target) in enumerate(pairs):
        a = [(C.c_float * 3)() for _ in range(4)]
        rc = lib().crt_host_camera_state(int(width), int(height), _f3(position), _f3(target), *a)
        if rc != 0:
            raise CrtError(rc, lib().crt_host_last_error().decode())
        out[k] = [x for v in a for x in v]
    return out


LOOK_HEADER_WORDS, LOOK_MATERIAL_WORDS = 36, 6      # crt_abi.h: crt_look_header, crt_material


def look_words(material_count):
    """crt_look_words: the 4-byte words of one look record of a scene with `material_count` materials"""
    return LOOK_HEADER_WORDS + LOOK_MATERIAL_WORDS * int(material_count)


def look_records(looks):
    """[L, crt_look_words(materialCount)] uint32 look records (crt_update_look's argument, crt_render_looks' `looks`) from dicts with light_T / light_invT (mat4s, 16
    floats each, invT supplied by the caller as at upload), light_size, floor_texture, sky_texture (indices into the uploaded textures) and materials =
    (reflectivity, refractivity, absorption[3], texture index or -1) per material of the uploaded scene.  View the result as float32 to read the float words."""
    looks = list(looks)
    m = len(looks[0]["materials"]) if looks else 0
    out = np.zeros((len(looks), look_words(m)), np.uint32)
    f, i = out.view(np.float32), out.view(np.int32)
    for k, lk in enumerate(looks):
        if len(lk["materials"]) != m:
            raise ValueError("look_records: every look of an array has the scene's material count")
        f[k, 0:16] = np.asarray(lk["light_T"], np.float32).reshape(16)
        f[k, 16:32] = np.asarray(lk["light_invT"], np.float32).reshape(16)
        f[k, 32] = lk["light_size"]
        i[k, 33], i[k, 34] = int(lk["floor_texture"]), int(lk["sky_texture"])
        for j, (refl, refr, ab, tex) in enumerate(lk["materials"]):
            o = LOOK_HEADER_WORDS + LOOK_MATERIAL_WORDS * j
            f[k, o], f[k, o + 1] = refl, refr
            f[k, o + 2:o + 5] = np.asarray(ab, np.float32).reshape(3)
            i[k, o + 5] = int(tex)
    return out


def look_dicts(records):
    """look_records' inverse: one dict per record (fresh lists and arrays, so a caller can change one field and pack again)"""
    rec = np.ascontiguousarray(records, np.uint32)
    rec = rec.reshape(1, -1) if rec.ndim == 1 else rec
    f, i = rec.view(np.float32), rec.view(np.int32)
    m = (rec.shape[1] - LOOK_HEADER_WORDS) // LOOK_MATERIAL_WORDS
    return [dict(light_T=f[k, 0:16].copy(), light_invT=f[k, 16:32].copy(), light_size=float(f[k, 32]), floor_texture=int(i[k, 33]), sky_texture=int(i[k, 34]),
                 materials=[(float(f[k, o]), float(f[k, o + 1]), tuple(float(x) for x in f[k, o + 2:o + 5]), int(i[k, o + 5]))
                            for o in (LOOK_HEADER_WORDS + LOOK_MATERIAL_WORDS * j for j in range(m))]) for k in range(rec.shape[0])]


def device_count():
    return int(lib().crt_device_count())


class Context:
    """crt_ctx: one device, one image (or a strided subset of its 16x16 tiles)."""

    def __init__(self, width, height, depth_limit=5, device=0, tile_first=0, tile_stride=1, tile_count=-1,
                 max_frames_per_launch=0, collect_stats=False, render_streams=0):
        self.L = lib()
        cfg = Config(width, height, depth_limit, device, tile_first, tile_stride, tile_count, max_frames_per_launch, int(collect_stats), render_streams)
        h = C.c_void_p()
        rc = self.L.crt_create(C.byref(h), C.byref(cfg))
        if rc != 0:
            raise CrtError(rc, self.L.crt_last_error(None).decode())
        self.h = h
        self.W, self.H = width, height
        self.device = device
        self._owned = True
        self.tiles = (width // 16) * (height // 16) if tile_count < 0 else tile_count      # owned tiles

    @classmethod
    def borrow(cls, handle, width, height, device=0):
        o = cls.__new__(cls)
        o.L = lib()
        o.h = C.c_void_p(handle)
        o.W, o.H = width, height
        o.device = device
        o._owned = False
        return o

    def close(self):
        if getattr(self, "h", None) and self._owned:
            self.L.crt_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise CrtError(rc, self.L.crt_last_error(self.h).decode())

    def set_camera(self, cam_pos, top_left, top_right, bottom_left):
        self._ck(self.L.crt_set_camera(self.h, _f3(cam_pos), _f3(top_left), _f3(top_right), _f3(bottom_left)))

    def set_camera_state(self, position, target):
        a = [(C.c_float * 3)() for _ in range(4)]
        rc = self.L.crt_host_camera_state(self.W, self.H, _f3(position), _f3(target), *a)
        if rc != 0:
            raise CrtError(rc, self.L.crt_host_last_error().decode())
        self._ck(self.L.crt_set_camera(self.h, *a))

    def render(self, spp_first, frames, passes=1):
        self._ck(self.L.crt_render(self.h, C.c_uint32(spp_first), C.c_uint32(frames), C.c_uint32(passes)))

    def render_views(self, cameras, spp_first, frames, passes=1, scale=None):
        """crt_render_views: the frames of K cameras in one job (host buffers, synchronous).  cameras = [K, 12] float32 records (camera_records).  Returns the
        accumulators [K, H, W, 4] float32 — what set_camera + clear + render(spp_first, frames, passes) + accumulator() leaves per view, on the tiles this context
        owns; every other pixel is 0 — and, when `scale` is given, (accumulators, pixels [K, H, W] uint32): resolve_screen(scale)'s pixels of them."""
        cams = np.ascontiguousarray(cameras, np.float32).reshape(-1, 12)
        k = cams.shape[0]
        acc = np.zeros((k, self.H, self.W, 4), np.float32)
        px = np.zeros((k, self.H, self.W), np.uint32) if scale is not None else None
        self._ck(self.L.crt_render_views(self.h, _p(cams), C.c_uint32(k), C.c_uint32(spp_first), C.c_uint32(frames), C.c_uint32(passes),
                                         C.c_float(1.0 if scale is None else scale), _p(acc), _p(px) if px is not None else None))
        return acc if scale is None else (acc, px)

    def render_views_device(self, cams, out, spp_first, frames, passes=1, scale=None, pixels=None, stream=None):
        """crt_render_views_device: the same job for torch tensors on the context's device, enqueued on `stream` (default torch.cuda.current_stream()) without a host
        wait.  cams = [K, 12] float32, out = [K, H, W, 4] float32, pixels = None or [K, H, W] int32 (the uint32 bit patterns; needs `scale`), all contiguous; only
        the pixels of owned tiles are written.  Returns out, or (out, pixels) when pixels is given."""
        import torch
        dev = torch.device("cuda", self.device)
        k = cams.shape[0] if isinstance(cams, torch.Tensor) and cams.dim() == 2 else -1
        for t, dt, shape, name in ((cams, torch.float32, (k, 12), "cams"), (out, torch.float32, (k, self.H, self.W, 4), "out"), (pixels, torch.int32, (k, self.H, self.W), "pixels")):
            if t is None and name == "pixels":
                continue
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("render_views_device: %s must be a contiguous %s tensor of shape %s on cuda:%d" % (name, dt, shape, self.device))
        if pixels is not None and scale is None:
            raise ValueError("render_views_device: pixels need a scale")

        def run(st):
            self._ck(self.L.crt_render_views_device(self.h, C.c_void_p(cams.data_ptr()), C.c_uint32(k), C.c_uint32(spp_first), C.c_uint32(frames), C.c_uint32(passes),
                                                    C.c_float(1.0 if scale is None else scale), C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(pixels.data_ptr()) if pixels is not None else None, C.c_void_p(st.cuda_stream)))
            return out if pixels is None else (out, pixels)
        return self._enqueue(stream, run)

    def update_look(self, look):
        """crt_update_look: the live scene's look — light quad, floor / skydome texture, materials — changed in place (no re-upload).  look = one record of
        look_records, [crt_look_words(materialCount)] uint32."""
        rec = np.ascontiguousarray(look, np.uint32).reshape(-1)
        self._ck(self.L.crt_update_look(self.h, _p(rec)))

    def render_looks(self, cameras, looks, spp_first, frames, passes=1, scale=None, view_look=None):
        """crt_render_looks: the frames of K cameras over L looks of the live scene in one job (host buffers, synchronous; the live scene is not changed).
        cameras = [K, 12] float32 (camera_records), looks = [L, crt_look_words(materialCount)] uint32 (look_records), view_look = None (view k renders look k; L == K)
        or K indices into the looks.  Returns the accumulators [K, H, W, 4] float32 — per view what update_look(looks[l]) + set_camera + clear + render(spp_first,
        frames, passes) + accumulator() leaves on the tiles this context owns, every other pixel 0 — and, when `scale` is given, (accumulators, pixels [K, H, W] uint32)."""
        cams = np.ascontiguousarray(cameras, np.float32).reshape(-1, 12)
        rec = np.ascontiguousarray(looks, np.uint32)
        if rec.ndim != 2:
            raise ValueError("render_looks: looks must be [L, crt_look_words(materialCount)] uint32")
        k, n = cams.shape[0], rec.shape[0]
        vl = None if view_look is None else np.ascontiguousarray(view_look, np.int32).reshape(-1)
        if vl is not None and vl.shape[0] != k:
            raise ValueError("render_looks: view_look needs one index per camera")
        acc = np.zeros((k, self.H, self.W, 4), np.float32)
        px = np.zeros((k, self.H, self.W), np.uint32) if scale is not None else None
        self._ck(self.L.crt_render_looks(self.h, _p(cams), C.c_uint32(k), _p(rec), C.c_uint32(n), _p(vl) if vl is not None else None, C.c_uint32(spp_first),
                                         C.c_uint32(frames), C.c_uint32(passes), C.c_float(1.0 if scale is None else scale), _p(acc), _p(px) if px is not None else None))
        return acc if scale is None else (acc, px)

    def render_looks_device(self, cams, looks, out, spp_first, frames, passes=1, scale=None, pixels=None, view_look=None, stream=None):
        """crt_render_looks_device: the same job for torch tensors on the context's device, enqueued on `stream` (default torch.cuda.current_stream()); one host
        wait, for the build's status header.  cams = [K, 12] float32, looks = [L, crt_look_words(materialCount)] int32 (the records' bit patterns), out = [K, H, W, 4]
        float32, pixels = None or [K, H, W] int32 (needs `scale`), view_look = None or [K] int32, all contiguous; only the pixels of owned tiles are written.
        Returns out, or (out, pixels) when pixels is given."""
        import torch
        dev = torch.device("cuda", self.device)
        k = cams.shape[0] if isinstance(cams, torch.Tensor) and cams.dim() == 2 else -1
        n, w = (looks.shape[0], looks.shape[1]) if isinstance(looks, torch.Tensor) and looks.dim() == 2 else (-1, -1)
        for t, dt, shape, name in ((cams, torch.float32, (k, 12), "cams"), (looks, torch.int32, (n, w), "looks"), (out, torch.float32, (k, self.H, self.W, 4), "out"),
                                   (pixels, torch.int32, (k, self.H, self.W), "pixels"), (view_look, torch.int32, (k,), "view_look")):
            if t is None and name in ("pixels", "view_look"):
                continue
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("render_looks_device: %s must be a contiguous %s tensor of shape %s on cuda:%d" % (name, dt, shape, self.device))
        if pixels is not None and scale is None:
            raise ValueError("render_looks_device: pixels need a scale")

        def run(st):
            self._ck(self.L.crt_render_looks_device(self.h, C.c_void_p(cams.data_ptr()), C.c_uint32(k), C.c_void_p(looks.data_ptr()), C.c_uint32(n),
                                                    C.c_void_p(view_look.data_ptr()) if view_look is not None else None, C.c_uint32(spp_first), C.c_uint32(frames),
                                                    C.c_uint32(passes), C.c_float(1.0 if scale is None else scale), C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(pixels.data_ptr()) if pixels is not None else None, C.c_void_p(st.cuda_stream)))
            return out if pixels is None else (out, pixels)
        return self._enqueue(stream, run)

    def render_poses(self, cameras, T, spp_first, frames, passes=1, scale=None, view_pose=None, want_tlas=False):
        """crt_render_poses: the frames of K cameras over P poses of a two-level scene's instances in one job (host buffers, synchronous; the live scene is not
        changed).  cameras = [K, 12] float32 (camera_records), T = [P, blasCount, 16] float32 row-major mat4s (update_transforms_device's, per pose), view_pose = None
        (view k renders pose k; P == K) or K indices into the poses.  Returns the accumulators [K, H, W, 4] float32 — per view what update_transforms_device(T[p]) +
        set_camera + clear + render(spp_first, frames, passes) + accumulator() leaves on the tiles this context owns, every other pixel 0 —, then the pixels
        [K, H, W] uint32 when `scale` is given, then the TLAS nodes [P, 2 * blasCount] (TLAS_DTYPE) when want_tlas: a tuple when more than one."""
        cams = np.ascontiguousarray(cameras, np.float32).reshape(-1, 12)
        t = np.ascontiguousarray(T, np.float32)
        if t.ndim != 3 or t.shape[2] != 16:
            raise ValueError("render_poses: T must be [P, blasCount, 16] float32")
        k, p, n = cams.shape[0], t.shape[0], t.shape[1]
        vp = None if view_pose is None else np.ascontiguousarray(view_pose, np.int32).reshape(-1)
        if vp is not None and vp.shape[0] != k:
            raise ValueError("render_poses: view_pose needs one index per camera")
        acc = np.zeros((k, self.H, self.W, 4), np.float32)
        px = np.zeros((k, self.H, self.W), np.uint32) if scale is not None else None
        nodes = np.zeros((p, 2 * n), TLAS_DTYPE) if want_tlas else None
        self._ck(self.L.crt_render_poses(self.h, _p(cams), C.c_uint32(k), _p(t), C.c_uint32(p), C.c_uint32(n), _p(vp) if vp is not None else None, C.c_uint32(spp_first),
                                         C.c_uint32(frames), C.c_uint32(passes), C.c_float(1.0 if scale is None else scale), _p(acc), _p(px) if px is not None else None,
                                         _p(nodes) if nodes is not None else None))
        out = [acc] + ([px] if px is not None else []) + ([nodes] if nodes is not None else [])
        return out[0] if len(out) == 1 else tuple(out)

    def render_poses_device(self, cams, T, out, spp_first, frames, passes=1, scale=None, pixels=None, view_pose=None, want_tlas=False, stream=None):
        """crt_render_poses_device: the same job for torch tensors on the context's device, enqueued on `stream` (default torch.cuda.current_stream()); one host
        wait, for the build headers.  cams = [K, 12] float32, T = [P, blasCount, 16] float32, out = [K, H, W, 4] float32, pixels = None or [K, H, W] int32 (needs
        `scale`), view_pose = None or [K] int32, all contiguous; only the pixels of owned tiles are written.  Returns out, then pixels when given, then the TLAS
        nodes [P, 2 * blasCount] (numpy, TLAS_DTYPE) when want_tlas: a tuple when more than one."""
        import torch
        dev = torch.device("cuda", self.device)
        k = cams.shape[0] if isinstance(cams, torch.Tensor) and cams.dim() == 2 else -1
        p, n = (T.shape[0], T.shape[1]) if isinstance(T, torch.Tensor) and T.dim() == 3 else (-1, -1)
        for t, dt, shape, name in ((cams, torch.float32, (k, 12), "cams"), (T, torch.float32, (p, n, 16), "T"), (out, torch.float32, (k, self.H, self.W, 4), "out"),
                                   (pixels, torch.int32, (k, self.H, self.W), "pixels"), (view_pose, torch.int32, (k,), "view_pose")):
            if t is None and name in ("pixels", "view_pose"):
                continue
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("render_poses_device: %s must be a contiguous %s tensor of shape %s on cuda:%d" % (name, dt, shape, self.device))
        if pixels is not None and scale is None:
            raise ValueError("render_poses_device: pixels need a scale")
        nodes = np.zeros((p, 2 * n), TLAS_DTYPE) if want_tlas else None

        def run(st):
            self._ck(self.L.crt_render_poses_device(self.h, C.c_void_p(cams.data_ptr()), C.c_uint32(k), C.c_void_p(T.data_ptr()), C.c_uint32(p), C.c_uint32(n),
                                                    C.c_void_p(view_pose.data_ptr()) if view_pose is not None else None, C.c_uint32(spp_first), C.c_uint32(frames),
                                                    C.c_uint32(passes), C.c_float(1.0 if scale is None else scale), C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(pixels.data_ptr()) if pixels is not None else None, _p(nodes) if nodes is not None else None,
                                                    C.c_void_p(st.cuda_stream)))
            res = [out] + ([pixels] if pixels is not None else []) + ([nodes] if nodes is not None else [])
            return res[0] if len(res) == 1 else tuple(res)
        return self._enqueue(stream, run)

    def render_shapes(self, cameras, bvh, positions, spp_first, frames, passes=1, scale=None, T=None, view_shape=None, want_root_boxes=False, want_tlas=False):
        """crt_render_shapes: the frames of K cameras over S shapes of uploaded BVH `bvh` in one job (host buffers, synchronous; the live scene is not changed).
        cameras = [K, 12] float32 (camera_records), positions = [S, triCount, 3, 3] (or [S, triCount, 9]) float32, per shape what refit_device takes, T = None (a
        FileScene) or [S, blasCount, 16] float32 row-major mat4s (update_transforms_device's, per shape), view_shape = None (view k renders shape k; S == K) or K
        indices into the shapes.  Returns the accumulators [K, H, W, 4] float32 — per view what refit_device(bvh, positions[s]) (+ update_transforms_device(T[s])) +
        set_camera + clear + render(spp_first, frames, passes) + accumulator() leaves on the tiles this context owns, every other pixel 0 —, then the pixels
        [K, H, W] uint32 when `scale` is given, then the TLAS nodes [S, 2 * blasCount] (TLAS_DTYPE) when want_tlas, then node 0's boxes [S, 2, 3] float32 (aabbMin,
        aabbMax: refit_device's) when want_root_boxes: a tuple when more than one."""
        cams = np.ascontiguousarray(cameras, np.float32).reshape(-1, 12)
        pos = np.ascontiguousarray(positions, np.float32)
        if pos.ndim < 3 or pos.shape[2:] not in ((3, 3), (9,)):
            raise ValueError("render_shapes: positions must be [S, triCount, 3, 3] or [S, triCount, 9] float32")
        k, s, tris = cams.shape[0], pos.shape[0], pos.shape[1]
        t = None if T is None else np.ascontiguousarray(T, np.float32)
        if t is not None and (t.ndim != 3 or t.shape[2] != 16 or t.shape[0] != s):
            raise ValueError("render_shapes: T must be [S, blasCount, 16] float32")
        n = 0 if t is None else t.shape[1]
        vs = None if view_shape is None else np.ascontiguousarray(view_shape, np.int32).reshape(-1)
        if vs is not None and vs.shape[0] != k:
            raise ValueError("render_shapes: view_shape needs one index per camera")
        if want_tlas and t is None:
            raise ValueError("render_shapes: a FileScene has no TLAS")
        acc = np.zeros((k, self.H, self.W, 4), np.float32)
        px = np.zeros((k, self.H, self.W), np.uint32) if scale is not None else None
        nodes = np.zeros((s, 2 * n), TLAS_DTYPE) if want_tlas else None
        boxes = np.zeros((s, 2, 3), np.float32) if want_root_boxes else None
        self._ck(self.L.crt_render_shapes(self.h, _p(cams), C.c_uint32(k), C.c_uint32(bvh), _p(pos), C.c_uint32(s), C.c_uint32(tris), _p(t) if t is not None else None, C.c_uint32(n),
                                          _p(vs) if vs is not None else None, C.c_uint32(spp_first), C.c_uint32(frames), C.c_uint32(passes), C.c_float(1.0 if scale is None else scale),
                                          _p(acc), _p(px) if px is not None else None, _p(boxes) if boxes is not None else None, _p(nodes) if nodes is not None else None))
        out = [acc] + ([px] if px is not None else []) + ([nodes] if nodes is not None else []) + ([boxes] if boxes is not None else [])
        return out[0] if len(out) == 1 else tuple(out)

    def render_shapes_device(self, cams, bvh, positions, out, spp_first, frames, passes=1, scale=None, pixels=None, T=None, view_shape=None, want_root_boxes=False, want_tlas=False,
                             stream=None):
        """crt_render_shapes_device: the same job for torch tensors on the context's device, enqueued on `stream` (default torch.cuda.current_stream()); one host
        wait, for the job header (and a two-level scene's build headers).  cams = [K, 12] float32, positions = [S, triCount, 3, 3] or [S, triCount, 9] float32, T =
        None or [S, blasCount, 16] float32, out = [K, H, W, 4] float32, pixels = None or [K, H, W] int32 (needs `scale`), view_shape = None or [K] int32, all
        contiguous; only the pixels of owned tiles are written.  Returns out, then pixels when given, then the TLAS nodes [S, 2 * blasCount] (numpy, TLAS_DTYPE) when
        want_tlas, then node 0's boxes [S, 2, 3] (numpy) when want_root_boxes: a tuple when more than one."""
        import torch
        dev = torch.device("cuda", self.device)
        k = cams.shape[0] if isinstance(cams, torch.Tensor) and cams.dim() == 2 else -1
        if not isinstance(positions, torch.Tensor) or positions.dim() < 3 or tuple(positions.shape[2:]) not in ((3, 3), (9,)):
            raise ValueError("render_shapes_device: positions must be a float32 tensor of shape [S, triCount, 3, 3] or [S, triCount, 9] on cuda:%d" % self.device)
        s, tris = positions.shape[0], positions.shape[1]
        n = T.shape[1] if isinstance(T, torch.Tensor) and T.dim() == 3 else (0 if T is None else -1)
        for t, dt, shape, name in ((cams, torch.float32, (k, 12), "cams"), (positions, torch.float32, tuple(positions.shape), "positions"), (T, torch.float32, (s, n, 16), "T"),
                                   (out, torch.float32, (k, self.H, self.W, 4), "out"), (pixels, torch.int32, (k, self.H, self.W), "pixels"), (view_shape, torch.int32, (k,), "view_shape")):
            if t is None and name in ("pixels", "view_shape", "T"):
                continue
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("render_shapes_device: %s must be a contiguous %s tensor of shape %s on cuda:%d" % (name, dt, shape, self.device))
        if pixels is not None and scale is None:
            raise ValueError("render_shapes_device: pixels need a scale")
        if want_tlas and T is None:
            raise ValueError("render_shapes_device: a FileScene has no TLAS")
        nodes = np.zeros((s, 2 * n), TLAS_DTYPE) if want_tlas else None
        boxes = np.zeros((s, 2, 3), np.float32) if want_root_boxes else None

        def run(st):
            self._ck(self.L.crt_render_shapes_device(self.h, C.c_void_p(cams.data_ptr()), C.c_uint32(k), C.c_uint32(bvh), C.c_void_p(positions.data_ptr()), C.c_uint32(s), C.c_uint32(tris),
                                                     C.c_void_p(T.data_ptr()) if T is not None else None, C.c_uint32(n),
                                                     C.c_void_p(view_shape.data_ptr()) if view_shape is not None else None, C.c_uint32(spp_first), C.c_uint32(frames),
                                                     C.c_uint32(passes), C.c_float(1.0 if scale is None else scale), C.c_void_p(out.data_ptr()),
                                                     C.c_void_p(pixels.data_ptr()) if pixels is not None else None, _p(boxes) if boxes is not None else None,
                                                     _p(nodes) if nodes is not None else None, C.c_void_p(st.cuda_stream)))
            res = [out] + ([pixels] if pixels is not None else []) + ([nodes] if nodes is not None else []) + ([boxes] if boxes is not None else [])
            return res[0] if len(res) == 1 else tuple(res)
        return self._enqueue(stream, run)

    def render_shape_sets(self, cameras, bvhs, positions, spp_first, frames, passes=1, scale=None, T=None, view_shape=None, want_root_boxes=False, want_tlas=False):
        """crt_render_shape_sets: the frames of K cameras over S shapes of a two-level scene in which the M uploaded BLASes `bvhs` deform per shape, in one job (host
        buffers, synchronous; the live scene is not changed).  cameras = [K, 12] float32 (camera_records), bvhs = M distinct BLAS indices, positions = a list of M arrays
        [S, triCount_m, 3, 3] float32 in the order of bvhs (per shape what refit_device takes for that BVH), or one array [S, setTris, 9] (or [S, setTris, 3, 3]) with
        the blocks in that order, T = [S, blasCount, 16] float32, view_shape = None (view k renders shape k; S == K) or K indices into the shapes.  Returns what
        render_shapes returns — per view what refit_device(bvhs[m], ...) for every m + update_transforms_device(T[s]) + set_camera + clear + render + accumulator()
        leaves —, with node 0's boxes [S, M, 2, 3] float32 when want_root_boxes."""
        cams = np.ascontiguousarray(cameras, np.float32).reshape(-1, 12)
        ids = np.ascontiguousarray(bvhs, np.uint32).reshape(-1)
        if isinstance(positions, (list, tuple)):
            parts = [np.ascontiguousarray(a, np.float32) for a in positions]
            if len(parts) != ids.shape[0] or any(a.ndim < 3 or a.shape[0] != parts[0].shape[0] for a in parts):
                raise ValueError("render_shape_sets: positions must hold one [S, triCount_m, 3, 3] array per BVH of the set")
            pos = np.ascontiguousarray(np.concatenate([a.reshape(a.shape[0], a.shape[1], 9) for a in parts], axis=1)) if parts else np.zeros((0, 0, 9), np.float32)
        else:
            pos = np.ascontiguousarray(positions, np.float32)
        if pos.ndim < 3 or pos.shape[2:] not in ((3, 3), (9,)):
            raise ValueError("render_shape_sets: positions must be M arrays [S, triCount_m, 3, 3] or one [S, setTris, 9] float32 array")
        k, s, tris, m = cams.shape[0], pos.shape[0], pos.shape[1], ids.shape[0]
        t = None if T is None else np.ascontiguousarray(T, np.float32)
        if t is not None and (t.ndim != 3 or t.shape[2] != 16 or t.shape[0] != s):
            raise ValueError("render_shape_sets: T must be [S, blasCount, 16] float32")
        n = 0 if t is None else t.shape[1]
        vs = None if view_shape is None else np.ascontiguousarray(view_shape, np.int32).reshape(-1)
        if vs is not None and vs.shape[0] != k:
            raise ValueError("render_shape_sets: view_shape needs one index per camera")
        acc = np.zeros((k, self.H, self.W, 4), np.float32)
        px = np.zeros((k, self.H, self.W), np.uint32) if scale is not None else None
        nodes = np.zeros((s, 2 * n), TLAS_DTYPE) if want_tlas else None
        boxes = np.zeros((s, m, 2, 3), np.float32) if want_root_boxes else None
        self._ck(self.L.crt_render_shape_sets(self.h, _p(cams), C.c_uint32(k), _p(ids), C.c_uint32(m), _p(pos), C.c_uint32(s), C.c_uint32(tris), _p(t) if t is not None else None,
                                              C.c_uint32(n), _p(vs) if vs is not None else None, C.c_uint32(spp_first), C.c_uint32(frames), C.c_uint32(passes),
                                              C.c_float(1.0 if scale is None else scale), _p(acc), _p(px) if px is not None else None, _p(boxes) if boxes is not None else None,
                                              _p(nodes) if nodes is not None else None))
        out = [acc] + ([px] if px is not None else []) + ([nodes] if nodes is not None else []) + ([boxes] if boxes is not None else [])
        return out[0] if len(out) == 1 else tuple(out)

    def render_shape_sets_device(self, cams, bvhs, positions, out, spp_first, frames, passes=1, scale=None, pixels=None, T=None, view_shape=None, want_root_boxes=False,
                                 want_tlas=False, stream=None):
        """crt_render_shape_sets_device: the same job for torch tensors on the context's device, enqueued on `stream` (default torch.cuda.current_stream()); one host
        wait, for the job header and the build headers.  cams = [K, 12] float32, bvhs = M BLAS indices (host), positions = [S, setTris, 3, 3] or [S, setTris, 9]
        float32 (per shape the BVHs' blocks in the order of bvhs), T = [S, blasCount, 16] float32, out = [K, H, W, 4] float32, pixels = None or [K, H, W] int32 (needs
        `scale`), view_shape = None or [K] int32, all contiguous; only the pixels of owned tiles are written.  Returns out, then pixels when given, then the TLAS
        nodes [S, 2 * blasCount] (numpy, TLAS_DTYPE) when want_tlas, then node 0's boxes [S, M, 2, 3] (numpy) when want_root_boxes: a tuple when more than one."""
        import torch
        dev = torch.device("cuda", self.device)
        ids = np.ascontiguousarray(bvhs, np.uint32).reshape(-1)
        k = cams.shape[0] if isinstance(cams, torch.Tensor) and cams.dim() == 2 else -1
        if not isinstance(positions, torch.Tensor) or positions.dim() < 3 or tuple(positions.shape[2:]) not in ((3, 3), (9,)):
            raise ValueError("render_shape_sets_device: positions must be a float32 tensor of shape [S, setTris, 3, 3] or [S, setTris, 9] on cuda:%d" % self.device)
        s, tris, m = positions.shape[0], positions.shape[1], ids.shape[0]
        n = T.shape[1] if isinstance(T, torch.Tensor) and T.dim() == 3 else -1
        for t, dt, shape, name in ((cams, torch.float32, (k, 12), "cams"), (positions, torch.float32, tuple(positions.shape), "positions"), (T, torch.float32, (s, n, 16), "T"),
                                   (out, torch.float32, (k, self.H, self.W, 4), "out"), (pixels, torch.int32, (k, self.H, self.W), "pixels"), (view_shape, torch.int32, (k,), "view_shape")):
            if t is None and name in ("pixels", "view_shape"):
                continue
            if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("render_shape_sets_device: %s must be a contiguous %s tensor of shape %s on cuda:%d" % (name, dt, shape, self.device))
        if pixels is not None and scale is None:
            raise ValueError("render_shape_sets_device: pixels need a scale")
        nodes = np.zeros((s, 2 * n), TLAS_DTYPE) if want_tlas else None
        boxes = np.zeros((s, m, 2, 3), np.float32) if want_root_boxes else None

        def run(st):
            self._ck(self.L.crt_render_shape_sets_device(self.h, C.c_void_p(cams.data_ptr()), C.c_uint32(k), _p(ids), C.c_uint32(m), C.c_void_p(positions.data_ptr()), C.c_uint32(s),
                                                         C.c_uint32(tris), C.c_void_p(T.data_ptr()), C.c_uint32(n),
                                                         C.c_void_p(view_shape.data_ptr()) if view_shape is not None else None, C.c_uint32(spp_first), C.c_uint32(frames),
                                                         C.c_uint32(passes), C.c_float(1.0 if scale is None else scale), C.c_void_p(out.data_ptr()),
                                                         C.c_void_p(pixels.data_ptr()) if pixels is not None else None, _p(boxes) if boxes is not None else None,
                                                         _p(nodes) if nodes is not None else None, C.c_void_p(st.cuda_stream)))
            res = [out] + ([pixels] if pixels is not None else []) + ([nodes] if nodes is not None else []) + ([boxes] if boxes is not None else [])
            return res[0] if len(res) == 1 else tuple(res)
        return self._enqueue(stream, run)

    def tick(self, spp, passes=1, pixels=True, accumulator=True):
        """crt_tick: one Renderer::Tick at `spp` (crt_render(spp, 1, passes) + read-back + resolve; frames after a run of still Ticks are rendered ahead).
        Returns (pixels (H, W) uint32 or None, accumulator (H, W, 4) float32 or None, energy)."""
        px = np.empty((self.H, self.W), np.uint32) if pixels else None
        acc = np.empty((self.H, self.W, 4), np.float32) if accumulator else None
        e = C.c_float()
        self._ck(self.L.crt_tick(self.h, C.c_uint32(spp), C.c_uint32(passes), _p(px) if px is not None else None, _p(acc) if acc is not None else None, C.byref(e)))
        return px, acc, e.value

    def reserve(self, frames, passes=1):
        self._ck(self.L.crt_reserve(self.h, C.c_uint32(frames), C.c_uint32(passes)))

    def whitted_tick(self):
        px = np.empty((self.H, self.W), np.uint32)
        self._ck(self.L.crt_whitted_tick(self.h, _p(px)))
        return px

    def whitted_tick_inspect(self, inspect=0, peak_traversal=0, peak_tests=0, counts=False):
        """crt_whitted_tick_inspect: one Whitted Tick in mode `inspect` (INSPECT_NONE / _TRAVERSAL / _TESTS) with the peaks carried in.  Returns (pixels, metrics dict)
        or, with counts=True, (pixels, metrics dict, traversed (H, W) int32, tested (H, W) int32) of the primary rays."""
        px = np.empty((self.H, self.W), np.uint32)
        tr = np.empty((self.H, self.W), np.int32) if counts else None
        te = np.empty((self.H, self.W), np.int32) if counts else None
        m = WhittedMetricsS()
        self._ck(self.L.crt_whitted_tick_inspect(self.h, C.c_int(inspect), C.c_int32(peak_traversal), C.c_int32(peak_tests), _p(px), _p(tr) if counts else None, _p(te) if counts else None, C.byref(m)))
        return (px, m.as_dict(), tr, te) if counts else (px, m.as_dict())

    def sync(self):
        self._ck(self.L.crt_sync(self.h))

    def clear(self):
        self._ck(self.L.crt_clear(self.h))

    def accumulator(self):
        a = np.empty((self.H, self.W, 4), np.float32)
        self._ck(self.L.crt_read_accumulator(self.h, _p(a)))
        return a

    def resolve_screen(self, scale):
        px = np.empty((self.H, self.W), np.uint32)
        e = C.c_float()
        self._ck(self.L.crt_resolve_screen(self.h, C.c_float(scale), _p(px), C.byref(e)))
        return px, e.value

    def set_render_accel(self, kind):
        """crt_set_render_accel: 0 = BVH / TLAS, ACCEL_KDTREE / ACCEL_GRID = Sample and Trace go through the uploaded alternative accelerator"""
        self._ck(self.L.crt_set_render_accel(self.h, int(kind)))

    def find_nearest_alt(self, kind, O, D):
        """scene.FindNearest with FileScene's KD-tree / grid in place of the BVH (crt_find_nearest_alt)"""
        O = np.ascontiguousarray(O, np.float32).reshape(-1, 3); D = np.ascontiguousarray(D, np.float32).reshape(-1, 3)
        rays = np.zeros(O.shape[0], RAY_DTYPE); rays["O"] = O; rays["D"] = D
        hits = np.zeros(O.shape[0], HIT_DTYPE)
        self._ck(self.L.crt_find_nearest_alt(self.h, int(kind), _p(rays), _p(hits), C.c_size_t(O.shape[0])))
        return hits

    def upload_blas_accel(self, kind, structs, tris):
        """crt_upload_blas_accel: a two-level scene's BLASKDTree / BLASGrid set; structs[i] as HostScene.blas_alt returns them, tris[i] BLAS i's TRI_DTYPE array"""
        keep = [(np.ascontiguousarray(t), {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in st.items()}) for t, st in zip(tris, structs)]
        arr = (AltAccelS * max(len(keep), 1))()
        for i, (t, st) in enumerate(keep):
            arr[i] = alt_desc(kind, t, st)
        self._ck(self.L.crt_upload_blas_accel(self.h, int(kind), arr, C.c_uint32(len(keep))))

    def upload_desc(self, kind, bvhs, textures, floor_texture, sky_texture, materials, light_T, light_invT, light_size=0.5,
                    floor_n=(0, 1, 0), floor_d=1.0, floor_invto=None, obj_mat_idx=None, tlas_nodes=None, update_what=None):
        """crt_upload_scene with arrays BUILT ELSEWHERE, in the reference's own layouts (INTEGRATION.md path A): bvhs = dicts with `nodes` (32-byte BVHNode
        records), `tris` (112-byte Tri records), `triIndices` (uint32) and, for two-level scenes, objIdx / matIdx / T / invT; textures = uint32 (h, w)
        arrays of 0x00RRGGBB texels; materials = (reflectivity, refractivity, absorption[3], texture index or -1).  Nothing of the repo's host front is involved."""
        keep = []
        bs = (BvhS * len(bvhs))()
        for i, b in enumerate(bvhs):
            nodes = np.ascontiguousarray(b["nodes"]); tris = np.ascontiguousarray(b["tris"]); idx = np.ascontiguousarray(b["triIndices"], np.uint32)
            assert nodes.dtype.itemsize == 32 and tris.dtype.itemsize == 112
            keep += [nodes, tris, idx]
            bs[i].nodes = nodes.ctypes.data; bs[i].nodesUsed = int(b.get("nodesUsed", len(nodes))); bs[i].triangles = tris.ctypes.data; bs[i].triCount = len(tris)
            bs[i].triangleIndices = idx.ctypes.data; bs[i].objIdx = int(b.get("objIdx", -1)); bs[i].matIdx = int(b.get("matIdx", -1))
            bs[i].T[:] = list(np.asarray(b.get("T", np.eye(4)), np.float32).reshape(16)); bs[i].invT[:] = list(np.asarray(b.get("invT", np.eye(4)), np.float32).reshape(16))
        ts = (TextureS * len(textures))()
        for i, t in enumerate(textures):
            t = np.ascontiguousarray(t, np.uint32); keep.append(t)
            ts[i].pixels = t.ctypes.data; ts[i].height, ts[i].width = t.shape
        ms = (MaterialS * max(len(materials), 1))()
        for i, (refl, refr, ab, tex) in enumerate(materials):
            ms[i].reflectivity = refl; ms[i].refractivity = refr; ms[i].absorption[:] = list(ab); ms[i].texture = tex
        d = SceneDescS()
        d.kind = kind; d.bvhs = bs; d.bvhCount = len(bvhs)
        if tlas_nodes is not None:
            tn = np.ascontiguousarray(tlas_nodes); keep.append(tn); d.tlasNodes = tn.ctypes.data; d.tlasNodeCount = len(tn)
        if obj_mat_idx is not None:
            om = np.ascontiguousarray(obj_mat_idx, np.int32); keep.append(om); d.objMatIdx = om.ctypes.data; d.objCount = len(om)
        d.materials = ms; d.materialCount = len(materials); d.textures = ts; d.textureCount = len(textures)
        d.floorTexture = floor_texture; d.skyTexture = sky_texture
        d.lightT[:] = list(np.asarray(light_T, np.float32).reshape(16)); d.lightInvT[:] = list(np.asarray(light_invT, np.float32).reshape(16)); d.lightSize = light_size
        d.floorN[:] = list(floor_n); d.floorD = floor_d
        if floor_invto is None:                                              # file_scene.cpp:16: Plane(.., texW / 100) with an integer division
            floor_invto = 1.0 / float(max(int(textures[floor_texture].shape[1]) // 100, 1)) if 0 <= floor_texture < len(textures) else 1.0
        d.floorInvto = floor_invto
        if update_what is not None:                                          # the same description to crt_update_scene (in-place update of the uploaded scene)
            self._ck(self.L.crt_update_scene(self.h, C.byref(d), C.c_uint32(update_what)))
            return
        self._ck(self.L.crt_upload_scene(self.h, C.byref(d)))

    def find_nearest(self, O, D, inside=None):
        O = np.asarray(O, np.float32).reshape(-1, 3)
        D = np.asarray(D, np.float32).reshape(-1, 3)
        rays = np.zeros(O.shape[0], RAY_DTYPE)
        rays["O"], rays["D"] = O, D
        if inside is not None:
            rays["inside"] = inside
        hits = np.zeros(O.shape[0], HIT_DTYPE)
        self._ck(self.L.crt_find_nearest(self.h, _p(rays), _p(hits), C.c_size_t(O.shape[0])))
        return hits

    def is_occluded(self, O, D, t, accel=0):
        """scene.IsOccluded per ray (crt_is_occluded, host buffers, synchronous): the light quad bounded by t, then the BVH / TLAS (accel 0) or the uploaded
        KD-tree / grid (ACCEL_KDTREE / ACCEL_GRID) over the whole ray.  t: one value or one per ray.  Returns a bool array."""
        O = np.asarray(O, np.float32).reshape(-1, 3)
        D = np.asarray(D, np.float32).reshape(-1, 3)
        rays = np.zeros(O.shape[0], SHADOW_RAY_DTYPE)
        rays["O"], rays["D"] = O, D
        rays["t"] = np.broadcast_to(np.asarray(t, np.float32).reshape(-1), (O.shape[0],))
        out = np.zeros(O.shape[0], np.int32)
        self._ck(self.L.crt_is_occluded(self.h, int(accel), _p(rays), _p(out), C.c_size_t(O.shape[0])))
        return out != 0

    def get_hit_info(self, O, D, hits):
        """scene.GetHitInfo + material->GetAlbedo per ray (crt_get_hit_info, host buffers, synchronous): O / D = [N, 3], hits = HIT_DTYPE records of any
        find-nearest entry.  Returns HIT_INFO_DTYPE records; a miss carries the sky colour as albedo and material MATERIAL_MISS."""
        O = np.asarray(O, np.float32).reshape(-1, 3)
        D = np.asarray(D, np.float32).reshape(-1, 3)
        rays = np.zeros(O.shape[0], RAY_DTYPE)
        rays["O"], rays["D"] = O, D
        hits = np.ascontiguousarray(hits, HIT_DTYPE).reshape(-1)
        if hits.shape[0] != O.shape[0]:
            raise ValueError("get_hit_info: one hit record per ray")
        out = np.zeros(O.shape[0], HIT_INFO_DTYPE)
        self._ck(self.L.crt_get_hit_info(self.h, _p(rays), _p(hits), _p(out), C.c_size_t(O.shape[0])))
        return out

    def get_sky_color(self, D):
        """scene.GetSkyColor per direction (crt_get_sky_color, host buffers, synchronous).  Returns [N, 3] float32."""
        D = np.asarray(D, np.float32).reshape(-1, 3)
        rays = np.zeros(D.shape[0], RAY_DTYPE)
        rays["D"] = D
        rgb = np.zeros((D.shape[0], 3), np.float32)
        self._ck(self.L.crt_get_sky_color(self.h, _p(rays), _p(rgb), C.c_size_t(D.shape[0])))
        return rgb

    def get_light(self):
        """(GetLightPos(), GetLightColor()) of the uploaded triangle scene, two float32 [3] arrays"""
        pos, col = (C.c_float * 3)(), (C.c_float * 3)()
        self._ck(self.L.crt_get_light(self.h, pos, col))
        return np.array(pos[:], np.float32), np.array(col[:], np.float32)

    # ---- the queries on device buffers (torch tensors; torch is imported only here) ----
    def _records(self, rays, O, D, last, last_is_int, what):
        """the [N, 7] 28-byte records (crt_ray / crt_shadow_ray) on the context's device: `rays` as given, or built from O, D and the last column"""
        import torch
        dev = torch.device("cuda", self.device)

        def on_device(x, name):
            if not isinstance(x, torch.Tensor) or x.device != dev:
                raise ValueError("%s: %s must be a torch tensor on %s" % (what, name, dev))
            if not x.is_contiguous():
                raise ValueError("%s: %s must be contiguous" % (what, name))
            return x

        if rays is not None:
            if O is not None or D is not None:
                raise ValueError("%s: pass either rays or O / D" % what)
            on_device(rays, "rays")
            if rays.dim() != 2 or rays.shape[1] != 7 or rays.dtype not in (torch.float32, torch.int32):
                raise ValueError("%s: rays must be [N, 7] float32 / int32 records" % what)
            return rays
        O, D = on_device(O, "O"), on_device(D, "D")
        if O.dtype != torch.float32 or D.dtype != torch.float32 or O.dim() != 2 or O.shape[1] != 3 or D.shape != O.shape:
            raise ValueError("%s: O and D must be [N, 3] float32" % what)
        n = O.shape[0]
        if last_is_int:                                                       # crt_ray.inside: an int32 bit pattern in the float32 record
            col = torch.zeros(n, dtype=torch.int32, device=dev) if last is None else torch.as_tensor(last, device=dev).to(torch.int32).expand(n)
            col = col.contiguous().view(torch.float32)
        else:                                                                 # crt_shadow_ray.t
            col = torch.as_tensor(last, dtype=torch.float32, device=dev).reshape(-1).expand(n)
        return torch.cat([O, D, col.reshape(n, 1)], 1).contiguous()

    def find_nearest_device(self, rays=None, O=None, D=None, inside=None, accel=0, stream=None):
        """crt_find_nearest_device: scene.FindNearest for rays that live on the GPU, enqueued on `stream` (default torch.cuda.current_stream()) without a host wait.
        rays = [N, 7] crt_ray records, or O / D = [N, 3] float32 (+ inside).  accel: 0 = BVH / TLAS / PrimitiveScene, ACCEL_KDTREE / ACCEL_GRID.
        Returns the [N, 7] float32 tensor of crt_hit records (hit_fields() splits it)."""
        import torch

        def run(st):
            r = self._records(rays, O, D, inside, True, "find_nearest_device")
            hits = torch.empty((r.shape[0], 7), dtype=torch.float32, device=r.device)
            self._ck(self.L.crt_find_nearest_device(self.h, int(accel), C.c_void_p(r.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_size_t(r.shape[0]), C.c_void_p(st.cuda_stream)))
            return hits
        return self._enqueue(stream, run)

    def is_occluded_device(self, rays=None, O=None, D=None, t=None, accel=0, stream=None):
        """crt_is_occluded_device: scene.IsOccluded for rays on the GPU, enqueued on `stream` (default torch.cuda.current_stream()) without a host wait.
        rays = [N, 7] crt_shadow_ray records, or O / D = [N, 3] float32 + t (one value or [N]).  Returns an [N] int32 tensor of 1 / 0."""
        import torch
        if rays is None and t is None:
            raise ValueError("is_occluded_device: t is required with O / D")

        def run(st):
            r = self._records(rays, O, D, t, False, "is_occluded_device")
            occ = torch.empty(r.shape[0], dtype=torch.int32, device=r.device)
            self._ck(self.L.crt_is_occluded_device(self.h, int(accel), C.c_void_p(r.data_ptr()), C.c_void_p(occ.data_ptr()), C.c_size_t(r.shape[0]), C.c_void_p(st.cuda_stream)))
            return occ
        return self._enqueue(stream, run)

    def get_hit_info_device(self, rays, hits, stream=None):
        """crt_get_hit_info_device: GetHitInfo + GetAlbedo for rays and hit records that live on the GPU ([N, 7] crt_ray records and the [N, 7] crt_hit records a
        find_nearest_device call returned), enqueued on `stream` (default torch.cuda.current_stream()) without a host wait.  Returns the [N, 12] float32 tensor of
        crt_hit_info records (hit_info_fields() splits it)."""
        import torch

        def run(st):
            r = self._records(rays, None, None, None, True, "get_hit_info_device")
            h = self._records(hits, None, None, None, True, "get_hit_info_device")
            if h.shape[0] != r.shape[0]:
                raise ValueError("get_hit_info_device: one hit record per ray")
            out = torch.empty((r.shape[0], 12), dtype=torch.float32, device=r.device)
            self._ck(self.L.crt_get_hit_info_device(self.h, C.c_void_p(r.data_ptr()), C.c_void_p(h.data_ptr()), C.c_void_p(out.data_ptr()), C.c_size_t(r.shape[0]), C.c_void_p(st.cuda_stream)))
            return out
        return self._enqueue(stream, run)

    def get_sky_color_device(self, rays=None, O=None, D=None, stream=None):
        """crt_get_sky_color_device: GetSkyColor for rays on the GPU ([N, 7] crt_ray records, or O / D = [N, 3] float32; only D is read), enqueued on `stream`.
        Returns an [N, 3] float32 tensor."""
        import torch

        def run(st):
            r = self._records(rays, O, D, None, True, "get_sky_color_device")
            rgb = torch.empty((r.shape[0], 3), dtype=torch.float32, device=r.device)
            self._ck(self.L.crt_get_sky_color_device(self.h, C.c_void_p(r.data_ptr()), C.c_void_p(rgb.data_ptr()), C.c_size_t(r.shape[0]), C.c_void_p(st.cuda_stream)))
            return rgb
        return self._enqueue(stream, run)

    def sample(self, O, D, seeds, inside=None, accel=0):
        """Renderer::Sample(ray, seed, 0) per ray (crt_sample, host buffers, synchronous): O / D = [N, 3] (D is used as given: hand in unit directions), seeds = [N]
        uint32 xorshift32 states, inside = None / one value / [N].  accel: 0 = BVH / TLAS / PrimitiveScene, ACCEL_KDTREE / ACCEL_GRID.
        Returns (rgb [N, 3] float32, seeds_out [N] uint32); a ray with seed 0, a non-finite component or D = 0 is not traced: NaN, its seed unchanged."""
        O = np.asarray(O, np.float32).reshape(-1, 3)
        D = np.asarray(D, np.float32).reshape(-1, 3)
        rays = np.zeros(O.shape[0], RAY_DTYPE)
        rays["O"], rays["D"] = O, D
        if inside is not None:
            rays["inside"] = inside
        s = np.array(seeds, dtype=np.uint32).reshape(-1)                        # a copy: the C entry updates it in place
        if s.shape[0] != O.shape[0]:
            raise ValueError("sample: one seed per ray")
        rgb = np.zeros((O.shape[0], 3), np.float32)
        self._ck(self.L.crt_sample(self.h, int(accel), _p(rays), _p(s), _p(rgb), C.c_size_t(O.shape[0])))
        return rgb, s

    def sample_device(self, rays=None, O=None, D=None, inside=None, seeds=None, accel=0, stream=None):
        """crt_sample_device: Renderer::Sample(ray, seed, 0) for rays that live on the GPU, enqueued on `stream` (default torch.cuda.current_stream()) without a host
        wait.  rays = [N, 7] crt_ray records, or O / D = [N, 3] float32 (+ inside); seeds = [N] int32 tensor on the context's device carrying the uint32 xorshift32
        states (the convention of the records' `inside` column).  Returns (rgb [N, 3] float32, seeds_out [N] int32) as new tensors; `seeds` is not modified."""
        import torch
        if not isinstance(seeds, torch.Tensor) or seeds.device != torch.device("cuda", self.device):
            raise ValueError("sample_device: seeds must be a torch tensor on cuda:%d" % self.device)
        if seeds.dtype != torch.int32 or seeds.dim() != 1 or not seeds.is_contiguous():
            raise ValueError("sample_device: seeds must be a contiguous [N] int32 tensor (the uint32 bit patterns)")

        def run(st):
            r = self._records(rays, O, D, inside, True, "sample_device")
            if seeds.shape[0] != r.shape[0]:
                raise ValueError("sample_device: one seed per ray")
            s = seeds.clone()                                                 # on the stream: the in/out argument
            rgb = torch.empty((r.shape[0], 3), dtype=torch.float32, device=r.device)
            self._ck(self.L.crt_sample_device(self.h, int(accel), C.c_void_p(r.data_ptr()), C.c_void_p(s.data_ptr()), C.c_void_p(rgb.data_ptr()), C.c_size_t(r.shape[0]), C.c_void_p(st.cuda_stream)))
            return rgb, s
        return self._enqueue(stream, run)

    def sample_resident_lanes(self, accel=0):
        """the lanes a full crt_sample launch over this scene holds at once (tools / tests: an n above it makes every wavefront draw from the cursor again)"""
        n = C.c_uint32()
        self._ck(self.L.crt_debug_sample_resident_lanes(self.h, int(accel), C.byref(n)))
        return int(n.value)

    def trace(self, rays, accel=0, counts=False):
        """The Whitted Renderer::Trace(ray, 0) per ray (crt_trace, host buffers, synchronous): rays = an [N] RAY_DTYPE array (D is used as given).  accel: 0 = BVH /
        TLAS, ACCEL_KDTREE / ACCEL_GRID.  Returns rgb [N, 3] float32, or with counts=True (rgb, traversed [N] int32, tested [N] int32): the depth-0 ray's
        Ray::traversed / Ray::tested.  A ray with a non-finite component or D = 0 is not traced: NaN, and -1 in both counts."""
        rays = np.ascontiguousarray(rays)
        if rays.dtype != RAY_DTYPE or rays.ndim != 1:
            raise ValueError("trace: rays must be a one-dimensional RAY_DTYPE array")
        n = rays.shape[0]
        rgb = np.zeros((n, 3), np.float32)
        trav, tested = (np.zeros(n, np.int32), np.zeros(n, np.int32)) if counts else (None, None)
        self._ck(self.L.crt_trace(self.h, int(accel), _p(rays), _p(rgb), _p(trav) if counts else None, _p(tested) if counts else None, C.c_size_t(n)))
        return (rgb, trav, tested) if counts else rgb

    def trace_device(self, rays, accel=0, counts=False, stream=None):
        """crt_trace_device: the Whitted Renderer::Trace(ray, 0) for rays that live on the GPU ([N, 7] crt_ray records), enqueued on `stream` (default
        torch.cuda.current_stream()) without a host wait.  Returns rgb [N, 3] float32, or with counts=True (rgb, traversed [N] int32, tested [N] int32), new tensors."""
        import torch

        def run(st):
            r = self._records(rays, None, None, None, True, "trace_device")
            n = r.shape[0]
            rgb = torch.empty((n, 3), dtype=torch.float32, device=r.device)
            trav = torch.empty(n, dtype=torch.int32, device=r.device) if counts else None
            tested = torch.empty(n, dtype=torch.int32, device=r.device) if counts else None
            self._ck(self.L.crt_trace_device(self.h, int(accel), C.c_void_p(r.data_ptr()), C.c_void_p(rgb.data_ptr()), C.c_void_p(trav.data_ptr()) if counts else None,
                                             C.c_void_p(tested.data_ptr()) if counts else None, C.c_size_t(n), C.c_void_p(st.cuda_stream)))
            return (rgb, trav, tested) if counts else rgb
        return self._enqueue(stream, run)

    def trace_resident_lanes(self, accel=0):
        """the lanes a full crt_trace launch over this scene holds at once (tools / tests: an n above it makes every wavefront draw from the cursor again)"""
        n = C.c_uint32()
        self._ck(self.L.crt_debug_trace_resident_lanes(self.h, int(accel), C.byref(n)))
        return int(n.value)

    def _positions(self, positions, what):
        """the device pointer and triangle count of a refit's positions: a contiguous float32 tensor [triCount, 3, 3] or [triCount, 9] on the context's device"""
        import torch
        if not isinstance(positions, torch.Tensor) or positions.device != torch.device("cuda", self.device):
            raise ValueError("%s: positions must be a torch tensor on cuda:%d" % (what, self.device))
        if positions.dtype != torch.float32 or not positions.is_contiguous() or positions.dim() < 2 or tuple(positions.shape[1:]) not in ((3, 3), (9,)):
            raise ValueError("%s: positions must be a contiguous float32 tensor of shape [triCount, 3, 3] or [triCount, 9]" % what)
        return C.c_void_p(positions.data_ptr()), C.c_uint32(positions.shape[0])

    def refit_device(self, bvh, positions, stream=None, root_box=True):
        """crt_refit_device: BVH::Refit of uploaded BVH `bvh` on the GPU from `positions` (vertex0, vertex1, vertex2 per triangle, the reference's triangle order),
        enqueued on `stream` (default torch.cuda.current_stream()); returns once the refitted root has been read back.  Returns node 0's box as a [2, 3] float32
        array (aabbMin, aabbMax), or None with root_box=False.  Two-level scenes: the TLAS is the caller's to rebuild (HostScene.refit_device does it)."""
        def run(st):
            ptr, n = self._positions(positions, "refit_device")
            box = (C.c_float * 6)()
            self._ck(self.L.crt_refit_device(self.h, C.c_uint32(bvh), ptr, n, C.c_void_p(st.cuda_stream), box if root_box else None))
            return np.array(box[:], np.float32).reshape(2, 3) if root_box else None
        return self._enqueue(stream, run)

    def _transforms(self, T, what):
        """the device pointer and instance count of a set of transforms: a contiguous float32 tensor [N, 16] or [N, 4, 4] (row-major mat4s) on the context's device"""
        import torch
        if not isinstance(T, torch.Tensor) or T.device != torch.device("cuda", self.device):
            raise ValueError("%s: the transforms must be a torch tensor on cuda:%d" % (what, self.device))
        if T.dtype != torch.float32 or not T.is_contiguous() or T.dim() < 2 or tuple(T.shape[1:]) not in ((16,), (4, 4)):
            raise ValueError("%s: the transforms must be a contiguous float32 tensor of shape [N, 16] or [N, 4, 4]" % what)
        return C.c_void_p(T.data_ptr()), C.c_uint32(T.shape[0])

    def update_transforms_device(self, T, stream=None):
        """crt_update_transforms_device: BLASBVH::SetTransform(T[i]) of every instance of a two-level scene + TLASBVH::Build on the GPU, from a tensor of row-major
        mat4s ([N, 16] or [N, 4, 4], rigid), enqueued on `stream` (default torch.cuda.current_stream()); returns once the build has been read back.  Returns the
        rebuilt TLASBVH::tlasNode array (TLAS_DTYPE, 2 N records)."""
        def run(st):
            ptr, n = self._transforms(T, "update_transforms_device")
            nodes = np.zeros(2 * n.value, TLAS_DTYPE)
            self._ck(self.L.crt_update_transforms_device(self.h, ptr, n, C.c_void_p(st.cuda_stream), _p(nodes)))
            return nodes
        return self._enqueue(stream, run)

    def build_grid_device(self, bvh, positions, stream=None):
        """crt_build_grid_device: Grid::Build / BLASGrid::Build of uploaded BVH `bvh` on the GPU from `positions` (refit_device's tensor), enqueued on `stream` (default
        torch.cuda.current_stream()); returns once the bounds and the reference count have been read back.  The grid becomes the FileScene's ACCEL_GRID structure (its
        KD-tree is marked absent), or BLAS `bvh`'s part of a two-level scene's uploaded grid set, which is live again once every refitted BLAS has been rebuilt.  The
        BVH / TLAS are not touched: refit_device (+ update_transforms_device) with the same positions keeps them in step."""
        def run(st):
            ptr, n = self._positions(positions, "build_grid_device")
            self._ck(self.L.crt_build_grid_device(self.h, C.c_uint32(bvh), ptr, n, C.c_void_p(st.cuda_stream)))
        return self._enqueue(stream, run)

    def get_grid(self, bvh=0):
        """crt_get_grid: the live grid of a FileScene (bvh 0) or of BLAS `bvh` of a two-level set, uploaded or device-built, in HostScene.build_alt's layout"""
        res = np.zeros(3, np.int32); f = np.zeros(9, np.float32); cells, refs = C.c_uint32(), C.c_uint32()
        fp = f.ctypes.data
        self._ck(self.L.crt_get_grid(self.h, C.c_uint32(bvh), _p(res), C.c_void_p(fp), C.c_void_p(fp + 12), C.c_void_p(fp + 24), C.byref(cells), C.byref(refs), None, None))
        start = np.zeros(cells.value + 1, np.uint32); r = np.zeros(max(refs.value, 1), np.int32)
        self._ck(self.L.crt_get_grid(self.h, C.c_uint32(bvh), None, None, None, None, None, None, _p(start), _p(r)))
        return dict(resolution=res, cellSize=f[0:3].copy(), boundsMin=f[3:6].copy(), boundsMax=f[6:9].copy(), cellStart=start, refs=r[:refs.value])

    def build_kdtree_device(self, bvh, positions, stream=None):
        """crt_build_kdtree_device: KDTree::Build / BLASKDTree::Build of uploaded BVH `bvh` on the GPU from `positions` (refit_device's tensor), enqueued on `stream`
        (default torch.cuda.current_stream()); returns once the last level's counts have been read back (one host wait per level of the tree).  The tree becomes the
        FileScene's ACCEL_KDTREE structure (its grid is marked absent), or BLAS `bvh`'s part of a two-level scene's uploaded KD set, which is live again once every
        refitted BLAS has been rebuilt.  The BVH / TLAS are not touched: refit_device (+ update_transforms_device) with the same positions keeps them in step."""
        def run(st):
            ptr, n = self._positions(positions, "build_kdtree_device")
            self._ck(self.L.crt_build_kdtree_device(self.h, C.c_uint32(bvh), ptr, n, C.c_void_p(st.cuda_stream)))
        return self._enqueue(stream, run)

    def get_kdtree(self, bvh=0):
        """crt_get_kdtree: the live KD-tree of a FileScene (bvh 0) or of BLAS `bvh` of a two-level set, uploaded or device-built: dict(nodes, refs, height)"""
        nn, nr, h = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(self.L.crt_get_kdtree(self.h, C.c_uint32(bvh), C.byref(nn), C.byref(nr), C.byref(h), None, None))
        nodes = np.zeros(nn.value, KD_NODE_DTYPE); r = np.zeros(max(nr.value, 1), np.uint32)
        self._ck(self.L.crt_get_kdtree(self.h, C.c_uint32(bvh), None, None, None, _p(nodes), _p(r)))
        return dict(nodes=nodes, refs=r[:nr.value], height=int(h.value))

    def build_bvh_device(self, bvh, positions, stream=None, root_box=True):
        """crt_build_bvh_device: BVH::Build (binned SAH) of uploaded BVH `bvh` on the GPU from `positions` (refit_device's tensor), enqueued on `stream` (default
        torch.cuda.current_stream()); returns once the new tree has been read back into the context's mirror (one host wait per level of the tree before that).  The
        scene is then what a fresh upload of the host-rebuilt scene gives.  Returns node 0's box as refit_device does.  Two-level scenes: the TLAS is the caller's to
        rebuild (update_transforms_device, or HostScene.build_bvh_device)."""
        def run(st):
            ptr, n = self._positions(positions, "build_bvh_device")
            box = (C.c_float * 6)()
            self._ck(self.L.crt_build_bvh_device(self.h, C.c_uint32(bvh), ptr, n, C.c_void_p(st.cuda_stream), box if root_box else None))
            return np.array(box[:], np.float32).reshape(2, 3) if root_box else None
        return self._enqueue(stream, run)

    def get_bvh(self, bvh=0):
        """crt_get_bvh: BVH `bvh` of the live scene in the reference's form, reconstructed from the device's geometry buffer:
        dict(nodes (NODE_DTYPE, nodesUsed records), indices, nodesUsed, maxDepth, height)"""
        used, depth, h = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(self.L.crt_get_bvh(self.h, C.c_uint32(bvh), C.byref(used), C.byref(depth), C.byref(h), None, None))
        nodes = np.zeros(used.value, NODE_DTYPE)
        self._ck(self.L.crt_get_bvh(self.h, C.c_uint32(bvh), None, None, None, _p(nodes), None))
        idx = np.zeros(int(nodes["triCount"].sum()), np.uint32)                 # every triangle is in exactly one leaf
        self._ck(self.L.crt_get_bvh(self.h, C.c_uint32(bvh), None, None, None, None, _p(idx)))
        return dict(nodes=nodes, indices=idx, nodesUsed=int(used.value), maxDepth=int(depth.value), height=int(h.value))

    def _enqueue(self, stream, run):
        """run(st) on the torch stream `stream` (default: the current one).  Torch's default stream has the handle 0, which the ABI reads as the context's own
        stream: on it the query runs on a side stream that waits for it and that it waits for in turn (events, no host wait)."""
        import torch
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if st.cuda_stream != 0:
            with torch.cuda.stream(st):
                return run(st)
        side = getattr(self, "_side_stream", None)
        if side is None:
            side = self._side_stream = torch.cuda.Stream(device=self.device)
        side.wait_stream(st)
        with torch.cuda.stream(side):
            out = run(side)
        st.wait_stream(side)
        for t in (out if isinstance(out, tuple) else (out,)):
            if isinstance(t, torch.Tensor):
                t.record_stream(st)                                           # allocated on the side stream, consumed on st
        return out

    def counters(self):
        c = CountersS()
        self._ck(self.L.crt_get_counters(self.h, C.byref(c)))
        return {n: int(getattr(c, n)) for n, _ in c._fields_}

    def reset_counters(self):
        self._ck(self.L.crt_reset_counters(self.h))

    def timing(self):
        t = TimingS()
        self._ck(self.L.crt_get_timing(self.h, C.byref(t)))
        return dict(render_kernel_ms=t.render_kernel_ms, resolve_kernel_ms=t.resolve_kernel_ms, render_launches=t.render_launches, pool_launches=t.pool_launches, split_launches=t.split_launches)

    def pool_lds(self, frames):
        """crt_debug_pool_lds: (LDS bytes one render_pool_kernel wavefront of a launch of `frames` frames on the uploaded scene asks for, the per-workgroup limit
        the library holds it to, the width of the scene's pool references: 16, 32 or 0 = none)"""
        self.L.crt_debug_pool_lds.restype = C.c_int
        self.L.crt_debug_pool_lds.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        b, lim, bits = C.c_uint32(), C.c_uint32(), C.c_uint32()
        if self.L.crt_debug_pool_lds(self.h, int(frames), C.byref(b), C.byref(lim), C.byref(bits)) != 0:
            raise CrtError(-3, "pool_lds: no scene uploaded")
        return b.value, lim.value, bits.value

    def arith_forms(self, what, records=None, n=None, seed=1):
        """crt_debug_arith_forms: a short arithmetic form of dev_common.h against the form it stands for, on the device (device/probe.hip probe_arith_kernel lists
        `what` and the record layouts).  records: uint32 [k, words] read first (sweeps: the 4-word header), then generated records up to n in all.  Returns
        (differing records, index of the lowest or None, its operands [3], old result [2], new result [2]) — the last three as uint32 bit patterns."""
        f = self.L.crt_debug_arith_forms
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        r = None if records is None else np.ascontiguousarray(records, np.uint32)
        n_in = 0 if (r is None or what == 3) else len(r)
        out = np.zeros(9, np.uint32)
        self._ck(f(self.h, int(what), None if r is None else _p(r), n_in, n_in if n is None else int(n), int(seed), _p(out)))
        return int(out[0]), (None if out[0] == 0 else int(out[1])), out[2:5].copy(), out[5:7].copy(), out[7:9].copy()

    def job_costs(self):
        """crt_debug_job_costs: (tile costs uint32 [owned tiles], pool window ticks, sky window ticks) as the planner holds them; CrtError (state) until a
        measuring job's costs have been adopted or set_job_costs has installed some, and again after whatever drops them (camera, scene, accelerator)"""
        f = self.L.crt_debug_job_costs
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        n = getattr(self, "tiles", None)
        if n is None: n = len(self.tile_classes())
        out = np.zeros(max(1, n), np.uint32)
        pool, sky = C.c_double(0), C.c_double(0)
        rc = f(self.h, _p(out), C.byref(pool), C.byref(sky))
        if rc != 0:
            raise CrtError(rc, "crt_debug_job_costs: no tile costs held")
        return out[:n], pool.value, sky.value

    def set_job_costs(self, cost, pool_window_ticks, sky_window_ticks=0.0):
        """crt_debug_set_job_costs: installs tile costs (one per owned tile, local tile order, 100 MHz ticks) and the machine time of one window of the image under
        the pool / of its sky launch, as if a measuring job had left them: the next job is planned from them.  cost=None passes NULL (refused)."""
        f = self.L.crt_debug_set_job_costs
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double]
        c = None if cost is None else np.ascontiguousarray(cost, np.uint32)
        n = getattr(self, "tiles", None)
        if c is not None and n is not None and len(c) != n:
            raise ValueError("set_job_costs: %d costs for %d owned tiles" % (len(c), n))
        self._ck(f(self.h, None if c is None else _p(c), float(pool_window_ticks), float(sky_window_ticks)))

    def tile_classes(self, ex=False):
        """crt_debug_tile_classes: the pool kernel's tile classes as the device holds them, one byte per owned tile (TILE_NO_LIGHT | TILE_NO_FLOOR | TILE_NO_TREE);
        ex: crt_debug_tile_classes_ex, the whole byte (TILE_FLOOR_SURE as well)"""
        f = self.L.crt_debug_tile_classes_ex if ex else self.L.crt_debug_tile_classes
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        n = f(self.h, None, 0)
        if n < 0:
            self._ck(n)
        out = np.zeros(n, np.uint8)
        if n:
            rc = f(self.h, _p(out), n)
            if rc < 0:
                self._ck(rc)
        return out

    def tile_clocks(self, tile_count):
        a = np.zeros((tile_count, 2), np.uint64)
        self._ck(self.L.crt_get_tile_clocks(self.h, _p(a)))
        return a

    def bind_accumulator(self, device_ptr):
        self._ck(self.L.crt_bind_accumulator(self.h, C.c_void_p(device_ptr)))

    def accumulator_device_ptr(self):
        p = C.c_void_p()
        self._ck(self.L.crt_accumulator_device_ptr(self.h, C.byref(p)))
        return p.value

def hit_fields(hits):
    """the seven crt_hit fields of an [N, 7] record tensor from find_nearest_device, as views: t / u / v float32, objIdx / triIdx / traversed / tested int32"""
    import torch
    i = hits.view(torch.int32)
    return dict(t=hits[:, 0], u=hits[:, 1], v=hits[:, 2], objIdx=i[:, 3], triIdx=i[:, 4], traversed=i[:, 5], tested=i[:, 6])


def hit_info_fields(info):
    """the fields of an [N, 12] crt_hit_info record tensor from get_hit_info_device, as views: I / N / albedo [N, 3] float32, u / v float32, material int32"""
    import torch
    return dict(I=info[:, 0:3], material=info.view(torch.int32)[:, 3], N=info[:, 4:7], u=info[:, 7], albedo=info[:, 8:11], v=info[:, 11])


class HostScene:
    """FileScene / TLASFileScene built on the CPU by the C++ host front (XML + OBJ + textures + SAH-BVH / TLAS)."""

    def __init__(self, xml_path, kind, base_dir=None):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.crt_host_scene_load(xml_path.encode(), int(kind), (base_dir or "").encode(), C.byref(h))
        if rc != 0:
            raise CrtError(rc, self.L.crt_host_last_error().decode())
        self.h = h
        self.kind = int(kind)

    def close(self):
        if getattr(self, "h", None):
            self.L.crt_host_scene_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise CrtError(rc, self.L.crt_host_last_error().decode())

    def upload(self, ctx):
        self._ck(self.L.crt_host_scene_upload(self.h, ctx.h))

    def triangle_count(self):
        return self.L.crt_host_scene_triangle_count(self.h)

    def bvh_count(self):
        return self.L.crt_host_scene_bvh_count(self.h)

    def bvh(self, i=0):
        nu, tc, md = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(self.L.crt_host_scene_bvh_info(self.h, i, C.byref(nu), C.byref(tc), C.byref(md)))
        nodes = np.zeros(nu.value, NODE_DTYPE)
        idx = np.zeros(tc.value, np.uint32)
        tris = np.zeros(tc.value, TRI_DTYPE)
        self._ck(self.L.crt_host_scene_bvh_copy(self.h, i, _p(nodes), _p(idx), _p(tris)))
        return dict(nodes=nodes, triIndices=idx, tris=tris, nodesUsed=nu.value, maxDepth=md.value)

    def move_and_refit(self, i, positions):
        """BVH::Refit for moved vertices: positions = (triCount, 3, 3) floats in the reference's triangle order; upload() again afterwards"""
        positions = np.ascontiguousarray(positions, np.float32)
        self._ck(self.L.crt_host_scene_bvh_move_and_refit(self.h, int(i), _p(positions), C.c_uint32(positions.shape[0])))

    def refit_device(self, ctx, i, positions, stream=None):
        """crt_host_scene_bvh_refit_device: Refit of BVH i on the GPU from a positions tensor (Context.refit_device's), then node 0's new box on the host and, for a
        two-level scene, SetTransform + TLASBVH::Build + update(UPDATE_TRANSFORMS).  The host arrays of BVH i are stale afterwards: upload / update(UPDATE_BOUNDS)
        raise until move_and_refit(i, ...) brings positions to the host again."""
        def run(st):
            ptr, n = ctx._positions(positions, "refit_device")
            self._ck(self.L.crt_host_scene_bvh_refit_device(self.h, ctx.h, int(i), ptr, n, C.c_void_p(st.cuda_stream)))
        return ctx._enqueue(stream, run)

    def set_transforms_device(self, ctx, T, stream=None):
        """crt_host_scene_update_transforms_device: every instance's transform from a tensor on the GPU (Context.update_transforms_device's), the TLAS rebuilt there;
        the host scene's T, invT, world bounds and TLAS follow (blas_transform(i), tlas()), so no update(ctx, UPDATE_TRANSFORMS) is needed."""
        def run(st):
            ptr, n = ctx._transforms(T, "set_transforms_device")
            if n.value != self.bvh_count():
                raise ValueError("set_transforms_device: %d transforms for %d instances" % (n.value, self.bvh_count()))
            self._ck(self.L.crt_host_scene_update_transforms_device(self.h, ctx.h, ptr, C.c_void_p(st.cuda_stream)))
        return ctx._enqueue(stream, run)

    def build_grid_device(self, ctx, i, positions, stream=None):
        """crt_host_scene_build_grid_device: the grid of BVH i rebuilt on the GPU from a positions tensor (Context.build_grid_device's), then this scene's grid mirror
        refreshed from the device: blas_alt(ACCEL_GRID, i) / the FileScene's alt arrays describe the live grid."""
        def run(st):
            ptr, n = ctx._positions(positions, "build_grid_device")
            self._ck(self.L.crt_host_scene_build_grid_device(self.h, ctx.h, int(i), ptr, n, C.c_void_p(st.cuda_stream)))
        return ctx._enqueue(stream, run)

    def build_bvh_device(self, ctx, i, positions, stream=None):
        """crt_host_scene_build_bvh_device: BVH i rebuilt on the GPU from a positions tensor (Context.build_bvh_device's), this scene's triangles moved and its tree
        rebuilt on the host alike (the two trees are identical), and a TLAS scene's TLAS rebuilt on the host and sent."""
        def run(st):
            ptr, n = ctx._positions(positions, "build_bvh_device")
            self._ck(self.L.crt_host_scene_build_bvh_device(self.h, ctx.h, int(i), ptr, n, C.c_void_p(st.cuda_stream)))
        return ctx._enqueue(stream, run)

    def move_and_rebuild(self, i, positions):
        """crt_host_scene_bvh_move_and_rebuild: new vertex positions ((n, 3, 3) float32) for BVH i, centroids recomputed, BVH::Build on the host (+ TLAS)"""
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 9)
        self._ck(self.L.crt_host_scene_bvh_move_and_rebuild(self.h, int(i), _p(pos), C.c_uint32(len(pos))))

    def build_kdtree_device(self, ctx, i, positions, stream=None):
        """crt_host_scene_build_kdtree_device: the KD-tree of BVH i rebuilt on the GPU from a positions tensor (Context.build_kdtree_device's), then this scene's KD
        mirror refreshed from the device: blas_alt(ACCEL_KDTREE, i) / kdtree() describe the live tree."""
        def run(st):
            ptr, n = ctx._positions(positions, "build_kdtree_device")
            self._ck(self.L.crt_host_scene_build_kdtree_device(self.h, ctx.h, int(i), ptr, n, C.c_void_p(st.cuda_stream)))
        return ctx._enqueue(stream, run)

    def kdtree(self):
        """the FileScene's KD-tree mirror (after build_alt(ACCEL_KDTREE) or build_kdtree_device), in build_alt's layout"""
        return self._alt(ACCEL_KDTREE, lambda info: self.L.crt_host_scene_alt_info(self.h, ACCEL_KDTREE, info),
                         lambda a, b, c: self.L.crt_host_scene_alt_copy(self.h, ACCEL_KDTREE, a, b, c))

    def grid(self):
        """the FileScene's grid mirror (after build_alt(ACCEL_GRID) or build_grid_device), in build_alt's layout"""
        return self._alt(ACCEL_GRID, lambda info: self.L.crt_host_scene_alt_info(self.h, ACCEL_GRID, info),
                         lambda a, b, c: self.L.crt_host_scene_alt_copy(self.h, ACCEL_GRID, a, b, c))

    def build_alt(self, kind):
        """KDTree::Build / Grid::Build over the FileScene's triangles on the host; returns the flattened structure (the layout crt_upload_alt_accel takes).
        TLAS scene: BLASKDTree / BLASGrid per BLAS over its own triangles; returns the list of blas_alt(kind, i)."""
        self._ck(self.L.crt_host_scene_build_alt(self.h, int(kind)))
        if self.kind == 1:
            return [self.blas_alt(kind, i) for i in range(self.bvh_count())]
        return self._alt(kind, lambda info: self.L.crt_host_scene_alt_info(self.h, int(kind), info),
                         lambda a, b, c: self.L.crt_host_scene_alt_copy(self.h, int(kind), a, b, c))

    def blas_alt(self, kind, i):
        """BLAS i's BLASKDTree / BLASGrid of a TLAS scene (after build_alt), in build_alt's layout"""
        return self._alt(kind, lambda info: self.L.crt_host_scene_blas_alt_info(self.h, int(kind), int(i), info),
                         lambda a, b, c: self.L.crt_host_scene_blas_alt_copy(self.h, int(kind), int(i), a, b, c))

    def _alt(self, kind, info_fn, copy_fn):
        info = (C.c_uint32 * 4)()
        self._ck(info_fn(info))
        if kind == ACCEL_KDTREE:
            nodes = np.zeros(info[0], KD_NODE_DTYPE); refs = np.zeros(max(info[1], 1), np.uint32)
            self._ck(copy_fn(_p(nodes), _p(refs), None))
            return dict(nodes=nodes, refs=refs[:info[1]], maxDepth=int(info[2]), nodesUsed=int(info[3]))
        res = np.array([info[0], info[1], info[2]], np.int32)
        start = np.zeros(int(res.prod()) + 1, np.uint32); refs = np.zeros(max(info[3], 1), np.int32); f = np.zeros(9, np.float32)
        self._ck(copy_fn(_p(start), _p(refs), _p(f)))
        return dict(resolution=res, cellSize=f[0:3].copy(), boundsMin=f[3:6].copy(), boundsMax=f[6:9].copy(), cellStart=start, refs=refs[:info[3]])

    def upload_alt(self, ctx, kind):
        self._ck(self.L.crt_host_scene_upload_alt(self.h, ctx.h, int(kind)))

    def set_transform(self, i, T):
        """BLASBVH::SetTransform(T) of instance i (T = 4x4 row-major, rigid) + TLASBVH::Build on the host; update(ctx, UPDATE_TRANSFORMS) moves it to the device"""
        T = np.ascontiguousarray(T, np.float32).reshape(16)
        self._ck(self.L.crt_host_scene_set_transform(self.h, int(i), _p(T)))

    def look(self):
        """the scene's look as one record of look_records ([crt_look_words(materialCount)] uint32): the file's, or the last set_look's"""
        n = C.c_uint32()
        self._ck(self.L.crt_host_scene_look(self.h, None, C.byref(n)))
        rec = np.zeros(n.value, np.uint32)
        self._ck(self.L.crt_host_scene_look(self.h, _p(rec), C.byref(n)))
        return rec

    def set_look(self, look):
        """takes a look over (light quad, floor / skydome texture index, materials) so that the next upload describes the scene with it; the device is not touched
        (Context.update_look changes a live scene's look in place)"""
        rec = np.ascontiguousarray(look, np.uint32).reshape(-1)
        if rec.shape[0] != self.look().shape[0]:
            raise ValueError("set_look: the record has %d words, the scene's look %d" % (rec.shape[0], self.look().shape[0]))
        self._ck(self.L.crt_host_scene_set_look(self.h, _p(rec)))

    def update(self, ctx, what):
        """in-place device update (crt_update_scene): UPDATE_TRANSFORMS after set_transform, UPDATE_BOUNDS after move_and_refit; no re-upload"""
        self._ck(self.L.crt_host_scene_update(self.h, ctx.h, C.c_uint32(what)))

    def blas_transform(self, i):
        T, invT, lo, hi = np.zeros(16, np.float32), np.zeros(16, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._ck(self.L.crt_host_scene_blas_transform(self.h, i, _p(T), _p(invT), _p(lo), _p(hi)))
        return T, invT, lo, hi

    def tlas(self):
        nodes = np.zeros(2 * self.bvh_count(), TLAS_DTYPE)
        nu = C.c_uint32()
        self._ck(self.L.crt_host_scene_tlas_copy(self.h, _p(nodes), C.byref(nu)))
        return nodes, nu.value


class PrimitiveSceneS(C.Structure):
    _fields_ = [("quadT", C.c_float * 16), ("quadInvT", C.c_float * 16), ("quadSize", C.c_float), ("spherePos", C.c_float * 3),
                ("cubeMin", C.c_float * 3), ("cubeMax", C.c_float * 3), ("cubeM", C.c_float * 16), ("cubeInvM", C.c_float * 16),
                ("torusT", C.c_float * 16), ("torusInvT", C.c_float * 16), ("torusRt2", C.c_float), ("torusRc2", C.c_float), ("torusR2", C.c_float),
                ("reflectivity", C.c_float * 11), ("refractivity", C.c_float * 11), ("absorption", C.c_float * 33), ("red", TextureS), ("blue", TextureS)]


class HostPrimitiveScene:
    """PrimitiveScene of the reference (infra/scene/primitive_scene.cpp): constructor, SetTime, upload through crt_upload_primitive_scene"""

    def __init__(self, assets_dir=None):
        self.L = lib()
        h = C.c_void_p()
        r = self.L.crt_host_primitive_scene_create(assets_dir.encode() if assets_dir else None, C.byref(h))
        if r != 0:
            raise CrtError(r, self.L.crt_host_last_error().decode())
        self.h = h

    def set_time(self, t):
        self.L.crt_host_primitive_scene_set_time(self.h, C.c_float(t))

    def desc(self):
        d = PrimitiveSceneS()
        self.L.crt_host_primitive_scene_desc(self.h, C.byref(d))
        return d

    def state(self):
        """the 108 floats of the oracle's orc_prim_state: quad T, invT, cube M, invM, torus T, invT, sphere position, rt2, rc2, r2, cube box"""
        d = self.desc()
        return np.array(list(d.quadT) + list(d.quadInvT) + list(d.cubeM) + list(d.cubeInvM) + list(d.torusT) + list(d.torusInvT) + list(d.spherePos)
                        + [d.torusRt2, d.torusRc2, d.torusR2] + list(d.cubeMin) + list(d.cubeMax), np.float32)

    def upload(self, ctx):
        r = self.L.crt_host_primitive_scene_upload(self.h, ctx.h)
        if r != 0:
            raise CrtError(r, self.L.crt_last_error(ctx.h).decode())

    def desc_with_state(self, state):
        """desc() with the 108 floats of state() overwritten (tests: arbitrary matrices, e.g. identity cube / torus transforms); the wall images stay this scene's"""
        st = np.ascontiguousarray(state, np.float32).reshape(108)
        d = self.desc()
        for k, name in enumerate(("quadT", "quadInvT", "cubeM", "cubeInvM", "torusT", "torusInvT")):
            getattr(d, name)[:] = [float(v) for v in st[16 * k:16 * k + 16]]
        d.spherePos[:] = [float(v) for v in st[96:99]]
        d.torusRt2, d.torusRc2, d.torusR2 = float(st[99]), float(st[100]), float(st[101])
        d.cubeMin[:] = [float(v) for v in st[102:105]]
        d.cubeMax[:] = [float(v) for v in st[105:108]]
        return d

    def upload_desc(self, ctx, d):
        """crt_upload_primitive_scene with a description the caller has edited (the C ABI accepts any); this scene must outlive the call (it owns the wall images)"""
        self.L.crt_upload_primitive_scene.argtypes = [C.c_void_p, C.POINTER(PrimitiveSceneS)]
        r = self.L.crt_upload_primitive_scene(ctx.h, C.byref(d))
        if r != 0:
            raise CrtError(r, self.L.crt_last_error(ctx.h).decode())

    def close(self):
        if self.h:
            self.L.crt_host_primitive_scene_free(self.h); self.h = None


class HostRenderer:
    """Renderer facade: Init / Tick / ClearAccumulator with the reference's public members."""

    def __init__(self, scene, width, height, device=0):
        self.L = lib()
        self.scene = scene
        h = C.c_void_p()
        rc = self.L.crt_host_renderer_create(scene.h, width, height, device, C.byref(h))
        if rc != 0:
            raise CrtError(rc, self.L.crt_host_last_error().decode())
        self.h = h
        self.W, self.H = width, height

    def close(self):
        if getattr(self, "h", None):
            self.L.crt_host_renderer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise CrtError(rc, self.L.crt_host_last_error().decode())

    def init(self):
        self._ck(self.L.crt_host_renderer_init(self.h))

    def set_camera(self, position, target):
        self._ck(self.L.crt_host_renderer_set_camera(self.h, _f3(position), _f3(target)))

    def set_passes(self, passes):
        self._ck(self.L.crt_host_renderer_set_passes(self.h, passes))

    def clear(self):
        self._ck(self.L.crt_host_renderer_clear(self.h))

    def tick(self, dt=0.0):
        self._ck(self.L.crt_host_renderer_tick(self.h, C.c_float(dt)))

    def render(self, frames):
        self._ck(self.L.crt_host_renderer_render(self.h, frames))

    def tick_whitted(self):
        self._ck(self.L.crt_host_renderer_tick_whitted(self.h))

    def set_inspect(self, traversal=False, tests=False):
        """the Whitted Renderer's m_inspectTraversal / m_inspectIntersectionTest (traversal wins if both are set)"""
        self._ck(self.L.crt_host_renderer_set_inspect(self.h, int(bool(traversal)), int(bool(tests))))

    def whitted_metrics(self):
        """the report of the last tick_whitted: crt_whitted_metrics' fields (peaks as carried so far) + averageTraversal / averageTests (float32)"""
        m = WhittedMetricsS(); a, b = C.c_float(), C.c_float()
        self._ck(self.L.crt_host_renderer_whitted_metrics(self.h, C.byref(m), C.byref(a), C.byref(b)))
        d = m.as_dict(); d["averageTraversal"] = np.float32(a.value); d["averageTests"] = np.float32(b.value)
        return d

    @property
    def spp(self):
        return self.L.crt_host_renderer_spp(self.h)

    @property
    def energy(self):
        return float(self.L.crt_host_renderer_energy(self.h))

    def accumulator(self):
        p = self.L.crt_host_renderer_accumulator(self.h)
        return np.ctypeslib.as_array(p, shape=(self.H, self.W, 4)).copy()

    def screen(self):
        p = self.L.crt_host_renderer_screen(self.h)
        return np.ctypeslib.as_array(p, shape=(self.H, self.W)).copy()

    def context(self):
        return Context.borrow(self.L.crt_host_renderer_ctx(self.h), self.W, self.H)


def load_obj(path):
    L = lib()
    n = C.c_uint32()
    pp, pn, pu = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
    rc = L.crt_host_obj_load(path.encode(), C.byref(n), C.byref(pp), C.byref(pn), C.byref(pu))
    if rc != 0:
        raise CrtError(rc, L.crt_host_last_error().decode())
    pos = np.ctypeslib.as_array(pp, shape=(n.value, 3)).copy()
    nrm = np.ctypeslib.as_array(pn, shape=(n.value, 3)).copy()
    uv = np.ctypeslib.as_array(pu, shape=(n.value, 2)).copy()
    for q in (pp, pn, pu):
        L.crt_host_free(C.cast(q, C.c_void_p))
    return pos, nrm, uv


def load_image(path):
    L = lib()
    w, h = C.c_int(), C.c_int()
    px = C.POINTER(C.c_uint32)()
    rc = L.crt_host_image_load(path.encode(), C.byref(w), C.byref(h), C.byref(px))
    if rc != 0:
        raise CrtError(rc, L.crt_host_last_error().decode())
    a = np.ctypeslib.as_array(px, shape=(h.value, w.value)).copy()
    L.crt_host_free(C.cast(px, C.c_void_p))
    return a


# ------------------------------------------------------------------------------------------------------------
# multi-GPU work split (one process per GPU, torch.distributed over RCCL) — pure arithmetic, shared by bench.py and tests
# ------------------------------------------------------------------------------------------------------------
def host_math_probe(inputs):
    """test entry: the host front's tmplmath.h restatements (csrc/host/hmath.h), layout of the real-reference harness's ref_math_probe (tests/golden/make_golden.py)"""
    inputs = np.ascontiguousarray(inputs, np.float32).reshape(-1, 12)
    out = np.zeros((len(inputs), 120), np.float32)
    lib().crt_host_math_probe(inputs.ctypes.data_as(C.c_void_p), C.c_uint32(len(inputs)), out.ctypes.data_as(C.c_void_p))
    return out


def host_grid_build(positions):
    """test / tool entry: the host front's Grid::Build (csrc/host/accel_alt.cpp) over bare positions ((n, 3, 3) float32), in HostScene.build_alt's layout"""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 9)
    L = lib()
    res = np.zeros(3, np.int32); f = np.zeros(9, np.float32); refs = C.c_uint32()

    def ck(rc):
        if rc != 0:
            raise CrtError(rc, L.crt_host_last_error().decode())
    ck(L.crt_host_grid_build(_p(pos), C.c_uint32(len(pos)), _p(res), _p(f), C.byref(refs), None, None))
    start = np.zeros(int(res.prod()) + 1, np.uint32); r = np.zeros(max(refs.value, 1), np.int32)
    ck(L.crt_host_grid_build(_p(pos), C.c_uint32(len(pos)), None, None, None, _p(start), _p(r)))
    return dict(resolution=res, cellSize=f[0:3].copy(), boundsMin=f[3:6].copy(), boundsMax=f[6:9].copy(), cellStart=start, refs=r[:refs.value])


def host_bvh_build(positions):
    """test / tool entry: the host front's BVH::Build (csrc/host/accel.cpp BuildSAH) over bare positions ((n, 3, 3) float32), in Context.get_bvh's layout"""
    L = lib()
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 9)
    info = (C.c_uint32 * 3)()
    nodes = np.zeros(2 * len(pos) - 1, NODE_DTYPE); idx = np.zeros(len(pos), np.uint32)
    rc = L.crt_host_bvh_build(_p(pos), C.c_uint32(len(pos)), info, _p(nodes), _p(idx))
    if rc != 0:
        raise RuntimeError("crt_host_bvh_build: %s" % L.crt_host_last_error().decode())
    return dict(nodes=nodes[:info[0]].copy(), indices=idx, nodesUsed=int(info[0]), maxDepth=int(info[1]), height=int(info[2]))


def host_kd_build(positions):
    """test / tool entry: the host front's KDTree::Build (csrc/host/accel_alt.cpp) over bare positions ((n, 3, 3) float32), in HostScene.build_alt's layout"""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 9)
    L = lib()
    info = (C.c_uint32 * 4)()

    def ck(rc):
        if rc != 0:
            raise CrtError(rc, L.crt_host_last_error().decode())
    ck(L.crt_host_kd_build(_p(pos), C.c_uint32(len(pos)), info, None, None))
    nodes = np.zeros(info[0], KD_NODE_DTYPE); r = np.zeros(max(info[1], 1), np.uint32)
    ck(L.crt_host_kd_build(_p(pos), C.c_uint32(len(pos)), None, _p(nodes), _p(r)))
    return dict(nodes=nodes, refs=r[:info[1]], maxDepth=int(info[2]), nodesUsed=int(info[3]))


def host_vertex_dedup(v8):
    """test entry: the host front's unique-vertex table (csrc/host/accel.cpp Dedup): (corner indices, unique vertices)"""
    v8 = np.ascontiguousarray(v8, np.float32).reshape(-1, 8)
    idx = np.zeros(len(v8), np.uint32); uniq = np.zeros((len(v8), 8), np.float32)
    L = lib(); L.crt_host_vertex_dedup.restype = C.c_uint32
    n = L.crt_host_vertex_dedup(v8.ctypes.data_as(C.c_void_p), C.c_uint32(len(v8)), idx.ctypes.data_as(C.c_void_p), uniq.ctypes.data_as(C.c_void_p))
    return idx, uniq[:n].copy()


def spp_window(rank, frames_per_rank, first_spp=1):
    """Weak scaling: rank r renders frames whose spp counter runs first_spp + r*F .. first_spp + (r+1)*F - 1.
    (tile, frame) streams are independent (renderer.cpp:120), so windows can be rendered anywhere and summed."""
    return first_spp + rank * frames_per_rank


def tile_partition(rank, world, n_tiles):
    """Strong scaling: rank r owns tiles r, r + world, r + 2*world, ... (interleaved: heavy image regions are shared out).
    Returns (tileFirst, tileStride, tileCount) for crt_config.  Each pixel is non-zero on exactly one rank, so a sum
    all-reduce of the accumulators reproduces the single-GPU image exactly."""
    count = (n_tiles - rank + world - 1) // world if rank < n_tiles else 0
    return rank, world, count


TILE_NO_LIGHT, TILE_NO_FLOOR, TILE_NO_TREE = 1, 2, 4      # layout.h kTileNo*: tests no primary ray of a tile can pass
TILE_SKY = 7
TILE_FLOOR_SURE = 8                                       # layout.h kTileFloorSure: the floor plane's test EVERY primary ray of a tile passes (the _ex entries only)
TILE_FLOOR = TILE_NO_LIGHT | TILE_NO_TREE | TILE_FLOOR_SURE


def tile_classes_host(camera, light_offsets, light_size, floor_d, root_pair, width, height, tile_first=0, tile_stride=1, tile_count=-1, flags=7, ex=False):
    """crt_debug_tile_classes_host (no GPU): the tile classes of a bare Scene block.  camera = camPos, topLeft, topRight, bottomLeft (12 floats); light_offsets =
    lightInvT[3], [7], [11]; root_pair = the root's NodePair (16 floats); flags: 1 lightAxis, 2 floorAxisY, 4 rootIsPair.  ex: crt_debug_tile_classes_host_ex, the
    whole byte (TILE_FLOOR_SURE as well)."""
    if tile_count < 0:
        tile_first, tile_stride, tile_count = 0, 1, (width // 16) * (height // 16)
    v = np.concatenate([np.asarray(camera, np.float32).reshape(12), np.asarray(light_offsets, np.float32).reshape(3), np.array([light_size, floor_d], np.float32),
                        np.asarray(root_pair, np.float32).reshape(16)]).astype(np.float32)
    out = np.zeros(tile_count, np.uint8)
    L = lib()
    f = L.crt_debug_tile_classes_host_ex if ex else L.crt_debug_tile_classes_host
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    rc = f(_p(v), flags, width, height, tile_first, tile_stride, tile_count, _p(out))
    if rc != 0:
        raise CrtError(rc, "crt_debug_tile_classes_host: invalid argument")
    return out


def reduce_accumulator(tensor, dist, dst=0):
    """ncclReduce of the float4 accumulators to one rank: only rank `dst` ends up with the whole image.  With tile ownership
    every pixel is non-zero on exactly one rank, so the sum is exact (x + 0 ...)."""
    dist.reduce(tensor, dst=dst, op=dist.ReduceOp.SUM)
    return tensor


def allreduce_accumulator(tensor, dist):
    """One collective per step: sum of the float4 accumulators over all ranks (RCCL over xGMI on GPUs, gloo in CPU tests)."""
    dist.all_reduce(tensor, op=dist.ReduceOp.SUM)
    return tensor
