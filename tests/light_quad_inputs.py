"""Rays for a turned or resized light quad (a look of crt_update_look / crt_render_looks), generated with a fixed seed, for tests/test_mesh_truth_cpu.py (the
oracle meets the truth on them, and they meet the truth's caps) and tests/test_gpu_light_quad.py (the kernels).  The quads are render_looks_inputs.quad_looks'.
Not collected by pytest.

The quad of a world (mesh_truth.World) is the square |x|, |z| < half of the frame (R | c): a point (x, z) of its plane is c + x R[:, 0] + z R[:, 2], its normal
R[:, 1].  Classes of make_rays (every origin but the shadow rays' at least 0.2 above the floor):
  edge      aimed at (+-(half -+ d), z) and (x, +-(half -+ d)), |x|, |z| < 0.9 half: just inside and just outside each of the four edges, from both faces.
            d = max(half * 2^-10, 3 * mesh_truth.EPS): the truth's own band round the half size is EPS = 1e-4, and a ray nearer the edge than that says nothing
            (it is "uninformative": either answer is right).  For half = 0.03125 that is 3e-4, a hundredth of the quad, where half * 2^-10 = 3e-5 lies inside
            the band; RAW_EDGE rays are aimed at half * (1 -+ 2^-10) all the same, and are held to the oracle bit for bit like every other ray.
  corner    the same d inside both edges at each corner, and outside one of them
  inside    the interior, from both faces
  graze     through interior points at 0.5 degrees to the plane
  through   through an interior point and a mesh triangle's centroid, the triangle met at a cosine of 0.2 or more: from beyond the quad (the quad first, the mesh
            behind it) and from beyond the mesh
  shadow    from floor points and from beside mesh centroids towards interior points, with a length that ends 1e-3 of the way short of the quad or beyond it
  miss      upwards through the quad's plane outside the square: the sky, unless a mesh is in the way
exact_rays: for the two quads whose cells are exactly 0 / +-1, rays exactly parallel to the plane and origins exactly in it (t = x / -0, 0 / D, 0 / -0).
axis_form: what Quad::Intersect's expressions come to on those two quads, a float32 one-liner on permuted coordinates that needs no oracle."""
import numpy as np

import mesh_truth as mt
import render_looks_inputs as li

F = np.float32
CLASSES = ("edge", "corner", "inside", "graze", "through", "shadow", "miss")
SHARES = (0.20, 0.06, 0.14, 0.08, 0.20, 0.14, 0.18)
RAW_EDGE = 8                                       # one per edge and side of it
N_RAYS = {"cube": 2048, "tlas": 1024}              # (the truth of 1 024 rays over tlas_scene.xml's 12 460 triangles takes 3 s of numpy)
# mesh_truth.MIN_MESH asks for 500 robust mesh hits of rays made to hit meshes; these are made for the quad, and a mesh is what some of them meet before or
# behind it (the `through` and `shadow` classes).  MAX_UNINFORMATIVE, MIN_PRIM and MIN_MISS hold as they are.
MIN_MESH = 40
MIN_ORDER = 20                                     # ... and of each order of quad and mesh (Case.order) at least this many
FLOOR_CLEAR = -0.8


def edge_offset(half):
    return max(half * 2.0 ** -10, 3 * mt.EPS)


def plane_point(world, x, z):
    return world.light + np.asarray(x)[:, None] * world.light_R[:, 0] + np.asarray(z)[:, None] * world.light_R[:, 2]


def _towards(world, rng, target, side, lo=0.4, hi=2.5, cos_min=0.25):
    """origins on the `side` (+-1 per ray) of the quad's plane from which a ray reaches `target` at a cosine of at least cos_min, clear of the floor"""
    k = len(target); n = world.light_R[:, 1]
    tang = rng.normal(size=(k, 3)); tang -= (tang @ n)[:, None] * n; tang = mt._unit(tang)
    a = rng.uniform(cos_min, 1.0, k)
    v = (side * a)[:, None] * n + np.sqrt(1 - a * a)[:, None] * tang
    dist = rng.uniform(lo, hi, k)
    room = np.where(v[:, 1] < 0, (target[:, 1] - FLOOR_CLEAR) / np.maximum(-v[:, 1], 1e-9), np.inf)
    dist = np.minimum(dist, 0.9 * room)
    assert (dist > 0.05).all()
    O = target + dist[:, None] * v
    return O, target - O


def make_rays(world, n, seed):
    """(O, D float32 [n, 3], t float32 [n]: a shadow length for the `shadow` class and NaN elsewhere, class [n])"""
    rng = np.random.default_rng(seed)
    h = world.light_half; d = edge_offset(h)
    counts = [int(round(s * n)) for s in SHARES]; counts[0] += n - sum(counts)
    wv = np.concatenate(world.world_v).reshape(-1, 3, 3); cen = wv.mean(1)
    Os, Ds, Ts = [], [], []

    def add(O, D, t=None):
        Os.append(O); Ds.append(D); Ts.append(np.full(len(O), np.nan) if t is None else t)

    # edge
    k = counts[0]
    off = np.full(k, d); off[:RAW_EDGE] = h * 2.0 ** -10
    along = rng.uniform(-0.9 * h, 0.9 * h, k)
    sign = np.where(np.arange(k) % 2 == 0, 1.0, -1.0)                       # which of the two opposite edges
    inout = np.where((np.arange(k) // 2) % 2 == 0, -1.0, 1.0)                # inside / outside
    axis = (np.arange(k) // 4) % 2                                          # the x edges / the z edges
    e = sign * (h + inout * off)
    x, z = np.where(axis == 0, e, along), np.where(axis == 0, along, e)
    add(*_towards(world, rng, plane_point(world, x, z), np.where((np.arange(k) // 8) % 2 == 0, 1.0, -1.0)))
    # corner
    k = counts[1]
    sx, sz = np.where(np.arange(k) % 2 == 0, 1.0, -1.0), np.where((np.arange(k) // 2) % 2 == 0, 1.0, -1.0)
    out = (np.arange(k) // 4) % 2                                           # 0: inside both edges, 1: outside the x edge
    add(*_towards(world, rng, plane_point(world, sx * (h + np.where(out == 1, d, -d)), sz * (h - d)), np.where((np.arange(k) // 8) % 2 == 0, 1.0, -1.0)))
    # inside
    k = counts[2]
    add(*_towards(world, rng, plane_point(world, rng.uniform(-0.9 * h, 0.9 * h, k), rng.uniform(-0.9 * h, 0.9 * h, k)), np.where(np.arange(k) % 2 == 0, 1.0, -1.0), cos_min=0.1))
    # graze: 0.5 degrees off the plane
    k = counts[3]
    q = plane_point(world, rng.uniform(-0.8 * h, 0.8 * h, k), rng.uniform(-0.8 * h, 0.8 * h, k))
    ang = rng.uniform(0, 2 * np.pi, k)
    inpl = np.cos(ang)[:, None] * world.light_R[:, 0] + np.sin(ang)[:, None] * world.light_R[:, 2]
    side = np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
    v = np.cos(np.radians(0.5)) * inpl + (side * np.sin(np.radians(0.5)))[:, None] * world.light_R[:, 1]
    v = np.where((v[:, 1] < -0.5)[:, None], v - 2 * (v * inpl).sum(1)[:, None] * inpl, v)        # (a steeply descending one is mirrored: upwards)
    dist = rng.uniform(0.3, 1.0, k)
    room = np.where(v[:, 1] < 0, (q[:, 1] - FLOOR_CLEAR) / np.maximum(-v[:, 1], 1e-9), np.inf)
    O = q + np.minimum(dist, 0.9 * room)[:, None] * v
    add(O, q - O)
    # through the quad and a mesh
    k = counts[4]
    pick = rng.integers(0, len(cen), 8 * k)
    q = plane_point(world, rng.uniform(-0.8 * h, 0.8 * h, 8 * k), rng.uniform(-0.8 * h, 0.8 * h, 8 * k))
    u = mt._unit(q - cen[pick])
    ng = mt._unit(mt._cross(wv[pick, 1] - wv[pick, 0], wv[pick, 2] - wv[pick, 0]))
    keep = np.flatnonzero(np.abs((ng * u).sum(1)) >= 0.2)[:k]               # (t through a triangle met at a shallow angle loses digits no tolerance of the truth sees)
    assert len(keep) == k
    g, q, u = cen[pick[keep]], q[keep], u[keep]
    beyond_quad = q + rng.uniform(0.3, 1.0, k)[:, None] * u
    back = np.minimum(rng.uniform(0.5, 1.5, k), 0.9 * (g[:, 1] - FLOOR_CLEAR) / np.maximum(u[:, 1], 1e-9))     # (as far back as the floor leaves room for)
    beyond_mesh = g - np.maximum(back, 0.0)[:, None] * u
    from_mesh = (np.arange(k) % 2 == 1) & (back > 0.05)
    O = np.where(from_mesh[:, None], beyond_mesh, beyond_quad)
    assert (O[:, 1] > FLOOR_CLEAR).all()
    add(O, np.where(from_mesh[:, None], u, -u))
    # shadow
    k = counts[5]
    q = plane_point(world, rng.uniform(-0.8 * h, 0.8 * h, k), rng.uniform(-0.8 * h, 0.8 * h, k))
    fl = np.stack([world.light[0] + rng.uniform(-2, 2, k), np.full(k, -1.0 + 1e-3), world.light[2] + rng.uniform(-2, 2, k)], 1)
    gm = cen[rng.integers(0, len(cen), k)]
    P = np.where((np.arange(k) % 2 == 0)[:, None], fl, gm + 0.02 * mt._unit(q - gm))
    dist = np.linalg.norm(q - P, axis=1)
    add(P, q - P, dist * np.where((np.arange(k) // 2) % 2 == 0, 1 - 1e-3, 1 + 1e-3))
    # miss
    k = counts[6]
    r = rng.uniform(1.3 * h + 0.05, 3 * h + 0.3, k); ang = rng.uniform(0, 2 * np.pi, k)
    lx, lz = r * np.cos(ang), r * np.sin(ang)
    big = np.maximum(np.abs(lx), np.abs(lz)) < 1.3 * h + 0.05                # (a point of the ring that is still over the square: pushed out along x)
    lx = np.where(big, np.where(lx < 0, -1.0, 1.0) * (1.3 * h + 0.05), lx)
    tp = plane_point(world, lx, lz)
    v = mt._unit(rng.normal(size=(k, 3))); v[:, 1] = np.abs(v[:, 1]) * 0.7 + 0.3; v = mt._unit(v)
    dn = v @ world.light_R[:, 1]
    v = np.where((np.abs(dn) < 0.1)[:, None], mt._unit(v + 0.3 * np.where(dn < 0, -1.0, 1.0)[:, None] * world.light_R[:, 1]), v)
    dist = np.minimum(rng.uniform(0.3, 2.0, k), 0.9 * (tp[:, 1] - FLOOR_CLEAR) / v[:, 1])
    add(tp - dist[:, None] * v, v)
    O, D = mt._as_rays(np.concatenate(Os), np.concatenate(Ds))
    cls = np.repeat(np.arange(len(CLASSES)), counts)
    assert (O[cls != CLASSES.index("shadow"), 1] > FLOOR_CLEAR - 1e-3).all()
    return O, D, np.concatenate(Ts).astype(F), cls


def shadow_lengths(t_given, tr, seed):
    """the shadow class's own lengths, mesh_truth.shadow_lengths for the rest"""
    return np.where(np.isnan(t_given), mt.shadow_lengths(tr, seed), t_given).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the two quads of exact cells
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def normal_axis(T):
    """the world axis the plane's normal lies along, for a T whose rotation cells are exactly 0 / +-1"""
    col = np.asarray(T, F).reshape(4, 4)[:3, 1]
    assert sorted(np.abs(col).tolist()) == [0.0, 0.0, 1.0]
    return int(np.flatnonzero(col)[0])


def exact_rays(T, half, seed, n=64):
    """rays no truth in float64 judges (their t is a division by zero, or zero): n exactly parallel to the plane (a quarter of them starting IN it: 0 / -0), and n
    starting exactly in the plane, over the square and beside it.  Quad::Intersect answers none of them with the light (t > 0 fails, or t < ray.t does)."""
    rng = np.random.default_rng(seed)
    T = np.asarray(T, F).reshape(4, 4); a = normal_axis(T); c = T[:3, 3]
    other = [i for i in range(3) if i != a]
    O = np.zeros((2 * n, 3), F); D = mt._unit(rng.normal(size=(2 * n, 3))).astype(F)
    O[:, other] = c[other] + rng.uniform(-2 * half, 2 * half, (2 * n, 2)).astype(F)
    O[:n, a] = c[a] + np.where(np.arange(n) % 4 == 0, 0.0, rng.uniform(-0.5, 0.5, n)).astype(F)
    D[:n, a] = np.where(np.arange(n) % 2 == 0, F(0.0), -F(0.0))             # both zeros
    O[n:, a] = c[a]
    assert (D[:n, a] == 0).all() and (D[n:, a] != 0).all() and (O[n:, a] == c[a]).all()
    return O, D


def axis_form(name, T, half, O, D):
    """(the quad is a candidate, its t) per ray as float32 arithmetic gives them: Quad::Intersect's sums with the exact cells of quarter_z (invT rows (0, -1, 0, py),
    (1, 0, 0, -px), (0, 0, 1, -pz)) and half_x (rows (1, 0, 0, -px), (0, -1, 0, py), (0, 0, -1, pz)) written out: a product with 0 adds nothing, one with +-1 is
    the coordinate.  The ray's own t limit (1e34) is applied; a nearer mesh or floor is the caller's."""
    O, D = np.asarray(O, F), np.asarray(D, F); px, py, pz = np.asarray(T, F).reshape(4, 4)[:3, 3]; h = F(half)
    with np.errstate(all="ignore"):
        if name == "quarter_z":
            t = ((O[:, 0] - px).astype(F) / -D[:, 0]).astype(F)
            ix = ((py - O[:, 1]).astype(F) + (t * -D[:, 1]).astype(F)).astype(F)
            iz = ((O[:, 2] - pz).astype(F) + (t * D[:, 2]).astype(F)).astype(F)
        elif name == "half_x":
            t = ((py - O[:, 1]).astype(F) / D[:, 1]).astype(F)
            ix = ((O[:, 0] - px).astype(F) + (t * D[:, 0]).astype(F)).astype(F)
            iz = ((pz - O[:, 2]).astype(F) + (t * -D[:, 2]).astype(F)).astype(F)
        else:
            raise ValueError(name)
        hit = (t < F(1e34)) & (t > 0) & (ix > -h) & (ix < h) & (iz > -h) & (iz < h)
    return hit, t


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# a look's rays and their truth
# ---------------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """scene `scene` ('cube' / 'tlas' of render_looks_inputs) under the quad look `look`: its world from the arrays of `source` (anything that answers bvh_count(),
    bvh(i) and blas_transform(i): the oracle's scene on the CPU, the library's host scene on the GPU), the rays and their truth; computed once, never written to"""

    def __init__(self, orc, scene, name, look, source, seed=7):
        import mesh_truth_scenes as MC
        from conftest import scene_path
        xml, self.kind = li.SCENES[scene]
        self.scene, self.name, self.look = scene, name, look
        self.sc, light, obj_mat, invto = MC.describe(orc, scene_path(xml))
        self.world = mt.world_of(source, self.kind, light, obj_mat, invto, light_T=np.asarray(look["light_T"], F).reshape(4, 4), light_half=look["light_size"])
        self.O, self.D, given, self.cls = make_rays(self.world, N_RAYS[scene], seed)
        self.tr = mt.nearest_truth(self.world, self.O, self.D)
        self.ti = mt.hit_info_truth(self.world, self.O, self.D, self.tr)
        self.ts = shadow_lengths(given, self.tr, 3)
        self.occ = mt.occluded_truth(self.world, self.O, self.D, self.ts, self.tr)
        self.caps = mt.check_caps(self.tr, "%s under %s" % (scene, name), min_mesh=MIN_MESH)
        # the order of quad and mesh is judged on enough rays of each kind: a mesh robustly first in the `through` and in the `shadow` class, and the quad
        # robustly first with a mesh candidate behind it
        mesh_first = self.tr["kind_hi"] == 2
        self.order = dict(through=int((mesh_first & (self.cls == CLASSES.index("through"))).sum()), shadow=int((mesh_first & (self.cls == CLASSES.index("shadow"))).sum()),
                          quad_first=int(((self.tr["kind_hi"] == 0) & np.isfinite(self.tr["mesh_hi"])).sum()))
        assert min(self.order.values()) >= MIN_ORDER, (scene, name, self.order)
        for a in (self.O, self.D, self.ts):
            a.setflags(write=False)

    def light_faces(self):
        """how many robust light hits come from the side the normal points to, and from the other"""
        m = self.tr["kind_hi"] == 0
        s = (self.D[m].astype(np.float64) @ self.world.light_R[:, 1]) > 0
        return int(s.sum()), int((~s).sum())
