"""Closed-form ground truth for Renderer::Sample, ProcessTile, the Whitted integrator and the PrimitiveScene, in float64 numpy.

Every other render test holds a kernel to oracle/crt_oracle.cpp bit for bit; kernel and oracle are two restatements of the same reading of the reference.  What is
here is derived from the reference's lines a third time, as mathematics: the EXPECTATION of the reference's estimator on scenes small enough to have one, and the
analytic nearest hit of the PrimitiveScene's primitives.  Nothing in this module imports the oracle or the library; the test modules hand their results in.

Statistical criterion of every comparison with a mean of N samples:   |mean - want| <= Z * sigma_truth / sqrt(N),   Z = 5,
with sigma_truth from the SECOND MOMENT OF THE TRUTH (never from the samples).  The two test modules make some 50 distinct comparisons of this kind on the scenes
as their files give them, and some 100 more under the quad looks below (QUAD_LOOKS: 5 looks x 5 floor points through the BVH — the TLAS returns the same samples —
and 5 looks x 8 floor tiles x 3 channels share one render per look, counted once per tile: 25 + 40, and the render_looks job's 40 again); the kernels return the
oracle's bits, so theirs are the same numbers again.  A correct estimator fails one of 150 three-channel comparisons with probability < 450 * 5.8e-7 = 2.7e-4, and the
seeds are fixed, so what passes once passes always.

THE QUAD.  quad = (centre, half) is the scene files' quad, parallel to the floor; quad = (centre, R, half) a look's (crt_update_look): the square |x|, |z| < half of
the frame whose axes are R's columns, R[:, 1] its normal's axis.  It emits (24, 24, 22) from BOTH faces (the path tracer returns the light's colour before it
looks at a normal, renderer.cpp:69), so every integral takes |cos theta'|; the Whitted point light is the centre moved 0.01 down in WORLD y whatever R is
(file_scene.cpp:156-162: the two corners' mean, minus (0, 0.01, 0)), and its N.L is the floor's normal alone.  Every test quad lies wholly above the floor, which
the contour formula needs and floor_radiance asserts.

Line numbers: renderer.cpp = "3. PathTracer/renderer.cpp" unless "2. WhittedStyle" is named; the other files are template/ and infra/ of the reference.
"""
import numpy as np

Z = 5.0
EPSILON = 1e-3                                     # renderer.h:12
LIGHT = np.array([24.0, 24.0, 22.0])               # file_scene.cpp:164-167
FLOOR_Y = -1.0                                     # file_scene.cpp:16: Plane(1, (0, 1, 0), 1): y = -1
LIGHT_HALF = 0.5                                   # file_scene.cpp:15: Quad(0, 1); primitives.h:328
N1, N2 = 1.0, float(np.float32(1.2))               # renderer.cpp:31
R0 = ((N1 - N2) / (N1 + N2)) ** 2                  # renderer.cpp:37; the same from either side


def texel_rgb(rgb8):
    """Texture::Sample's colour of an 8-bit texel (texture.h:90-93): c * (1 / 255.0f) in float32"""
    return (np.asarray(rgb8, np.float32) * np.float32(1.0 / 255.0)).astype(np.float64)


def z_ok(mean, want, second_moment, n):
    """the criterion above, per channel; returns (ok, z scores)"""
    mean, want, second_moment = np.asarray(mean, np.float64), np.asarray(want, np.float64), np.asarray(second_moment, np.float64)
    sigma = np.sqrt(np.maximum(second_moment - want * want, 0.0))
    tol = Z * sigma / np.sqrt(n)
    z = (mean - want) / np.maximum(sigma / np.sqrt(n), 1e-300)
    return bool((np.abs(mean - want) <= tol).all()), z


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the floor under a constant sky and the light quad
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _corner(x, z, h):
    a, b = np.sqrt(x * x + h * h), np.sqrt(z * z + h * h)
    return (x / a * np.arctan(z / a) + z / b * np.arctan(x / b)) / (2.0 * np.pi)


def _quad_edges(P, quad):
    P = np.asarray(P, np.float64); c, s = np.asarray(quad[0], np.float64), float(quad[1])
    return c[0] - s - P[..., 0], c[0] + s - P[..., 0], c[2] - s - P[..., 2], c[2] + s - P[..., 2], c[1] - P[..., 1]


def quad_frame(quad):
    """(centre, R [3, 3], half) of either form of a quad"""
    if len(quad) == 2:
        return np.asarray(quad[0], np.float64), np.eye(3), float(quad[1])
    return np.asarray(quad[0], np.float64), np.asarray(quad[1], np.float64).reshape(3, 3), float(quad[2])


def quad_corners(quad):
    c, R, h = quad_frame(quad)
    return np.stack([c + sx * h * R[:, 0] + sz * h * R[:, 2] for sx, sz in ((-1, -1), (1, -1), (1, 1), (-1, 1))])


def form_factor_polygon(P, n, corners):
    """Lambert's contour formula: the form factor from a differential area at P [..., 3] with normal n to the polygon `corners` [k, 3], all of it above P's horizon:
    1 / 2 pi * sum gamma_i n . (r_i x r_i+1) / |r_i x r_i+1|, gamma_i the angle the edge subtends.  The sign of the sum is the polygon's winding; a quad that emits
    from both faces counts either way: the absolute value."""
    P, n, corners = np.asarray(P, np.float64), np.asarray(n, np.float64), np.asarray(corners, np.float64)
    r = corners - P[..., None, :]
    assert ((r @ n) > 0).all(), "a corner at or below the horizon"
    r = r / np.linalg.norm(r, axis=-1, keepdims=True)
    rn = np.roll(r, -1, axis=-2)
    cr = np.cross(r, rn); sn = np.linalg.norm(cr, axis=-1)
    gamma = np.arctan2(sn, (r * rn).sum(-1))
    return np.abs((gamma * (cr @ n) / sn).sum(-1)) / (2.0 * np.pi)


def form_factor(P, quad):
    """form factor from a horizontal differential area at P [..., 3] (normal +y) to the quad above it.  quad = (centre, half size), parallel: the corner term
    x / sqrt(x^2 + h^2) atan(z / sqrt(x^2 + h^2)) + z / sqrt(z^2 + h^2) atan(x / sqrt(z^2 + h^2)) over 2 pi, summed with signs over the four corners;
    quad = (centre, R, half): form_factor_polygon"""
    if len(quad) == 3:
        return form_factor_polygon(P, [0.0, 1.0, 0.0], quad_corners(quad))
    x1, x2, z1, z2, h = _quad_edges(P, quad)
    return _corner(x2, z2, h) - _corner(x1, z2, h) - _corner(x2, z1, h) + _corner(x1, z1, h)


_GL = np.polynomial.legendre.leggauss(12)


def cos2_solid_angle(P, quad):
    """integral of cos^2(theta) d omega over the quad seen from P (theta from +y), by 12 x 12 Gauss-Legendre over the quad's own parametrisation:
    d omega = |cos theta'| dA / r^2, so the integrand is (d.y)^2 |d . n'| / r^5 with d the vector to the quad's point and n' = R[:, 1]"""
    P = np.asarray(P, np.float64)
    c, R, h = quad_frame(quad)
    g, w = _GL
    pts = c + h * g[:, None, None] * R[:, 0] + h * g[None, :, None] * R[:, 2]
    d = pts - P[..., None, None, :]
    r2 = (d * d).sum(-1)
    f = d[..., 1] ** 2 * np.abs(d @ R[:, 1]) / r2 ** 2.5
    return (f * w[:, None] * w[None, :]).sum(axis=(-1, -2)) * h * h


def cos2_solid_angle_parallel(P, quad):
    """the same for quad = (centre, half), parallel to the floor: integral of h^3 / r^5 dA (what cos2_solid_angle must come to there)"""
    x1, x2, z1, z2, h = _quad_edges(P, quad)
    g, w = _GL
    x = (x1[..., None] + x2[..., None]) / 2 + (x2 - x1)[..., None] / 2 * g
    z = (z1[..., None] + z2[..., None]) / 2 + (z2 - z1)[..., None] / 2 * g
    r2 = x[..., :, None] ** 2 + z[..., None, :] ** 2 + (h * h)[..., None, None]
    f = (h ** 3)[..., None, None] / r2 ** 2.5
    return (f * w[:, None] * w[None, :]).sum(axis=(-1, -2)) * (x2 - x1) * (z2 - z1) / 4


def form_factor_quadrature(P, quad, n=400):
    """brute force: cos(theta) |cos(theta')| / (pi r^2) over an n x n midpoint grid of the quad (the check of form_factor)"""
    if len(quad) == 3:
        c, R, h = quad_frame(quad)
        u = ((np.arange(n) + 0.5) / n * 2.0 - 1.0) * h
        d = c + u[:, None, None] * R[:, 0] + u[None, :, None] * R[:, 2] - np.asarray(P, np.float64)
        r2 = (d * d).sum(-1)
        return float((d[..., 1] * np.abs(d @ R[:, 1]) / (np.pi * r2 * r2)).sum() * (2.0 * h / n) ** 2)
    x1, x2, z1, z2, h = [float(v) for v in _quad_edges(np.asarray(P, np.float64), quad)]
    x = x1 + (np.arange(n) + 0.5) * (x2 - x1) / n; z = z1 + (np.arange(n) + 0.5) * (z2 - z1) / n
    r2 = x[:, None] ** 2 + z[None, :] ** 2 + h * h
    return float((h * h / (np.pi * r2 * r2)).sum() * (x2 - x1) * (z2 - z1) / (n * n))


def floor_radiance(P, rho, L_sky, quad, one_face=False):
    """(E[X], E[X^2]) [..., 3] of X = Sample(ray that hits the floor at P) when the bounce ray can meet only the light quad or the constant sky.
    renderer.cpp:95-98: R uniform on the hemisphere (tmplmath.h:535-544, pdf 1 / 2 pi), X = albedo * INVPI * 2 * PI * dot(R, N) * Sample(R), and
    Sample(R) = (24, 24, 22) on the quad (:69, both faces, file_scene.cpp:211) or the sky texel (:54).  So
        E[X]   = rho / pi * integral cos L_in d omega    = rho (L_sky (1 - F) + L_light F)
        E[X^2] = rho^2 (2 / pi) integral cos^2 L_in^2 d omega,  integral of cos^2 over the hemisphere = 2 pi / 3"""
    rho, L_sky = np.asarray(rho, np.float64), np.asarray(L_sky, np.float64)
    assert (quad_corners(quad)[:, 1] > FLOOR_Y).all(), "the quad reaches the floor"
    F = form_factor(P, quad)[..., None]; Q = cos2_solid_angle(P, quad)[..., None]
    if one_face:                                                           # a WRONG model, for the tests' controls: only the face the normal -R[:, 1] points from emits
        c, R, _ = quad_frame(quad)
        seen = (((np.asarray(P, np.float64) - c) @ -R[:, 1]) > 0)[..., None]
        F, Q = F * seen, Q * seen
    mean = rho * (L_sky * (1.0 - F) + LIGHT * F)
    second = rho * rho * (2.0 / np.pi) * (LIGHT * LIGHT * Q + L_sky * L_sky * (2.0 * np.pi / 3.0 - Q))
    return mean, second


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the dielectric slab at normal incidence
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _slab(albedo, absorption, thickness, L_sky, depth_limit, behind, reflected_keeps_flag, power):
    a = np.asarray(albedo, np.float64) ** power
    L = np.asarray(L_sky, np.float64) ** power
    m_inside = np.exp(-np.asarray(absorption, np.float64) * (thickness - EPSILON)) ** power     # the leg starts EPSILON past the last hit (:30, :40)
    zero = np.zeros(3)

    def leaves(depth, forward):
        # the ray has left the cube.  Backwards it misses everything: the sky, at any depth (:54 comes before :55).  Forwards the same, or a mirror whose
        # reflection misses everything: albedo * sky (:87, :20-25; the mirror absorbs nothing), and 0 if that hit is at the depth limit (:55)
        if not forward or behind is None:
            return L
        return zero if depth >= depth_limit else np.asarray(behind, np.float64) ** power * L

    def meets_face(depth, forward, within, flag):
        if depth >= depth_limit:
            return zero                                                    # :55, only on a hit
        m = m_inside if flag else 1.0                                      # :77-81: absorption at the hit that ends a leg whose ray says `inside`
        # :29-30 the reflected ray is built afresh: inside = false, wherever it is.  (The physical variant keeps the flag.)
        r_flag = flag if reflected_keeps_flag else False
        refl = meets_face(depth + 1, not forward, True, r_flag) if within else leaves(depth + 1, not forward)
        # :41 the transmitted ray flips the flag it was given
        trans = leaves(depth + 1, forward) if within else meets_face(depth + 1, forward, True, not flag)
        # :31-38 at cosi = 1: c = 0 and Fr = R0 whichever way n1, n2 are assigned; :42 transmits with probability 1 - Fr
        return a * m * (R0 * refl + (1.0 - R0) * trans)
    return meets_face(0, True, False, False)


def slab_radiance(albedo, absorption, thickness, L_sky, depth_limit, behind=None):
    """(E[X], E[X^2]) of Sample(ray at normal incidence on a dielectric cube, refractivity 1) under a constant sky.  `behind`: None = the ray that leaves the far
    face sees the sky as well; an albedo = it meets a mirror there whose reflection sees the sky (the floor is an infinite plane: one of the two ways out of a
    cube points down, and only another object keeps that ray off the diffuse floor).  The recursion and the reference lines it rests on are in _slab."""
    return (_slab(albedo, absorption, thickness, L_sky, depth_limit, behind, False, 1), _slab(albedo, absorption, thickness, L_sky, depth_limit, behind, False, 2))


def slab_radiance_physical(albedo, absorption, thickness, L_sky, depth_limit, behind=None):
    """the negative control: the textbook slab, in which an internally reflected ray is still inside and is absorbed on its next leg"""
    return (_slab(albedo, absorption, thickness, L_sky, depth_limit, behind, True, 1), _slab(albedo, absorption, thickness, L_sky, depth_limit, behind, True, 2))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# sky, mirror, transforms, boxes
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def sky_lookup(D, sky):
    """FileScene::GetSkyColor (file_scene.cpp:142-154) + Texture::Sample (texture.h:61-96) in float64 on sky = [h, w, 3] uint8, top row first.
    Returns (rgb [..., 3], texel coordinates x, y as reals: their distance to the next integer says how close the lookup is to a texel border)"""
    D = np.asarray(D, np.float64); D = D / np.linalg.norm(D, axis=-1, keepdims=True)
    h, w = sky.shape[:2]
    phi = np.arctan2(-D[..., 2], D[..., 0]) + np.pi
    theta = np.arccos(np.clip(-D[..., 1], -1.0, 1.0))
    u = np.clip(phi / (2.0 * np.pi), 0.0, 1.0); v = 1.0 - np.clip(theta / np.pi, 0.0, 1.0)
    x, y = u * w, v * h
    xi = np.clip(x.astype(np.int64), 0, w - 1); yi = np.clip(y.astype(np.int64), 0, h - 1)
    return texel_rgb(sky[yi, xi, :3]), x, y


def border_distance(x, y):
    return np.minimum(np.minimum(x - np.floor(x), np.ceil(x) - x), np.minimum(y - np.floor(y), np.ceil(y) - y))


def mirror_radiance(D, N, albedo, sky):
    """Sample of a ray that meets a mirror (reflectivity 1) with normal N whose reflection misses everything: albedo * sky(reflect(D, N))
    (renderer.cpp:20-25, :87; reflect = D - 2 dot(D, N) N).  Returns (rgb, texel x, texel y)"""
    D, N = np.asarray(D, np.float64), np.asarray(N, np.float64)
    R = D - 2.0 * (D * N).sum(-1, keepdims=True) * N
    rgb, x, y = sky_lookup(R, sky)
    return np.asarray(albedo, np.float64) * rgb, x, y


def euler_rotation(deg):
    """RotateX * RotateY * RotateZ of file_scene.cpp:45-48 (degrees), matrices as tmplmath.h:673-675"""
    ax, ay, az = np.deg2rad(np.asarray(deg, np.float64))
    c, s = np.cos, np.sin
    X = np.array([[1, 0, 0], [0, c(ax), -s(ax)], [0, s(ax), c(ax)]])
    Y = np.array([[c(ay), 0, s(ay)], [0, 1, 0], [-s(ay), 0, c(ay)]])
    Zm = np.array([[c(az), -s(az), 0], [s(az), c(az), 0], [0, 0, 1]])
    return X @ Y @ Zm


class Box:
    """cube.obj (corners +-1) under Translate(position) * rotation * Scale(scale): an oriented box"""

    def __init__(self, position, rotation, scale):
        self.c = np.asarray(position, np.float64); self.R = euler_rotation(rotation); self.half = np.asarray(scale, np.float64) * np.ones(3)

    def corners(self):
        s = np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], np.float64)
        return self.c + (s * self.half) @ self.R.T

    def intersect(self, O, D):
        """(t_enter, t_exit, axis of the entered face, sign of its outward normal on that axis) per ray; t_enter > t_exit: no hit"""
        O, D = np.asarray(O, np.float64), np.asarray(D, np.float64)
        o = (O - self.c) @ self.R; d = D @ self.R
        with np.errstate(divide="ignore", invalid="ignore"):
            t1 = (-self.half - o) / d; t2 = (self.half - o) / d
        lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
        axis = lo.argmax(-1)
        sign = -np.sign(np.take_along_axis(d, axis[..., None], -1)[..., 0])
        return lo.max(-1), hi.min(-1), axis, sign

    def blocks(self, O, D, tmax):
        """does the segment O + t D, 0 < t < tmax meet the box"""
        t0, t1, _, _ = self.intersect(O, D)
        return (t0 <= t1) & (t1 > 0) & (t0 < tmax)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# camera, pixels
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def camera_default(W, H):
    """Camera() (camera.h:14-22) with aspect = W / H: (camPos, topLeft, topRight, bottomLeft)"""
    a = W / H
    return np.array([0.0, 0.0, -2.0]), np.array([-a, 1.0, 0.0]), np.array([a, 1.0, 0.0]), np.array([-a, -1.0, 0.0])


def camera_state(position, target, W, H):
    """Camera::SetCameraState (camera.h:61-73)"""
    def nrm(v):
        return v / np.linalg.norm(v)
    p, t = np.asarray(position, np.float64), np.asarray(target, np.float64); a = W / H
    ahead = nrm(t - p); right = nrm(np.cross([0.0, 1.0, 0.0], ahead)); up = nrm(np.cross(ahead, right)); right = nrm(np.cross(up, ahead))
    return p, p + 2 * ahead - a * right + up, p + 2 * ahead + a * right + up, p + 2 * ahead - a * right - up


def primary_dirs(camera, W, H, x, y):
    """Camera::GetPrimaryRay (camera.h:23-30) for pixel coordinates x, y (reals): unit directions"""
    pos, tl, tr, bl = camera
    u, v = np.asarray(x, np.float64) / W, np.asarray(y, np.float64) / H
    P = tl + u[..., None] * (tr - tl) + v[..., None] * (bl - tl)
    D = P - pos
    return D / np.linalg.norm(D, axis=-1, keepdims=True)


def pixel_truth(camera, W, H, rho, sky, quad, sub=8):
    """(E, E2 [H, W, 3], sky share [H, W]) of one ProcessTile sample of every pixel (renderer.cpp:121-126: pixel (x, y) of the accumulator = primary rays through
    (x + r, y + r')): the sub x sub sub-pixel average of "sky texel if the ray goes up, floor_radiance at the plane hit if it goes down".  For views in which no
    primary ray meets the quad or a mesh.  sky: [h, w, 3] uint8."""
    s = (np.arange(sub) + 0.5) / sub
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    X = x[..., None, None] + s[None, None, None, :]; Y = y[..., None, None] + s[None, None, :, None]
    X, Y = np.broadcast_arrays(X, Y)
    D = primary_dirs(camera, W, H, X, Y)
    up = D[..., 1] > 0
    rgb, _, _ = sky_lookup(D, sky)
    t = -(camera[0][1] - FLOOR_Y) / np.where(up, -1.0, D[..., 1])
    P = camera[0] + t[..., None] * D
    P[up] = [quad[0][0], FLOOR_Y, quad[0][2]]                              # any valid point: masked below
    L_sky = texel_rgb(sky[0, 0, :3])
    assert (sky[..., :3] == sky[0, 0, :3]).all(), "floor_radiance needs a constant sky"
    fm, f2 = floor_radiance(P, rho, L_sky, quad)
    E = np.where(up[..., None], rgb, fm); E2 = np.where(up[..., None], rgb * rgb, f2)
    return E.mean(axis=(2, 3)), E2.mean(axis=(2, 3)), up.mean(axis=(2, 3))


def light_pixels(camera, W, H, quad, grow=0.5, margin=1e-3):
    """[H, W] bool: the pixel's footprint grown by `grow` pixels on every side lies inside the quad's projection (four corner rays; both shapes are convex),
    `margin` inside its edge"""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ok = np.ones((H, W), bool)
    for dx in (-grow, 1 + grow):
        for dy in (-grow, 1 + grow):
            D = primary_dirs(camera, W, H, x + dx, y + dy)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (quad[0][1] - camera[0][1]) / D[..., 1]
            I = camera[0] + t[..., None] * D
            ok &= (t > 0) & (np.abs(I[..., 0] - quad[0][0]) < quad[1] - margin) & (np.abs(I[..., 2] - quad[0][2]) < quad[1] - margin)
    return ok


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Whitted
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def whitted_floor(P, rho, quad, boxes=(), along_normal=False):
    """Trace of a primary ray that meets the diffuse floor at P (2. WhittedStyle/renderer.cpp:74-79, 105-126): rho / pi * (L_light cos / d^2 V + 0.3), the light
    point 0.01 under the quad's centre (file_scene.cpp:156-162), V = 0 where a box stands between (file_scene.cpp:177-187; the shadow ray runs from EPSILON to
    d - 2 EPSILON (:117) and the quad itself lies 0.01 / cos beyond its end).  Returns (rgb [..., 3], V)"""
    P = np.asarray(P, np.float64)
    lp = np.asarray(quad[0], np.float64) - [0.0, 0.01, 0.0]                # 0.01 down in world y, whatever the quad's frame and size
    if along_normal:                                                       # a WRONG model, for the tests' controls: 0.01 along the quad's normal -R[:, 1]
        lp = np.asarray(quad[0], np.float64) - 0.01 * quad_frame(quad)[1][:, 1]
    Lv = lp - P; d = np.linalg.norm(Lv, axis=-1); Lv = Lv / d[..., None]
    V = np.ones(P.shape[:-1], bool)
    for b in boxes:
        V &= ~b.blocks(P + Lv * EPSILON, Lv, d - 2 * EPSILON)
    # the quad itself (IsOccluded tests it first, file_scene.cpp:177-187): the light point lies 0.01 under the centre in world y, so a floor point on the far
    # side of a TILTED quad's plane sees it through the quad, and is dark
    c, R, half = quad_frame(quad)
    O = P + Lv * EPSILON
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((c - O) @ R[:, 1]) / (Lv @ R[:, 1])
    I = O + np.where(np.isfinite(t), t, 0.0)[..., None] * Lv - c
    V &= ~(np.isfinite(t) & (t > 0) & (t < d - 2 * EPSILON) & (np.abs(I @ R[:, 0]) < half) & (np.abs(I @ R[:, 2]) < half))
    cos = Lv[..., 1]
    return np.asarray(rho, np.float64) / np.pi * (LIGHT * (cos / (d * d) * V)[..., None] + 0.3), V


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# scene files
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def write_tga(path, rgb8, w=128, h=128):
    """one colour as an uncompressed 24-bit TGA: 18-byte header, then BGR bytes (w >= 100: file_scene.cpp:16 divides the floor texture's width by 100)"""
    hdr = np.zeros(18, np.uint8); hdr[2] = 2; hdr[12:14] = [w & 255, w >> 8]; hdr[14:16] = [h & 255, h >> 8]; hdr[16] = 24; hdr[17] = 0x20
    px = np.empty((h, w, 3), np.uint8); px[:] = np.asarray(rgb8, np.uint8)[::-1]
    with open(str(path), "wb") as f:
        f.write(hdr.tobytes()); f.write(px.tobytes())
    return str(path)


FLOOR_RGB = (200, 160, 120)
SKY_RGB = (90, 140, 230)
MAT_RGB = (192, 192, 192)                          # 0xc0 / 255
MIRROR_RGB = (192, 128, 64)
LIGHT_POS = (1.2, 3.0, 0.5)                        # off-centre: a mirrored or transposed image moves the light's pool of brightness to other tiles
QUAD = (np.array(LIGHT_POS), LIGHT_HALF)
FLOOR_POINTS = np.array([[1.2, -1.0, 0.5], [0.3, -1.0, 1.6], [3.0, -1.0, -1.0]])       # under the quad's centre, beside it, far from it
# under a turned quad: two more, either side of the centre along x (the point under the centre cannot tell R from its transpose)
QUAD_FLOOR_POINTS = np.array(FLOOR_POINTS.tolist() + [[2.4, -1.0, 0.5], [0.0, -1.0, 0.5]])
EYE = np.array([0.0, 0.3, -2.0])


def _half_turn_euler(k):
    """the angles (degrees) of RotateX * RotateY * RotateZ that make the half turn about k: R = 2 k k^T - 1, a SYMMETRIC rotation"""
    k = np.asarray(k, np.float64) / np.linalg.norm(k)
    R = 2.0 * np.outer(k, k) - np.eye(3)
    return tuple(float(v) for v in np.rad2deg([np.arctan2(-R[1, 2], R[2, 2]), np.arcsin(R[0, 2]), np.arctan2(-R[0, 1], R[0, 0])]))


# FileScene turns vertex normals by the TRANSPOSED matrix (model.cpp:70 hands invT to TransformVector; TLASFileScene turns them by T, blas_bvh.cpp:397), so the
# shading normal of a rotated cube is its face normal in a TLASFileScene only.  The slab is turned by a half turn, for which R^T = R: both scene kinds shade the
# face the ray meets with the face's own normal, and the recursion of slab_radiance holds for both.  (The mirror of S1 is where the transposed normal is pinned.)
SLAB = dict(position=(0.0, 0.5, 2.0), rotation=_half_turn_euler((0.5, -0.3, 1.8)), scale=(0.5, 0.5, 0.5))
SLAB_ABSORPTION = (0.5, 0.0, 0.25)
SLAB_AXIS = 2                                      # the ray runs along the box's z axis, about (0.50, -0.30, 0.81): no zero component
_n = Box(**SLAB).R[:, SLAB_AXIS]
# an axis-parallel mirror cube whose top face turns the ray that left the slab up into the sky
BEHIND = dict(position=tuple(float(v) for v in np.round(np.asarray(SLAB["position"]) + 2.5 * _n - [0.0, 0.3, 0.0], 3)), rotation=(0.0, 0.0, 0.0), scale=(0.3, 0.3, 0.3))
# turned about x as well: sky_gradient.png changes with the elevation only, and a turn about y alone leaves the elevation of a reflection off a side face alone
MIRROR = dict(position=(0.0, 0.5, 2.0), rotation=(20.0, 25.0, 0.0), scale=(0.5, 0.5, 0.5))


def write_scenes(tmp_path, write_scene):
    """the scenes as XML files under tmp_path: S0 = floor, light and one-colour sky (the cube lies under the floor), S1 = a mirror cube under sky_gradient.png,
    S2 = the dielectric slab, a mirror cube behind it, one-colour sky.  write_scene = tests/test_gpu_golden_and_edges.write_scene.  Returns {name: path}."""
    floor = write_tga(tmp_path / "floor.tga", FLOOR_RGB); sky = write_tga(tmp_path / "sky.tga", SKY_RGB)
    mat = write_tga(tmp_path / "mat.tga", MAT_RGB, 4, 4); mir = write_tga(tmp_path / "mir.tga", MIRROR_RGB, 4, 4)
    none = (0.0, 0.0, 0.0)

    def obj(d, mi):
        return ("cube", mi, d["position"], d["rotation"], d["scale"])
    s0 = write_scene(tmp_path, "cube", name="s0.xml", pos=(0.0, -5.0, 2.0), rot=none, light=LIGHT_POS, floor_tex=floor, sky=sky)
    s1 = write_scene(tmp_path, "cube", name="s1.xml", pos=MIRROR["position"], rot=MIRROR["rotation"], scale=MIRROR["scale"], mats=[(1.0, 0.0, none, mir)],
                     light=LIGHT_POS, floor_tex=floor)
    s2 = write_scene(tmp_path, "cube", name="s2.xml", pos=SLAB["position"], rot=SLAB["rotation"], scale=SLAB["scale"],
                     mats=[(0.0, 1.0, SLAB_ABSORPTION, mat), (1.0, 0.0, none, mir)], extra_objects=[obj(BEHIND, 1)], light=LIGHT_POS, floor_tex=floor, sky=sky)
    return dict(S0=s0, S1=s1, S2=s2)


def slab_ray():
    """the normal-incidence ray of S2 from this module's own transform of cube.obj: (O, D float32, thickness, distance to the near face, the slab's Box)"""
    b = Box(**SLAB)
    n = b.R[:, SLAB_AXIS]
    D = n.astype(np.float32); D = D / np.float32(np.linalg.norm(D.astype(np.float64)))
    O = (b.c - 3.0 * n).astype(np.float32)
    t0, t1, axis, sign = b.intersect(O.astype(np.float64), D.astype(np.float64))
    assert axis == SLAB_AXIS and sign == -1
    return O, D, float(t1 - t0), float(t0), b


def seeds(k, n):
    return np.random.default_rng(k).integers(1, 2 ** 32, n).astype(np.uint32)


def oracle_samples(o, O, D, seeds, inside=0):
    """orc_sample of ONE ray for every seed (a tight ctypes loop: a million samples a second): [n, 3] float32.  `o` is an orc.Oracle: the thing under test."""
    import ctypes as C
    n = len(seeds)
    ray = np.zeros(7, np.float32); ray[0:3] = O; ray[3:6] = D; ray[6:7].view(np.int32)[0] = inside
    sa = np.array(seeds, np.uint32); out = np.zeros((n, 3), np.float32)
    f, h, pr, ps, po = o.L.orc_sample, o.h, C.c_void_p(ray.ctypes.data), sa.ctypes.data, out.ctypes.data
    for i in range(n):
        f(h, pr, C.c_void_p(ps + 4 * i), C.c_void_p(po + 12 * i))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# PrimitiveScene (infra/scene/primitive_scene.cpp:4-67 for the constants, :92-175 for the order and the SPEEDTRIX root choices; template/primitives.h)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _affine(R=None, t=(0.0, 0.0, 0.0)):
    M = np.eye(4); M[:3, 3] = t
    if R is not None:
        M[:3, :3] = R
    return M


def _rot(axis, a):
    """mat4::RotateX / Y / Z (tmplmath.h:673-675)"""
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def prim_state(t):
    """the animated transforms of PrimitiveScene::SetTime (primitive_scene.cpp:43-67); t as the float32 the scene holds"""
    t = float(np.float32(t))
    quad = _affine(t=(0, float(np.float32(2.6)), 2)) @ _affine(_rot("z", np.sin(t * float(np.float32(0.6))) * float(np.float32(0.1)))) @ _affine(t=(0, float(np.float32(-0.9)), 0))
    cube = _affine(t=(float(np.float32(1.8)), 0, 2.5)) @ _affine(_rot("y", t * 0.5)) @ _affine(_rot("x", np.pi / 4)) @ _affine(_rot("z", np.pi / 4))
    torus = _affine(t=(-0.25, 0, 2)) @ _affine(_rot("x", np.pi / 4))                       # :23, tmplmath.h:734
    tm = 1.0 - (np.fmod(t, 2.0) - 1.0) ** 2
    ball = np.array([float(np.float32(-1.8)), float(np.float32(-0.4)) + tm, 1.0])
    return dict(quad=np.linalg.inv(quad), cube=np.linalg.inv(cube), torus=np.linalg.inv(torus), ball=ball)


NEAR = 1e-3


def prim_truth(O, D, t):
    """PrimitiveScene::FindNearest in float64: (t, objIdx, margin) per ray.  margin: the gap between the nearest candidate and the second nearest (a candidate is any
    root an object could return), the distance of a quad-plane hit to the quad's edge, how far a candidate root is from 0 (the hit tests are t > 0), and how far
    a grazing ray is from touching: a ray whose margin is under 1e-3 may be answered either way by float32 arithmetic.
    Quirks of the SPEEDTRIX paths that the answer depends on: the ball takes only its NEAR root (:151: a ray that starts inside does not see it), the
    rounded-corner sphere only its FAR root (:164); the cube returns tmin if positive, else tmax (primitives.h:220-227); walls by the sign of D (:105-113)."""
    O, D = np.asarray(O, np.float64), np.asarray(D, np.float64)
    n = len(O); st = prim_state(t)
    INF = 1e34
    cand_t = []; cand_id = []
    margin = np.full(n, np.inf)

    def near_zero(tc, live=None):
        a = np.abs(tc)
        if live is not None:
            a = np.where(live, a, np.inf)
        np.minimum(margin, a, out=margin)

    # walls (:100-113): x = -3 | 2.99, y = -1 | 2, z = -3 | 3.99
    for ax, (lo, hi, idlo, idhi) in enumerate([(-3.0, float(np.float32(2.99)), 4, 5), (-1.0, 2.0, 6, 7), (-3.0, float(np.float32(3.99)), 8, 9)]):
        pos = D[:, ax] >= 0
        plane = np.where(pos, hi, lo)
        with np.errstate(divide="ignore", invalid="ignore"):
            tw = (plane - O[:, ax]) / D[:, ax]
        cand_t.append(np.where(tw > 0, tw, INF)); cand_id.append(np.where(pos, idhi, idlo))
    # light quad (primitives.h:331-346)
    o = O @ st["quad"][:3, :3].T + st["quad"][:3, 3]; d = D @ st["quad"][:3, :3].T
    with np.errstate(divide="ignore", invalid="ignore"):
        tq = o[:, 1] / -d[:, 1]
    ix, iz = o[:, 0] + tq * d[:, 0], o[:, 2] + tq * d[:, 2]
    edge = np.minimum(LIGHT_HALF - np.abs(ix), LIGHT_HALF - np.abs(iz))
    quad_t = np.where((tq > 0) & (edge > 0), tq, INF); quad_edge = np.where(tq > 0, np.abs(edge), np.inf)
    cand_t.append(quad_t); cand_id.append(np.full(n, 0))
    # spheres: oc, b, d = b^2 - (|oc|^2 - r^2)
    for centre, r2, idx, far in ((st["ball"], float(np.float32(0.36)), 1, False), (np.array([0.0, 2.5, float(np.float32(-3.07))]), 64.0, 2, True)):
        oc = O - centre; b = (oc * D).sum(1); dd = b * b - ((oc * oc).sum(1) - r2)
        root = np.sqrt(np.maximum(dd, 0.0))
        ts = (root - b) if far else (-b - root)
        cand_t.append(np.where((dd > 0) & (ts > 0), ts, INF)); cand_id.append(np.full(n, idx))
        near_zero(ts, dd > 0)
        graze = (np.abs(dd) < NEAR * NEAR) & (-b > 0)
        cand_t.append(np.where(graze, -b, INF)); cand_id.append(np.full(n, -2 - idx))          # a phantom candidate: only its gap to the nearest counts
    # cube (primitives.h:198-227): box +-0.575 in object space
    o = O @ st["cube"][:3, :3].T + st["cube"][:3, 3]; d = D @ st["cube"][:3, :3].T
    half = float(np.float32(1.15)) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (-half - o) / d; t2 = (half - o) / d
    tmin, tmax = np.minimum(t1, t2).max(1), np.maximum(t1, t2).min(1)
    hit = tmin < tmax
    tc = np.where(hit & (tmin > 0), tmin, np.where(hit & (tmax > 0), tmax, INF))
    cand_t.append(tc); cand_id.append(np.full(n, 3))
    cand_t.append(np.where(hit & (tmin > 0) & (tmax > 0), tmax, INF)); cand_id.append(np.full(n, 3))
    near_zero(tmin, hit); near_zero(tmax, hit)
    grz = (np.abs(tmax - tmin) < NEAR) & (np.maximum(tmin, tmax) > 0)
    cand_t.append(np.where(grz & ~hit, np.minimum(tmin, tmax), INF)); cand_id.append(np.full(n, -5))
    np.minimum(margin, np.where(grz & hit, np.abs(tmax - tmin), np.inf), out=margin)
    # torus (primitives.h:380-461 solves the same quartic in closed form): (t^2 + 2 k t + m + R^2 - r^2)^2 = 4 R^2 ((Ox + t Dx)^2 + (Oy + t Dy)^2), around object z
    o = O @ st["torus"][:3, :3].T + st["torus"][:3, 3]; d = D @ st["torus"][:3, :3].T
    Rr, rr = float(np.float32(0.8)), float(np.float32(0.25))
    k = (o * d).sum(1); m = (o * o).sum(1)
    inside_sphere = k * k - m + (Rr + rr) ** 2 >= 0                                          # :398-399, the only rays that can meet it
    c = m + Rr * Rr - rr * rr
    xy_dd = d[:, 0] ** 2 + d[:, 1] ** 2; xy_od = o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1]; xy_oo = o[:, 0] ** 2 + o[:, 1] ** 2
    tor1 = np.full(n, INF); tor2 = np.full(n, INF); tor_soft = np.full(n, INF)
    for i in np.flatnonzero(inside_sphere):
        r = np.roots([1.0, 4 * k[i], 4 * k[i] ** 2 + 2 * c[i] - 4 * Rr * Rr * xy_dd[i], 4 * k[i] * c[i] - 8 * Rr * Rr * xy_od[i], c[i] ** 2 - 4 * Rr * Rr * xy_oo[i]])
        real = np.sort(r.real[np.abs(r.imag) < 1e-9])
        margin[i] = min(margin[i], np.abs(real).min() if len(real) else np.inf)
        p = real[real > 0]
        if len(p) > 0: tor1[i] = p[0]
        if len(p) > 1: tor2[i] = p[1]
        soft = r[(np.abs(r.imag) >= 1e-9) & (np.abs(r.imag) < NEAR) & (r.real > 0)]           # a ray that all but touches: a phantom candidate
        if len(soft): tor_soft[i] = soft.real.min()
    cand_t += [tor1, tor2, tor_soft]; cand_id += [np.full(n, 10), np.full(n, 10), np.full(n, -6)]
    T = np.stack(cand_t, 1); I = np.stack(cand_id, 1)
    rows = np.arange(n)
    # the nearest REAL candidate; phantoms (negative ids) only shrink the margin
    realT = np.where(I >= 0, T, INF); best = realT.argmin(1)
    tb = realT[rows, best]; ib = I[rows, best]
    others = np.where(np.arange(T.shape[1])[None, :] == best[:, None], INF, T)
    # the two cube candidates and the two torus roots belong to one object, yet which root is returned decides t: they count as rivals too
    gap = others.min(1) - tb
    np.minimum(margin, np.abs(gap), out=margin)
    # the quad's edge matters where its plane hit is the nearest thing or nearly so
    qnear = np.where(np.isfinite(quad_edge) & (tq > 0) & (tq < tb + NEAR), quad_edge, np.inf)
    np.minimum(margin, qnear, out=margin)
    return tb, ib, margin


# PrimitiveScene: |t_oracle - t_truth| per object over test_gpu_primitive_scene._rays(20000, 11) at t = 0, 1.3, 7.77 (rays with margin >= 1e-3), measured with
# tests/test_analytic_truth_cpu.py::test_primitive_scene (it prints the observed values); asserted = 4 x observed (room for the rays a later edit of _rays would
# draw; the GPU returns the oracle's bits).  The torus: 4 x its 99.9 % quantile for the quantile, and a separate cap on the maximum.
#                 object: (observed max |dt|, asserted)
PRIM_TOLERANCE = {
    "walls": (1.04e-6, 4.2e-6),
    "light quad": (3.94e-6, 1.6e-5),
    "rounded-corner sphere": (8.58e-7, 3.5e-6),
    "cube": (5.61e-6, 2.3e-5),
    "ball": (9.92e-5, 4.0e-4),
    "torus 99.9 %": (1.025e-3, 4.1e-3),
    "torus max": (1.955e-3, 7.9e-3),
}
PRIM_MAX_LOW_MARGIN = 0.005                         # share of rays whose margin may be under 1e-3 (observed: 15 of 20000)


def prim_check(t_got, idx_got, t_want, idx_want, margin):
    """the assertions of both PrimitiveScene tests; returns {row of PRIM_TOLERANCE: observed} for the report"""
    ok = margin >= NEAR
    assert (~ok).mean() <= PRIM_MAX_LOW_MARGIN, (~ok).sum()
    bad = np.flatnonzero(ok & (idx_got != idx_want))
    assert len(bad) == 0, ("objIdx", bad[:8].tolist(), idx_got[bad[:8]].tolist(), idx_want[bad[:8]].tolist())
    err = np.abs(np.asarray(t_got, np.float64) - t_want)
    seen = {}
    for name, ids in (("walls", range(4, 10)), ("light quad", [0]), ("rounded-corner sphere", [2]), ("cube", [3]), ("ball", [1])):
        m = ok & np.isin(idx_want, list(ids))
        assert m.sum() >= 100, (name, int(m.sum()))
        seen[name] = float(err[m].max())
        assert seen[name] <= PRIM_TOLERANCE[name][1], (name, seen[name])
    m = ok & (idx_want == 10)
    assert m.sum() >= 1000
    seen["torus 99.9 %"] = float(np.quantile(err[m], 0.999)); seen["torus max"] = float(err[m].max())
    assert seen["torus 99.9 %"] <= PRIM_TOLERANCE["torus 99.9 %"][1] and seen["torus max"] <= PRIM_TOLERANCE["torus max"][1], seen
    return seen


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the cases, shared by tests/test_analytic_truth_cpu.py (the oracle) and tests/test_gpu_analytic_truth.py (the kernels): inputs, wanted moments, checks
# ---------------------------------------------------------------------------------------------------------------------------------------------------
# N per case from the truth's own sigma: sigma / sqrt(N) <= 0.5 % of the mean for a floor point (sigma / mean is 2.6 .. 5.7: the quad is a small bright target for a
# uniform bounce), <= 0.1 % for the slab at depth limits 3 and 5 (sigma / mean <= 0.52).  At depth limit 1 only the ray reflected off the near face returns
# light: mean = albedo * R0 * sky, sigma / mean = 1 / sqrt(R0) = 11, and 0.1 % would take 1.2e8 samples; 2e6 give 0.8 %.  The criterion itself is the same.
N_FLOOR, N_SLAB, N_SLAB_1 = 1_400_000, 300_000, 2_000_000
W, H, FRAMES = 64, 64, 2048
LIGHT_CAMERA = ((1.2, -0.5, 0.3), (1.2, 3.0, 0.5))                         # under the quad, looking up at it
LIGHT_FRAMES = 64


def _unit32(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def check_mean(samples, want, second, what):
    """the z criterion on the mean of samples [n, 3]; prints the figures before it asserts"""
    n = len(samples)
    assert np.isfinite(samples).all(), what
    mean = np.asarray(samples).mean(axis=0, dtype=np.float64)
    ok, z = z_ok(mean, want, second, n)
    print("%s: n %d mean %s want %s z %s" % (what, n, mean, np.asarray(want), np.round(z, 2)))
    assert ok, (what, mean.tolist(), np.asarray(want).tolist(), z.tolist())
    return z


def floor_case(k, quad=None, salt=0):
    """floor point k of S0: (O, D float32, E, E2, seeds); quad: a look's quad (then k indexes QUAD_FLOOR_POINTS), salt: seeds of its own"""
    P = (FLOOR_POINTS if quad is None else QUAD_FLOOR_POINTS)[k]
    mean, second = floor_radiance(P, texel_rgb(FLOOR_RGB), texel_rgb(SKY_RGB), QUAD if quad is None else quad)
    if quad is not None:
        assert (Z * np.sqrt(second - mean * mean) / np.sqrt(N_FLOOR) <= 0.03 * mean).all()
        return EYE.astype(np.float32), _unit32(P - EYE), mean, second, seeds(1000 + 10 * salt + k, N_FLOOR)
    assert (np.sqrt(second - mean * mean) / np.sqrt(N_FLOOR) <= 0.005 * mean).all()
    return EYE.astype(np.float32), _unit32(P - EYE), mean, second, seeds(100 + k, N_FLOOR)


def slab_case(depth_limit):
    """S2's ray: (O, D float32, (E, E2), the same of the physical variant, seeds, thickness, distance to the near face)"""
    O, D, thickness, t0, _ = slab_ray()
    args = (texel_rgb(MAT_RGB), SLAB_ABSORPTION, thickness, texel_rgb(SKY_RGB), depth_limit, texel_rgb(MIRROR_RGB))
    want, phys = slab_radiance(*args), slab_radiance_physical(*args)
    n = N_SLAB_1 if depth_limit == 1 else N_SLAB
    if depth_limit >= 3:
        assert (np.sqrt(want[1] - want[0] ** 2) / np.sqrt(n) <= 0.001 * want[0]).all()
    return O, D, want, phys, seeds(200 + depth_limit, n), thickness, t0


def check_slab(samples, depth_limit, what):
    _, _, want, phys, _, _, _ = slab_case(depth_limit)
    check_mean(samples, want[0], want[1], what)
    if depth_limit >= 3:
        # the negative control: the test can tell the reference's slab from the physical one (which differs from depth limit 3 on: a third hit)
        ok, z = z_ok(np.asarray(samples).mean(axis=0, dtype=np.float64), phys[0], phys[1], len(samples))
        print("%s: physical variant z %s" % (what, np.round(z, 2)))
        assert not ok and max(abs(z[0]), abs(z[2])) > Z and abs(z[1]) <= Z, (what, z.tolist())      # it fails, and on an absorbing channel (red, blue), not on green


def shading_normal(box, axis, sign, kind):
    """the normal GetHitInfo returns for a face of cube.obj (flat vertex normals = the face normal in object space): kind 1 (TLASFileScene) turns it by T
    (blas_bvh.cpp:397), kind 0 (FileScene) by FastInvertedTransformNoScale(T) = the transposed matrix (model.cpp:57, :70), both normalised"""
    e = np.zeros(np.shape(axis) + (3,)); np.put_along_axis(e, np.asarray(axis)[..., None], np.asarray(sign, np.float64)[..., None], -1)
    M = box.R if kind == 1 else (box.R * box.half).T                       # (R S)^T = S R^T
    n = e @ M.T
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def mirror_case(kind, sky, n=8000):
    """rays at S1's mirror cube whose reflection (about the scene kind's shading normal) misses everything: (O, D float32, wanted rgb, entered face axis, the
    rgb that the OTHER scene kind's shading normal would give)"""
    rng = np.random.default_rng(300)
    b = Box(**MIRROR)
    O = np.stack([rng.uniform(-3.0, 3.0, n), rng.uniform(0.2, 4.0, n), rng.uniform(-2.0, 6.0, n)], 1).astype(np.float32)           # all around and above
    D = _unit32(b.c + rng.uniform(-0.6, 0.6, (n, 3)) - O)
    O64, D64 = O.astype(np.float64), D.astype(np.float64)
    t0, t1, axis, sign = b.intersect(O64, D64)
    I = O64 + t0[:, None] * D64
    local = np.abs((I - b.c) @ b.R)
    off_edge = (np.sort(local, axis=1)[:, 1] < b.half[0] - 1e-3)                              # the hit point is 1e-3 off the face's edges
    N = shading_normal(b, axis, sign, kind)
    N = np.where(((N * D64).sum(1) > 0)[:, None], -N, N)                                     # file_scene.cpp:211
    R = D64 - 2.0 * (D64 * N).sum(1, keepdims=True) * N
    start = I + R * EPSILON

    def near_quad(P, V, tmax):
        """may the ray P + t V, 0 < t < tmax, meet the light quad (grown by 0.01)"""
        with np.errstate(divide="ignore", invalid="ignore"):
            tl = (QUAD[0][1] - P[:, 1]) / V[:, 1]
        Il = P + tl[:, None] * V
        return (tl > 0) & (tl < tmax) & (np.abs(Il[:, 0] - QUAD[0][0]) < QUAD[1] + 0.01) & (np.abs(Il[:, 2] - QUAD[0][2]) < QUAD[1] + 0.01)
    light = near_quad(start, R, np.inf) | near_quad(O64, D64, t0 + 0.01)
    r0, r1, _, _ = b.intersect(start, R)
    again = (r0 <= r1 + 1e-3) & (r1 > -1e-3)
    rgb, x, y = mirror_radiance(D64, N, texel_rgb(MIRROR_RGB), sky)
    keep = (t0 < t1) & (t0 > 0) & off_edge & (R[:, 1] > 0.02) & ~light & ~again & (border_distance(x, y) >= 1e-3)
    N2 = shading_normal(b, axis, sign, 1 - kind)
    N2 = np.where(((N2 * D64).sum(1) > 0)[:, None], -N2, N2)
    rgb_other, _, _ = mirror_radiance(D64, N2, texel_rgb(MIRROR_RGB), sky)                   # what the other scene kind's normal would give: the test's contrast
    return O[keep], D[keep], rgb[keep], axis[keep], rgb_other[keep]


_truth_cache = {}


def render_truth(sky, quad=None, key="render"):
    """pixel_truth of S0 through the default camera, computed once per key: (E, E2, sky share)"""
    if key not in _truth_cache:
        _truth_cache[key] = pixel_truth(camera_default(W, H), W, H, texel_rgb(FLOOR_RGB), sky, QUAD if quad is None else quad)
    return _truth_cache[key]


def check_render(acc, frames, sky, what, quad=None, key="render"):
    """an accumulator [H, W, 4] of `frames` frames of S0 through the default camera: sky pixels, floor-tile means (ProcessTile's pixel <-> tile <-> accumulator
    mapping: the quad is off-centre, so a transposed or mirrored image moves the tile means by many sigma)"""
    E, E2, up = render_truth(sky, quad, key)
    assert np.isfinite(acc).all() and not acc[..., 3].any()
    img = acc[..., :3].astype(np.float64) / frames
    sky_px = up == 1.0; floor_px = up == 0.0
    assert (sky_px | floor_px).all()
    assert (np.abs(img[sky_px] - E[sky_px]) <= 1e-4 * E[sky_px]).all(), (what, "sky")
    tiles = lambda a: a.reshape(H // 16, 16, W // 16, 16, -1).swapaxes(1, 2).reshape(H // 16, W // 16, 256, -1)
    n_sky = n_floor = 0; zmax = 0.0
    for ty in range(H // 16):
        for tx in range(W // 16):
            s = tiles(sky_px[..., None])[ty, tx, :, 0]
            if s.all():
                n_sky += 1; continue
            assert not s.any()
            n_floor += 1
            mean = tiles(img)[ty, tx].mean(0); want = tiles(E)[ty, tx].mean(0)
            var = (tiles(E2)[ty, tx] - tiles(E)[ty, tx] ** 2).sum(0) / (256.0 ** 2 * frames)          # independent samples: 256 pixels x frames
            z = (mean - want) / np.sqrt(var); zmax = max(zmax, np.abs(z).max())
            assert (np.abs(mean - want) <= Z * np.sqrt(var)).all(), (what, "tile", tx, ty, mean.tolist(), want.tolist(), z.tolist())
    print("%s: %d sky tiles, %d floor tiles, largest |z| of a tile mean %.2f" % (what, n_sky, n_floor, zmax))
    assert (n_sky, n_floor) == (8, 8)


def check_light_pixels(acc, frames, what, quad=None, beyond=None):
    """quad: a parallel quad (centre, half) of another size; beyond: only the pixels that lie wholly OUTSIDE this smaller quad's projection (its edge grown by
    0.05: no corner of the pixel's footprint inside it)"""
    cam = camera_state(LIGHT_CAMERA[0], LIGHT_CAMERA[1], W, H)
    lit = light_pixels(cam, W, H, QUAD if quad is None else quad)
    if beyond is not None:
        touched = np.zeros((H, W), bool)
        for dx in (0.0, 1.0):
            for dy in (0.0, 1.0):
                y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
                D = primary_dirs(cam, W, H, x + dx, y + dy)
                t = (beyond[0][1] - cam[0][1]) / D[..., 1]
                I = cam[0] + t[..., None] * D
                touched |= (np.abs(I[..., 0] - beyond[0][0]) < beyond[1] + 0.05) & (np.abs(I[..., 2] - beyond[0][2]) < beyond[1] + 0.05)
        lit &= ~touched
    assert lit.sum() >= 16, lit.sum()
    want = (LIGHT * frames).astype(np.float32)                             # :69 returns (24, 24, 22) whatever the seed: `frames` exact additions
    assert (acc[lit][:, :3] == want).all(), (what, int(lit.sum()))
    return int(lit.sum())


def whitted_truth(boxes=(), quad=None):
    """the Whitted image of the floor through the default camera (2. WhittedStyle/renderer.cpp:144: rays through integer pixel coordinates): (rgb [H, W, 3],
    checked [H, W] bool = floor pixels away from the shadow's and the boxes' edges, floor [H, W] bool)"""
    cam = camera_default(W, H)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")

    def at_(dx, dy):
        D = primary_dirs(cam, W, H, x + dx, y + dy)
        down = D[..., 1] < 0
        t = -(cam[0][1] - FLOOR_Y) / np.where(down, D[..., 1], -1.0)
        P = cam[0] + t[..., None] * D
        rgb, V = whitted_floor(P, texel_rgb(FLOOR_RGB), QUAD if quad is None else quad, boxes)
        hit_box = np.zeros(down.shape, bool)
        for b in boxes:
            hit_box |= b.blocks(np.broadcast_to(cam[0], D.shape), D, np.where(down, t, np.inf))
        return rgb, V, down & ~hit_box, hit_box
    rgb, V, floor, hit_box = at_(0.0, 0.0)
    steady = np.ones((H, W), bool)                                         # a tenth of a pixel around the ray: float32 moves it by far less
    for dx in (-0.1, 0.1):
        for dy in (-0.1, 0.1):
            _, V2, f2, hb2 = at_(dx, dy)
            steady &= (V2 == V) & (hb2 == hit_box)
    return rgb, floor & steady, floor


def check_whitted(acc, boxes, what, shadow, quad=None, tol=1.0 / 255.0):
    rgb, checked, floor = whitted_truth(boxes, quad)
    left_out = 1.0 - checked.sum() / floor.sum()
    err = np.abs(acc[..., :3].astype(np.float64) - rgb)[checked]
    print("%s: %d floor pixels, %.2f %% left out, largest error %.2e" % (what, floor.sum(), 100 * left_out, err.max()))
    assert floor.sum() >= W * H // 3 and left_out <= 0.03, (what, left_out)
    assert (left_out > 0) == shadow, (what, left_out)
    assert err.max() <= tol, (what, err.max())


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the quad looks on S0 (applied by crt_update_look / in a crt_render_looks job; the oracle: set_light_quad)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _rot64(axis, deg):
    a = np.radians(deg); c, s_ = np.cos(a), np.sin(a); R = np.eye(3)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s_, s_, c
    return R


# name: (rotation block, half size); the transforms are tests/render_looks_inputs.py's about LIGHT_POS
QUAD_LOOKS = {
    "zyx": (_rot64("z", 25.0) @ _rot64("y", 30.0) @ _rot64("x", -35.0), 0.5),
    "z25": (_rot64("z", 25.0), 0.5),
    "half_x": (np.diag([1.0, -1.0, -1.0]), 0.5),
    "size_0.9": (np.eye(3), 0.9),
    "zyx_size_0.9": (_rot64("z", 25.0) @ _rot64("y", 30.0) @ _rot64("x", -35.0), 0.9),
}


# check_whitted's bound under a look: the pixel is some 25 float32 operations on values of at most about 1, each within 2^-24 = 6e-8 relative: 1.5e-6.
# (The scene files' 1 / 255 was set for an image read back through 8-bit pixels; the accumulator compared here is float32.)
WHITTED_QUAD_TOL = 2e-6


def look_quad(name):
    R, half = QUAD_LOOKS[name]
    return (np.array(LIGHT_POS), R.astype(np.float32).astype(np.float64), half)      # (the cells a look carries are float32)


def look_cells(name):
    """(T [16], half) float32 of the look: R | LIGHT_POS"""
    R, half = QUAD_LOOKS[name]
    T = np.eye(4, dtype=np.float32); T[:3, :3] = R.astype(np.float32); T[:3, 3] = np.asarray(LIGHT_POS, np.float32)
    return T.reshape(16), np.float32(half)
