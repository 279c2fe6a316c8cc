// tile_class.h — host only: what the primary rays of a 16x16 tile can NOT hit, proven before the launch (render_pool_kernel's `tileClass` argument).
//
// A pool wavefront renders one tile, and every primary ray starts at camPos and runs through one of the tile's 256 pixels, so whether a tile's rays can be
// accepted by the light quad's test, the floor plane's test or the slab test of the root's two children is a property of the tile.  classify_tiles decides it
// conservatively for every local tile: a SET bit is a proof that no primary ray of the tile passes that test as dev_common.h evaluates it in float; a CLEAR bit
// promises nothing and is always correct.  The kernel skips a test only under a set bit, so the samples do not change.
// kTileFloorSure is the one bit that proves the opposite: EVERY primary ray of the tile passes the floor plane's test (0 < t < 1e34), so with kTileNoLight and
// kTileNoTree (kTileFloor) the outcome of the whole primary FindNearest is known: the floor, at t = -primFloor / D.y.
//
// All arithmetic is double on the exact floats of the Scene block.  What makes a double result a proof about the kernel's float arithmetic is a guard band:
//   * the jitter (float)s * 2^-32 can round to 1.0, so a tile's pixel coordinates fill the CLOSED square [16 tx, 16 tx + 16] x [16 ty, 16 ty + 16]; the square is
//     classified GROWN BY ONE PIXEL on every side;
//   * the magnitude guard: if one pixel's step on the screen plane is below 2^-16 of the largest |coordinate| in play (camPos, screen corners, root-child boxes,
//     light / floor operands), no bit is set anywhere: the float rounding of P, v and the slab products (a few 2^-24 of that magnitude each) is then no longer
//     negligible against one pixel.  Above it those errors move a ray by less than 2^-6 pixel;
//   * sign decisions on v.y keep a margin of 2^-18 of that magnitude; a root-child corner nearer to the eye than 1/16 of the screen plane's distance clears
//     kTileNoTree everywhere (the rounding of lo - camPos is magnified on the screen by that ratio).
#pragma once
#include <cmath>
#include <cstring>
#include "layout.h"

namespace crt {

// cls[i] (bits: layout.h kTileNoLight / kTileNoFloor / kTileNoTree / kTileFloorSure) for the local tiles i = 0 .. tileCount - 1 (tile tileFirst + i * tileStride of a tilesX-wide grid) of a W x H image
inline void classify_tiles(const Scene& s, int W, int H, uint32_t tilesX, uint32_t tileFirst, uint32_t tileStride, uint32_t tileCount, uint8_t* cls)
{
    if (tileCount == 0) return;
    memset(cls, 0, tileCount);
    if (W <= 0 || H <= 0 || tilesX == 0) return;
    const double cam[3] = {s.camPos[0], s.camPos[1], s.camPos[2]};
    double TL[3], R[3], Dn[3];
    for (int k = 0; k < 3; k++) { TL[k] = s.topLeft[k]; R[k] = (double)s.topRight[k] - s.topLeft[k]; Dn[k] = (double)s.bottomLeft[k] - s.topLeft[k]; }
    const bool wantTree = s.rootIsPair != 0, wantFloor = s.floorAxisY != 0, wantLight = s.lightAxis != 0;
    if (!wantTree && !wantFloor && !wantLight) return;

    // ---- magnitude guard ----
    double mag = 0; bool finite = true;
    auto see = [&](double x) { if (!std::isfinite(x)) finite = false; else if (std::fabs(x) > mag) mag = std::fabs(x); };
    for (int k = 0; k < 3; k++) { see(cam[k]); see(TL[k]); see(s.topRight[k]); see(s.bottomLeft[k]); see(TL[k] + R[k] + Dn[k]); }
    if (wantTree) for (int c = 0; c < 2; c++) for (int k = 0; k < 3; k++) { see(s.rootPair[8 * c + k]); see(s.rootPair[8 * c + 4 + k]); }
    if (wantLight) { see(s.lightInvT[3]); see(s.lightInvT[7]); see(s.lightInvT[11]); see(s.lightSize); see(s.primLight[0]); see(s.primLight[1]); see(s.primLight[2]); }
    if (wantFloor) { see(s.floorD); see(s.primFloor); }
    see(s.invW); see(s.invH);
    const double rr = R[0] * R[0] + R[1] * R[1] + R[2] * R[2], dd = Dn[0] * Dn[0] + Dn[1] * Dn[1] + Dn[2] * Dn[2], rd = R[0] * Dn[0] + R[1] * Dn[1] + R[2] * Dn[2];
    if (!finite || !(rr > 0) || !(dd > 0)) return;
    const double invW = s.invW, invH = s.invH;                                  // the kernel's u = (x + jx) * invW
    const double step = std::fmin(std::sqrt(rr) * std::fabs(invW), std::sqrt(dd) * std::fabs(invH));
    if (!(step >= std::ldexp(mag, -16)) || !(invW > 0) || !(invH > 0)) return;
    const double tau = std::ldexp(mag, -18);

    // v = P - camPos at pixel coordinates (px, py): linear in both
    auto ray = [&](double px, double py, double v[3]) { for (int k = 0; k < 3; k++) v[k] = TL[k] + (px * invW) * R[k] + (py * invH) * Dn[k] - cam[k]; };

    // ---- kTileNoTree: the union screen rectangle (in pixels) of the 16 corners of the root's two children ----
    bool tree = wantTree; double bx0 = 1e300, bx1 = -1e300, by0 = 1e300, by1 = -1e300;
    if (tree) {
        const double N[3] = {R[1] * Dn[2] - R[2] * Dn[1], R[2] * Dn[0] - R[0] * Dn[2], R[0] * Dn[1] - R[1] * Dn[0]};
        const double num = (TL[0] - cam[0]) * N[0] + (TL[1] - cam[1]) * N[1] + (TL[2] - cam[2]) * N[2];
        const double det = rr * dd - rd * rd;                                   // Gram determinant: the screen's axes need not be orthogonal
        if (!(det > 1e-12 * rr * dd) || num == 0) tree = false;
        for (int c = 0; c < 2 && tree; c++)
            for (int i = 0; i < 8 && tree; i++) {
                double d[3];
                for (int k = 0; k < 3; k++) d[k] = (double)s.rootPair[8 * c + ((i >> k) & 1 ? 4 : 0) + k] - cam[k];
                const double den = d[0] * N[0] + d[1] * N[1] + d[2] * N[2];
                const double t = den != 0 ? num / den : -1;                     // cam + t d lies on the screen plane
                if (!(t > 0) || !(t <= 16)) { tree = false; break; }            // behind the eye, or too near to it
                double Q[3]; for (int k = 0; k < 3; k++) Q[k] = cam[k] + t * d[k] - TL[k];
                const double qr = Q[0] * R[0] + Q[1] * R[1] + Q[2] * R[2], qd = Q[0] * Dn[0] + Q[1] * Dn[1] + Q[2] * Dn[2];
                const double px = (qr * dd - qd * rd) / det / invW, py = (qd * rr - qr * rd) / det / invH;    // Q = (px invW) R + (py invH) Dn
                if (!std::isfinite(px) || !std::isfinite(py)) { tree = false; break; }
                bx0 = std::fmin(bx0, px); bx1 = std::fmax(bx1, px); by0 = std::fmin(by0, py); by1 = std::fmax(by1, py);
            }
    }

    // ---- operands of the floor plane's and the light quad's short tests (dev_common.h hit_light_floor<true>) ----
    const double fnum = s.primFloor;                                            // t = -num / D.y, accepted when t > 0
    const bool floorOk = wantFloor && fnum != 0;
    // kTileFloorSure also bounds t: |num| inside [2^-60, 2^60) and (per tile) |v.y| >= 2^-18 |v|, so |D.y| stays above 2^-19 and t inside (2^-61, 2^80)
    const bool sureOk = floorOk && std::fabs(fnum) < std::ldexp(1.0, 60) && std::fabs(fnum) >= std::ldexp(1.0, -60);
    const double lOy = s.primLight[0], lOx = s.primLight[1], lOz = s.primLight[2], lsize = s.lightSize;   // t = Oy / -D.y; I = (Ox, Oz) + t (D.x, D.z) inside (-size, size)^2
    const bool lightOk = wantLight && lOy != 0;

    for (uint32_t i = 0; i < tileCount; i++) {
        const uint32_t tile = tileFirst + i * tileStride;
        const double x0 = 16.0 * (tile % tilesX) - 1.0, x1 = x0 + 18.0, y0 = 16.0 * (tile / tilesX) - 1.0, y1 = y0 + 18.0;   // the grown square
        double v[4][3];
        ray(x0, y0, v[0]); ray(x1, y0, v[1]); ray(x0, y1, v[2]); ray(x1, y1, v[3]);
        double vyMin = v[0][1], vyMax = v[0][1];
        for (int j = 1; j < 4; j++) { vyMin = std::fmin(vyMin, v[j][1]); vyMax = std::fmax(vyMax, v[j][1]); }
        const bool up = vyMin >= tau, down = vyMax <= -tau;                     // the sign of D.y over the whole square (D = v * positive)
        uint8_t b = 0;
        if (tree && (x1 < bx0 || x0 > bx1 || y1 < by0 || y0 > by1)) b |= kTileNoTree;
        // floor: -num / D.y > 0 needs D.y and num of opposite sign
        if (floorOk && (fnum > 0 ? up : down)) b |= kTileNoFloor;
        // ... and is positive on the whole square when they are of opposite sign at all four corners (v.y is linear, |v| convex: the extremes are at the corners)
        if (sureOk && (fnum > 0 ? down : up)) {
            double vv = 0;
            for (int j = 0; j < 4; j++) vv = std::fmax(vv, v[j][0] * v[j][0] + v[j][1] * v[j][1] + v[j][2] * v[j][2]);
            const double vyAbsMin = fnum > 0 ? -vyMax : vyMin;
            if (std::isfinite(vv) && vyAbsMin >= std::ldexp(std::sqrt(vv), -18)) b |= kTileFloorSure;
        }
        // light: with q = -v.y / Oy (t = |v| / q), a ray is accepted only if q > 0 and the plane hit (Ox, Oz) + (v.x, v.z) / q lies inside (-size, size)^2, i.e. only if
        //   q > 0,  v.x - (size - Ox) q < 0,  v.x + (size + Ox) q > 0,  v.z - (size - Oz) q < 0,  v.z + (size + Oz) q > 0.
        // Each left side is affine in the pixel coordinates, so one that fails at all four corners fails on the whole square.  The first is "t <= 0 at all four
        // corners"; where t > 0 at all four, the other four say that the rectangle round the four plane hits is disjoint from the quad; and they also decide tiles
        // the horizon runs through, whose hits run off to infinity.  The guard band m is 2^-16 of the operands' magnitude on the same scale.
        if (lightOk) {
            double q[4], qMax = 0, vMax = 0;
            for (int j = 0; j < 4; j++) { q[j] = -v[j][1] / lOy; qMax = std::fmax(qMax, std::fabs(q[j])); vMax = std::fmax(vMax, std::fmax(std::fabs(v[j][0]), std::fabs(v[j][2]))); }
            const double m = std::ldexp(qMax * (std::fabs(lOx) + std::fabs(lOz) + std::fabs(lsize)) + vMax, -16), qTau = tau / std::fabs(lOy);
            bool behind = true, xHi = true, xLo = true, zHi = true, zLo = true;
            for (int j = 0; j < 4; j++) {
                behind = behind && q[j] <= -qTau;
                xHi = xHi && v[j][0] - (lsize - lOx) * q[j] >= m; xLo = xLo && v[j][0] + (lsize + lOx) * q[j] <= -m;
                zHi = zHi && v[j][2] - (lsize - lOz) * q[j] >= m; zLo = zLo && v[j][2] + (lsize + lOz) * q[j] <= -m;
            }
            if (std::isfinite(m) && (behind || xHi || xLo || zHi || zLo)) b |= kTileNoLight;
        }
        cls[i] = b;
    }
}

} // namespace crt
