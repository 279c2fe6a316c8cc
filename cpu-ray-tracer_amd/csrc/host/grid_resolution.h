// grid_resolution.h — the resolution lines of Grid::Build (infra/grid.cpp:14-26), in ONE place: the host build (accel_alt.cpp) and crt_build_grid_device (abi.cpp),
// which computes the bounds on the GPU and everything below on the host, call this function and so cannot disagree.  Plain floats: includable from any unit.
#pragma once
#include <cmath>

namespace crt {

// gridSize = localBounds.bmax3 - localBounds.bmin3; triCount = GetTriangleCount() (an int there, so 5 * triCount is an int product).  A flat mesh has volume 0:
// the quotient is +inf, gridSize[i] * inf is inf or NaN, and the conversion of either to int gives INT_MIN on x86 (cvttss2si), which the clamp turns into 1.
inline void grid_resolution(const float gridSize[3], int triCount, int resolution[3], float cellSize[3])
{
    const float cubeRoot = powf(5 * triCount / (gridSize[0] * gridSize[1] * gridSize[2]), 1 / 3.f);
    for (int i = 0; i < 3; i++) {
        int r = static_cast<int>(floorf(gridSize[i] * cubeRoot));
        r = r < 128 ? r : 128;                                                  // max(1, min(r, 128))
        resolution[i] = r > 1 ? r : 1;
    }
    for (int i = 0; i < 3; i++) cellSize[i] = gridSize[i] / resolution[i];
}

} // namespace crt
