// auv_mover_segs.h -- the pentagon of a moving obstacle, formed on demand from its pose: shared by the LiDAR sweep
// (k2_lidar.hip) and the renderer's geometry pass (k10_render.hip), so both see the same vertices bit for bit.
#pragma once
#include "auv_device.h"

namespace {   // (internal to each translation unit, like everything else the kernels inline)

// The five boundary segments of a mover (obstacles.py:217-233) formed on demand from its pose, with
// the arithmetic phase A used to form them: LDS keeps 40 bytes per mover instead of 160.
struct MoverSegs {
  double c, s, x, y, wd;    // snapped cos / sin of the heading, position, width
  __device__ __forceinline__ void vertex(int k, double& vx, double& vy) const {
    const double bx = (k <= 1) ? -wd / 2 : (k == 3 ? 3.0 / 2 * wd : wd / 2);
    const double by = (k == 0 || k == 4) ? -wd / 2 : (k == 3 ? 0.0 : wd / 2);
    const double x0 = 5.0 * wd / 18.0;
    const double xo = x0 - x0 * c, yo = 0.0 - x0 * s;
    vx = (c * bx + -s * by + xo) + x;
    vy = (s * bx + c * by + yo) + y;
  }
  __device__ __forceinline__ double4 operator[](int i) const {
    double ax, ay, bx, by;
    vertex(i, ax, ay);
    vertex(i == 4 ? 0 : i + 1, bx, by);
    return make_double4(ax, ay, bx, by);
  }
};

__device__ __forceinline__ MoverSegs mover_segs(const double4 rot, const double wd) {
  MoverSegs ms;
  ms.c = rot.x, ms.s = rot.y, ms.x = rot.z, ms.y = rot.w, ms.wd = wd;
  return ms;
}

}  // namespace
