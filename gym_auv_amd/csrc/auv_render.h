// auv_render.h -- the arguments of the renderer's two launches (k10_render.hip), by value in the kernel argument buffer.
#pragma once
#include "auv_device.h"

struct AuvRenderArgs {
  const int32_t* env_idx;   // [B] device copy of the caller's index list (checked on the host)
  int32_t B, H, W, view;
  double zoom, line_px;
  const double* trail;      // [B][L][2] or null
  const double* markers;    // [B][M][3] or null
  int32_t L, M;
  uint8_t palette[27];      // [9][3]
  uint8_t* frames;          // [B][H][W][3]
  double* cam;              // [B][8]
  double4* dyn_seg;         // [B][5 Mmax + 5]
  double4* ray_seg;         // [B][S]
  uint8_t* ray_q;           // [B][S]
  int32_t* trail_len;       // [B] rows of the trail before its first NaN row (written by the geometry pass)
#ifdef AUV_RENDER_DIAG
  unsigned long long* diag; // [2] diagnostic build only (tools/build_variant.sh render_diag "-DAUV_RENDER_DIAG"): segments before / after the tile cull
#endif
};

void auv_launch_render(const AuvDev& d, const AuvRenderArgs& a, hipStream_t st);
