// auv_snapshot.h — layout of a snapshot row (auv_snapshot / auv_restore), shared by the host side (auv_capi_aux.hip), which
// builds it from the handle's shape, and the copy kernels (k7_snapshot.hip), which walk it.  The documented layout is in
// include/auv_hip.h; this is its machine form.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define AUV_SNAP_FORMAT 1        // part of the layout fingerprint: bump when a row's content or order changes
#define AUV_SNAP_HEAD 96         // bytes of the fixed head: counters | state | reward64, rew_path, rew_lidar | world index, collision
#define AUV_SNAP_SEGS 10         // per-environment rows behind the head

// One per-environment row of a handle buffer: environment e's row is `bytes` bytes at base + e * bytes (the buffer is dense),
// and sits at `off` (a multiple of 16) of the snapshot row, padded with zero bytes to the next multiple of 16.
struct AuvSnapSeg {
  char* base;
  uint32_t bytes;
  uint32_t off;
};

struct AuvSnapArgs {
  AuvSnapSeg seg[AUV_SNAP_SEGS];   // info64, nav64, step_info, episode, lidar_d, obs64, mover, limits, nearby, sector_d
  // the head's sources
  int4* counters;
  unsigned long long* state;       // [6][N] doubles, moved as 64-bit words
  unsigned long long* reward64;
  unsigned long long* rew_path;
  unsigned long long* rew_lidar;
  int32_t* world_idx;
  uint8_t* collision;
  unsigned int* skipped;           // [1] pairs skipped for an index out of range, over the life of the bank
  uint32_t row_bytes;              // multiple of 16
  uint32_t obs_off;                // where the obs64 row sits in the snapshot row
  int32_t n, n_worlds;
};
