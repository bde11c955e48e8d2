// What an SpMM call launches, as sputnik_hip_spmm_launch_shape reports it
// (include/sputnik_hip.h): filled by spmm_exec and the launch functions of the tiled
// kernels INSTEAD of launching when they are handed one.  Host only.
#pragma once

#include <cstdint>

namespace sputnik_hip {

struct SpmmLaunchShape {
  int family;  // SPUTNIK_HIP_SPMM_ROWGATHER / _PANEL / _NARROW64 / _WIDE256 / _WIDE512 / _FLAT
  // the two tiled files (spmm_tiled.hip, spmm_tiled64.hip) only; 0 / -1 otherwise
  int tile_cols, tile_rows, waves, rows_per_wave, chunk;
  int sparse, batch;   // the short-segment form and its kBatch (0 / 0: the long form, the 64-column kernel)
  int grid_x, grid_y, slots, nchunks, n_tiles, ksplits;
  // bytes from the start of the workspace (the layout is that of the shape alone, so a plan
  // made without the replica count and a call that plans for itself agree on it); -1: none
  int64_t row_ok_offset, table_offset, partials_offset;
};

inline SpmmLaunchShape spmm_launch_shape_of(int family) {
  SpmmLaunchShape s{};
  s.family = family;
  s.row_ok_offset = s.table_offset = s.partials_offset = -1;
  return s;
}

}  // namespace sputnik_hip
