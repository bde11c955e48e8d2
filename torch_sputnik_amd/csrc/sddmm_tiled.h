// What sddmm_tiled.hip and sddmm_flat.hip export to sddmm.hip and many_mask.hip: the only
// declaration of it (default arguments live here and nowhere else).
#pragma once

#include "common.h"

namespace sputnik_hip {

// One SDDMM call, float32 or half operands alike: what the host path hands on unchanged.
// A host-side convenience only -- the kernels keep their parameter lists.
struct SddmmArgs {
  int m, k, n, nonzeros, replicas;
  const int *row_indices, *row_offsets, *column_indices;
  const void* lhs;
  int64_t lhs_stride;
  const void* rhs;
  int64_t rhs_stride;
  void* out;
  int64_t out_stride;
  int in_type, out_type;     // SPUTNIK_HIP_F32 / F16 / BF16; out float32 or in_type
  void* workspace;
  size_t workspace_bytes;
  hipStream_t stream;
  int mask_heads;            // > 0: "many mask" (many_mask.hip), replica r under mask r / heads
  int64_t mask_plan_ints;    // ints between the plans of consecutive masks
};
inline int sddmm_elem_bytes(int type) { return type == SPUTNIK_HIP_F32 ? 4 : 2; }

// (the values are the SPUTNIK_HIP_SDDMM_* family codes of include/sputnik_hip.h; kMfma: the
// summed form's matrix-core route, sddmm_mfma.hip)
enum class SddmmKernel { kRowWave = 0, kFlat = 1, kQuad = 2, kStationary = 3, kMfma = 4 };

// What a call launches, as sputnik_hip_sddmm_launch_shape reports it (include/sputnik_hip.h):
// filled by the launch functions below INSTEAD of launching when they are handed one.
struct SddmmLaunchShape {
  SddmmKernel kernel;
  int panel_width, slab_rows, passes;
  bool accumulates;          // later passes run the instance that adds into the output
  int slabs, grid_y, grid_z, row_blocks;   // of the first launch (grid x = slabs)
};

// sddmm_tiled.hip.  `summed`: the form summed over the replicas (its panel width, hence
// its slabs and its chunk table, can differ from the plain product's).
bool sddmm_tiled_applicable(const SddmmArgs& a, int elem_bytes);
size_t sddmm_tiled_workspace_bytes(int m, int k, int n, int nonzeros, bool summed = false);
int sddmm_tiled_plan(const SddmmArgs& a, bool summed = false, bool with_flat = false, int masks = 1);
// Kernels only, on a planned workspace.  `flat`: the plan carries the pair-flat kernel's lists.
SddmmKernel sddmm_tiled_kernel(const SddmmArgs& a, bool flat);   // which one the launch runs
int sddmm_tiled_launch(const SddmmArgs& a, bool flat = false, SddmmLaunchShape* shape = nullptr);
// a.out: float [replicas * panels][nonzeros]
int sddmm_tiled_launch_partials(const SddmmArgs& a, SddmmLaunchShape* shape = nullptr);
int sddmm_tiled_panels(int m, int k, int n, int nonzeros);
int sddmm_tiled_panel_width(int k);
int sddmm_tiled_slab_rows(int k);                                  // of the plain product's plan
int sddmm_tiled_sum_slab_rows(int m, int k, int n, int nonzeros);  // of the summed form's plan
int sddmm_tiled_passes_half(int k);
bool sddmm_tiled_sum_half_served(int m, int k, int n, int nonzeros);

// Bytes between the plans of consecutive masks in a "many mask" workspace.
// (the last word of a region is spare: the masks' start order, mask_start_word)
inline size_t sddmm_many_mask_plan_bytes(int m, int k, int n, int nonzeros) {
  return (sddmm_tiled_workspace_bytes(m, k, n, nonzeros) + sizeof(int) + 255) / 256 * 256;
}

// sddmm_flat.hip: the pair-flat kernel for planned masks and rows of 128 / 256 bytes
bool sddmm_flat_applicable(int m, int k, int n, int nonzeros, int elem_bytes);
size_t sddmm_flat_plan_bytes(int m, int n, int nonzeros);
int sddmm_flat_plan(int m, int n, int nonzeros, const int* row_indices, const int* row_offsets,
                    const int* column_indices, void* plan, hipStream_t stream);
int sddmm_flat_launch(int m, int k, int n, int nonzeros, int replicas, const int* row_indices,
                      const void* lhs, int64_t lhs_stride, const void* rhs, int64_t rhs_stride,
                      void* out, int64_t out_stride, int in_type, int out_type, const void* plan,
                      hipStream_t stream);

}  // namespace sputnik_hip
