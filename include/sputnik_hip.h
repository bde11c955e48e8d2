/*
 * sputnik_hip.h -- C ABI of the MI355X (gfx950) sparse kernel library
 * (libsputnik_hip.so).
 *
 * This is the drop-in boundary for the device side of the torch_sputnik
 * operator surface.  Each entry point replaces one library call the
 * reference's host wrappers make (file:line below are in the reference
 * checkout); the host side above it (torch_sputnik_amd/csrc/torch_binding.cpp)
 * mirrors the reference's five operators, src/sputnik.cpp:36-42.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *     its name says otherwise; no torch types.
 *   - all launches are asynchronous on `stream`; no entry point synchronises,
 *     allocates or frees device memory, so calls can be captured into a
 *     hipGraph.  Scratch memory is passed in by the caller (query its size
 *     with the matching *_workspace_bytes function), in the way the reference
 *     drives cusparseCsr2cscEx2_bufferSize (src/transpose_cuda.cu:22-31).
 *   - return value: 0 on success, otherwise the hipError_t of the failed
 *     launch, or SPUTNIK_HIP_INVALID_ARGUMENT for a shape the library
 *     rejects.  (The reference returns cudaError_t and aborts on != success,
 *     include/error_check.h:5-10.)
 *   - fp32 values, int32 indices, row-major dense operands, zero-based CSR:
 *     exactly the reference's layout (src/spmm_cuda.cu:49-56).
 *   - every output element is written by the kernels (rows without nonzeros
 *     get zeros), so outputs need no memset (the reference zero-fills them
 *     first, src/spmm_cuda.cu:46).
 *   - `row_indices` is a permutation of [0,m) giving the order in which rows
 *     are dealt to workgroups (load balancing); results never depend on it.
 *   - batched entry points run all replicas in ONE launch; a stride is the
 *     element distance between consecutive replicas (0 = operand shared).
 */
#ifndef SPUTNIK_HIP_H_
#define SPUTNIK_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Opaque HIP stream handle (same type as hipStream_t in <hip/hip_runtime_api.h>). */
typedef struct ihipStream_t* sputnik_hip_stream_t;

#define SPUTNIK_HIP_INVALID_ARGUMENT (-1)
/* a fused entry point does not serve this shape / alignment: use the separate operators */
#define SPUTNIK_HIP_UNSUPPORTED (-2)

/* Exported-symbol marker (the library is built with -fvisibility=hidden). */
#define SPUTNIK_HIP_API __attribute__((visibility("default")))

/* Storage types of the *_typed entry points (round 3).  The reference is float32
 * only (data_ptr<float>(), src/spmm_cuda.cu:51); float16 / bfloat16 operands are an
 * extension (BASELINE.json config 5) that the kernels read and write directly --
 * all arithmetic stays float32. */
#define SPUTNIK_HIP_F32 0
#define SPUTNIK_HIP_F16 1
#define SPUTNIK_HIP_BF16 2

/* Library / build identification: "sputnik_hip <version> gfx950". */
SPUTNIK_HIP_API const char* sputnik_hip_version(void);

/* Hash of the kernel sources this library was built from (12 hex digits).  The
 * profiles under profiles/ record it, and bench.py quotes a PMC traffic figure
 * only when it was collected on the build that is running. */
SPUTNIK_HIP_API const char* sputnik_hip_build_id(void);

/* Name of the device kernel that serves an SpMM call of this shape (the
 * dispatcher's choice: spmm.hip, spmm_tiled.hip), e.g. "spmm_flat_kernel<0>"; for
 * benchmarks and profiles, which report the dominant kernel by name.  The
 * pointer is to a static string. */
SPUTNIK_HIP_API const char* sputnik_hip_spmm_kernel_name(int m, int k, int n, int nonzeros,
                                                         int replicas);
/* The same for sputnik_hip_spmm_typed, whose dispatch is its own (operands of values_type /
 * dense_type, SPUTNIK_HIP_F32 / F16 / BF16; values_stride 0: shared values), when the workspace
 * is as large as sputnik_hip_spmm_typed_workspace_bytes asks and the operands are aligned and
 * contiguous: "left_spmm_half_tiles" (the matrix cores), "spmm_panel64_kernel" and
 * "spmm_rowgather_kernel" (their half-reading forms), or the float32 kernel that runs on
 * widened copies; "none" for a pair of types the call refuses. */
SPUTNIK_HIP_API const char* sputnik_hip_spmm_typed_kernel_name(int m, int k, int n, int nonzeros,
                                                               int replicas, int values_type,
                                                               int64_t values_stride,
                                                               int dense_type);
/* Rows of the output tile sputnik_hip_left_spmm_half_tiles gives a workgroup for a call of
 * this shape under the current options: 128 or 256 (0: nothing to launch).  Host only. */
SPUTNIK_HIP_API int sputnik_hip_left_spmm_half_tiles_tile_rows(int m, int n, int replicas);
/* The same for an SDDMM call (sddmm.hip, sddmm_tiled.hip, sddmm_flat.hip): operands of
 * `elem_bytes` (4: float32, 2: float16 / bfloat16), `planned` != 0 for a product on a
 * workspace that sputnik_hip_sddmm_plan filled ("sddmm_flat_kernel", "sddmm_quad_kernel",
 * "sddmm_stationary_kernel", "sddmm_rowwave_kernel"). */
SPUTNIK_HIP_API const char* sputnik_hip_sddmm_kernel_name(int m, int k, int n, int nonzeros,
                                                          int replicas, int elem_bytes,
                                                          int planned);
/* The route a SUMMED SDDMM call of this shape takes (sputnik_hip_sddmm_sum_batched / _typed /
 * _mixed and their planned forms) under the current options, when the workspace and the
 * scratch buffer are as large as the size queries ask and the operands are 16-byte aligned:
 * operands stored as `in_type` (SPUTNIK_HIP_F32 / F16 / BF16); `mixed` != 0: a (float32,
 * half) pair whose half operand has `in_type`; `planned` != 0: on a workspace that
 * sputnik_hip_sddmm_sum_plan filled.
 *   kernel       SPUTNIK_HIP_SUM_ROWWAVE: the row-wave kernel writes one partial vector per
 *                replica; _TILED: the rhs-stationary (float32) / quad (half) kernel writes one
 *                per (replica, panel); _MFMA: the matrix-core kernel; _PLAIN: one replica of
 *                one panel, nothing to sum -- the plain product (sputnik_hip_sddmm_kernel_name
 *                for one replica, not planned, names its kernel when panel_width != 0; the
 *                row-wave kernel otherwise)
 *   panel_width  columns of k per panel (_TILED, _PLAIN on the LDS kernels; 0 otherwise)
 *   panels       k / panel_width (1 otherwise)
 *   slab_rows    rows of rhs per slab (_TILED, _PLAIN), rows of the output tile (_MFMA)
 *   splits       workgroups that share an output tile (_MFMA; 1 otherwise)
 * Host only, launches nothing; any output pointer may be NULL.  Returns
 * SPUTNIK_HIP_INVALID_ARGUMENT for a call that launches nothing or an unknown type,
 * SPUTNIK_HIP_UNSUPPORTED for a mixed pair the matrix-core route does not serve.  For tests,
 * which assert the route they mean to reach. */
#define SPUTNIK_HIP_SUM_ROWWAVE 0
#define SPUTNIK_HIP_SUM_TILED 1
#define SPUTNIK_HIP_SUM_MFMA 2
#define SPUTNIK_HIP_SUM_PLAIN 3
SPUTNIK_HIP_API int sputnik_hip_sddmm_sum_route(int m, int k, int n, int nonzeros, int replicas,
                                                int in_type, int planned, int mixed, int* kernel,
                                                int* panel_width, int* panels, int* slab_rows,
                                                int* splits);
/* What an SDDMM call of this shape launches under the current options, down to the kernel
 * instance and its grid, when the workspace (and the summed form's scratch) are as large as
 * the size queries ask and the operands are 16-byte aligned and contiguous: operands stored as
 * `in_type`, output as `out_type` (SPUTNIK_HIP_F32 / F16 / BF16; float32 or in_type);
 * `planned` != 0: on a workspace that sputnik_hip_sddmm_plan / _sum_plan filled; `summed` != 0:
 * the summed form (sputnik_hip_sddmm_sum_batched / _typed; out_type float32), whose launch of
 * the partial products is described; `mask_heads` > 0: a sputnik_hip_sddmm_many_mask call of
 * replicas / mask_heads masks, `nonzeros` the largest mask's count (float32, not summed).
 *   family       SPUTNIK_HIP_SDDMM_ROWWAVE / _FLAT / _QUAD / _STATIONARY, or _MFMA (the summed
 *                form's matrix-core route)
 *   panel_width  columns of k a launch works on (_QUAD, _STATIONARY; _FLAT: k; 0 otherwise)
 *   slab_rows    rows of rhs per slab (_QUAD, _STATIONARY; _MFMA: rows of the output tile)
 *   passes       launches per replica slice, one panel each (1 for the summed form, whose
 *                panels lie side by side on grid z)
 *   accumulates  1: passes after the first run the instance that adds into the output
 *   grid_x, grid_y, grid_z   of the first launch (_QUAD, _STATIONARY; 0 otherwise): slabs, the
 *                row blocks of 256 rows a launch spreads over y, replicas (summed: replicas *
 *                panels)
 *   row_blocks   ceil(m / 256): with grid_y < row_blocks a workgroup walks several row blocks
 * The call runs the launch path itself and launches nothing; any output pointer may be NULL.
 * Returns SPUTNIK_HIP_INVALID_ARGUMENT for a call that launches nothing or for types no entry
 * point accepts, SPUTNIK_HIP_UNSUPPORTED where the call itself would.  For tests, which assert
 * the instance and the grid they mean to reach. */
#define SPUTNIK_HIP_SDDMM_ROWWAVE 0
#define SPUTNIK_HIP_SDDMM_FLAT 1
#define SPUTNIK_HIP_SDDMM_QUAD 2
#define SPUTNIK_HIP_SDDMM_STATIONARY 3
#define SPUTNIK_HIP_SDDMM_MFMA 4
SPUTNIK_HIP_API int sputnik_hip_sddmm_launch_shape(int m, int k, int n, int nonzeros, int replicas,
                                                   int in_type, int out_type, int planned,
                                                   int summed, int mask_heads, int* family,
                                                   int* panel_width, int* slab_rows, int* passes,
                                                   int* accumulates, int* grid_x, int* grid_y,
                                                   int* grid_z, int* row_blocks);
/* What a float32 SpMM call of this shape (sputnik_hip_spmm_batched / _bias_batched /
 * _batched_planned) launches under the current options, down to the kernel instance, its grid
 * and where its tables lie in the workspace -- when the workspace is as large as
 * sputnik_hip_spmm_workspace_bytes asks and 16-byte aligned, the dense operand is 16-byte
 * aligned, the replica strides are multiples of four elements, and `out` is aligned to
 * `out_alignment` bytes (a power of two from 4; 16 and more: every kernel's rule is met; less:
 * the 256- / 512-column and the panel kernel are not taken, and the 64-column kernel runs
 * without its K split).
 *   family          SPUTNIK_HIP_SPMM_ROWGATHER / _PANEL / _NARROW64 (spmm_tiled64_kernel) /
 *                   _WIDE256 / _WIDE512 (spmm_tiled_kernel on 256- / 512-column tiles) / _FLAT
 * For _NARROW64, _WIDE256 and _WIDE512 (0, offsets -1, for the other families):
 *   tile_cols, tile_rows        the tile of the output a workgroup owns
 *   waves, rows_per_wave        of a workgroup; tile_rows = waves * rows_per_wave
 *   chunk                       rows of the dense operand per LDS stage
 *   sparse, batch               1 and 4 / 8: the short-segment form and the entries of one of its
 *                               LDS round trips; 0 and 0: the long-segment form (_NARROW64: 0, 0)
 *   grid_x, grid_y              of the product's launch (_NARROW64: grid_x counts the K splits)
 *   slots, nchunks, n_tiles     row slots of the chunk table, K chunks, column tiles
 *   ksplits                     workgroups that share a tile's K walk (_NARROW64; 1: no split,
 *                               no sum kernel)
 *   workspace_bytes             sputnik_hip_spmm_workspace_bytes(m, k, n, nonzeros)
 *   row_ok_offset, table_offset, partials_offset
 *                               bytes from the workspace's start to this kernel's row order
 *                               words, its chunk table [nchunks + 1][slots] and the partial tiles
 *                               [ksplits][m][n] of a K split (-1: none).  The layout depends on
 *                               the shape and the options alone: a workspace that
 *                               sputnik_hip_spmm_plan filled (replica count unknown: the tables
 *                               of every kernel a later call may take, side by side) and one
 *                               that the call fills for itself hold this kernel's tables at the
 *                               same offsets.  (_FLAT: table_offset is where its plan starts.)
 * The call runs the launch path itself and launches nothing; `launch` may be NULL.  Returns
 * SPUTNIK_HIP_INVALID_ARGUMENT for a call that launches nothing (m, k, n or replicas < 1) or an
 * out_alignment that is no power of two from 4.  For tests, which assert the instance they mean
 * to reach. */
#define SPUTNIK_HIP_SPMM_ROWGATHER 0
#define SPUTNIK_HIP_SPMM_PANEL 1
#define SPUTNIK_HIP_SPMM_NARROW64 2
#define SPUTNIK_HIP_SPMM_WIDE256 3
#define SPUTNIK_HIP_SPMM_WIDE512 4
#define SPUTNIK_HIP_SPMM_FLAT 5
typedef struct sputnik_hip_spmm_launch {
  int family;
  int tile_cols, tile_rows, waves, rows_per_wave, chunk;
  int sparse, batch;
  int grid_x, grid_y;
  int slots, nchunks, n_tiles;
  int ksplits;
  int64_t workspace_bytes, row_ok_offset, table_offset, partials_offset;
} sputnik_hip_spmm_launch;
SPUTNIK_HIP_API int sputnik_hip_spmm_launch_shape(int m, int k, int n, int nonzeros, int replicas,
                                                  int out_alignment,
                                                  sputnik_hip_spmm_launch* launch);
/* The instance of the sparse softmax kernel (softmax.hip) that a call of this shape launches
 * for its first grid slice under the current options: values stored as `dtype`
 * (SPUTNIK_HIP_F32 / F16 / BF16), `backward` != 0 for the gradient.  The class is
 * `lanes_per_row` lanes per row with `base_pieces` 16-byte pieces per lane always worked on
 * and `pieces` at the most; `rows_per_group` consecutive rows per lane group, `depth` rows in
 * flight ahead, `nontemporal` 0 none / 1 loads / 2 stores / 3 both.  Host only, launches
 * nothing; any output pointer may be NULL.  Returns SPUTNIK_HIP_INVALID_ARGUMENT for a call
 * that launches nothing (m, nonzeros or replicas < 1) or an unknown dtype.  For tests, which
 * assert the instance they mean to reach. */
SPUTNIK_HIP_API int sputnik_hip_sparse_softmax_route(int m, int nonzeros, int replicas, int dtype,
                                                     int backward, int* lanes_per_row,
                                                     int* base_pieces, int* pieces,
                                                     int* rows_per_group, int* depth,
                                                     int* nontemporal);

/* ------------------------------------------------------------------------
 * SpMM   C[m,n] = A_csr[m,k] * B[k,n]
 * replaces sputnik::CudaSpmm(m,k,n,nnz,row_indices,values,row_offsets,
 *          column_indices,dense,out,stream)          src/spmm_cuda.cu:49-56
 * ---------------------------------------------------------------------- */
SPUTNIK_HIP_API int sputnik_hip_spmm(int m, int k, int n, int nonzeros,
                     const int* row_indices, const float* values,
                     const int* row_offsets, const int* column_indices,
                     const float* dense, float* out,
                     sputnik_hip_stream_t stream);

/*
 * Batched SpMM, one launch for all replicas.  Replaces the host loops
 *   src/spmm_cuda.cu:48-57               (values_stride = nonzeros)
 *   src/left_replicated_spmm.cu:32-41    (values_stride = 0: shared weights)
 * dense_stride is normally k*n and out_stride m*n.
 * `workspace` may be NULL (then only the workspace-free kernels are used);
 * otherwise it must hold sputnik_hip_spmm_workspace_bytes(m,k,n,nonzeros).
 */
SPUTNIK_HIP_API size_t sputnik_hip_spmm_workspace_bytes(int m, int k, int n, int nonzeros);

SPUTNIK_HIP_API int sputnik_hip_spmm_batched(int m, int k, int n, int nonzeros, int replicas,
                             const int* row_indices, const float* values,
                             int64_t values_stride, const int* row_offsets,
                             const int* column_indices, const float* dense,
                             int64_t dense_stride, float* out,
                             int64_t out_stride, void* workspace,
                             size_t workspace_bytes,
                             sputnik_hip_stream_t stream);

/*
 * The same in two steps, for callers whose sparsity pattern is static (layer
 * weights, attention masks): `plan` runs the topology-only pre-pass into the
 * workspace once, `batched_planned` may then be called any number of times
 * with that workspace (values, dense and out may change between calls; the
 * three index arrays, m, k and n may not).  No counterpart in the reference,
 * which re-derives everything per call (src/spmm_cuda.cu:48-57).
 * A planned workspace is also the call's SCRATCH (a single product against a narrow dense
 * operand keeps the partial tiles of its K split there): calls that share one workspace
 * must be ordered on one stream; concurrent streams take a workspace each (the plan is
 * topology only: `plan` may be run into any number of them).
 */
/* (Round 4) A single product against a narrow dense operand (n < 512, k >= 2048, one
 * replica) deals its K chunks to several workgroups per tile; their partial tiles live in
 * the workspace (sputnik_hip_spmm_workspace_bytes counts them) and are scratch of the
 * call: one workspace, planned or not, serves one stream at a time for such a shape. */
SPUTNIK_HIP_API int sputnik_hip_spmm_plan(int m, int k, int n, int nonzeros,
                          const int* row_indices, const int* row_offsets,
                          const int* column_indices, void* workspace,
                          size_t workspace_bytes, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_spmm_batched_planned(int m, int k, int n, int nonzeros,
                             int replicas, const int* row_indices,
                             const float* values, int64_t values_stride,
                             const int* row_offsets, const int* column_indices,
                             const float* dense, int64_t dense_stride, float* out,
                             int64_t out_stride, const void* workspace,
                             size_t workspace_bytes, sputnik_hip_stream_t stream);

/* ------------------------------------------------------------------------
 * SDDMM  out[p] = < lhs[i_p, 0:k], rhs[j_p, 0:k] >  for each stored (i_p,j_p)
 * lhs is [m,k], rhs is [n,k] (row-major, i.e. already "transposed").
 * replaces sputnik::CudaSddmm(m,k,n,nnz,row_indices,row_offsets,
 *          column_indices,lhs,rhs,out,stream)       src/sddmm_cuda.cu:46-53
 * and the host loop src/sddmm_cuda.cu:45-54 (batched form).
 * ---------------------------------------------------------------------- */
SPUTNIK_HIP_API int sputnik_hip_sddmm(int m, int k, int n, int nonzeros,
                      const int* row_indices, const int* row_offsets,
                      const int* column_indices, const float* lhs,
                      const float* rhs, float* out,
                      sputnik_hip_stream_t stream);

/* `workspace` may be NULL (workspace-free kernel only); otherwise it must hold
 * sputnik_hip_sddmm_workspace_bytes(m,k,n,nonzeros) (0 = none needed). */
SPUTNIK_HIP_API size_t sputnik_hip_sddmm_workspace_bytes(int m, int k, int n, int nonzeros);

SPUTNIK_HIP_API int sputnik_hip_sddmm_batched(int m, int k, int n, int nonzeros, int replicas,
                              const int* row_indices, const int* row_offsets,
                              const int* column_indices, const float* lhs,
                              int64_t lhs_stride, const float* rhs,
                              int64_t rhs_stride, float* out,
                              int64_t out_stride, void* workspace,
                              size_t workspace_bytes, sputnik_hip_stream_t stream);

/* Two-step form for static masks (as sputnik_hip_spmm_plan): `plan` runs the
 * topology-only pre-pass into the workspace once, `batched_planned` reuses it.
 * No counterpart in the reference (src/sddmm_cuda.cu:45-54 re-derives per call). */
SPUTNIK_HIP_API int sputnik_hip_sddmm_plan(int m, int k, int n, int nonzeros,
                              const int* row_indices, const int* row_offsets,
                              const int* column_indices, void* workspace,
                              size_t workspace_bytes, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sddmm_batched_planned(int m, int k, int n, int nonzeros,
                              int replicas, const int* row_indices, const int* row_offsets,
                              const int* column_indices, const float* lhs,
                              int64_t lhs_stride, const float* rhs, int64_t rhs_stride,
                              float* out, int64_t out_stride, const void* workspace,
                              size_t workspace_bytes, sputnik_hip_stream_t stream);

/*
 * SDDMM on operands stored as `in_type` (SPUTNIK_HIP_F32 / F16 / BF16; lhs and rhs
 * alike; strides in elements), output stored as `out_type` (F32, or in_type).  Half
 * operands are read as they are -- the LDS slab of rhs rows holds half values (half
 * the staging and half the LDS traffic of the float form), products are exact
 * (v_dot2_f32_f16 / _bf16), sums float32 -- where src/sddmm_cuda.cu:48-53 knows float
 * only.  workspace / planned as sputnik_hip_sddmm_batched{,_planned} (same size, same
 * plan: it does not depend on the types).  Returns SPUTNIK_HIP_UNSUPPORTED for a half
 * OUTPUT whose product needs more than one pass over the output (k wider than one
 * panel): take a float output then.
 */
/*
 * SpMM / left_spmm (values_stride = 0) with operands stored as float32, float16 or
 * bfloat16 -- values and dense independently, a half pair of ONE kind -- product
 * float32, optional bias / ReLU epilogue as sputnik_hip_spmm_bias_batched.  Half
 * operands are read as they are (src/spmm_cuda.cu:42,51 knows float only): the
 * panel-resident kernel widens the rows of B on their way into LDS (half the bytes
 * from memory, same compute loop) and serves up to two panels (k <= 1024) with
 * n >= 64; larger products, where the chunked float kernels win by a factor of two,
 * are widened into the workspace by one pass inside this call when the workspace has
 * sputnik_hip_spmm_typed_workspace_bytes; everything else (and every call without
 * that room) takes the row-gather kernel, which reads half rows of B from L2.
 */
SPUTNIK_HIP_API size_t sputnik_hip_spmm_typed_workspace_bytes(int m, int k, int n, int nonzeros,
                              int replicas, int values_type, int64_t values_stride,
                              int dense_type);
SPUTNIK_HIP_API int sputnik_hip_spmm_typed(int m, int k, int n, int nonzeros, int replicas,
                              const int* row_indices, const void* values, int values_type,
                              int64_t values_stride, const int* row_offsets,
                              const int* column_indices, const void* dense, int dense_type,
                              int64_t dense_stride, const float* bias, int relu, float* out,
                              int64_t out_stride, void* workspace, size_t workspace_bytes,
                              sputnik_hip_stream_t stream);

/*
 * left_spmm (values shared by the replicas: src/left_replicated_spmm.cu:32-41) as a DENSE
 * contraction on the matrix cores, for the half-storage extension (round 5,
 * csrc/spmm_mfma.hip): the CSR values are scattered into a zeroed [m, k] image of
 * `tile_type` (SPUTNIK_HIP_F16 / BF16) and multiplied against the dense operand
 * [replicas][k][n] on v_mfma_f32_32x32x16 tiles, float32 sums, float32 product with the
 * bias / ReLU epilogue of sputnik_hip_spmm_bias_batched.  At layer densities every tile of
 * the weight is occupied, and the tiles cost 1 / density times the sparse flops on a unit
 * sixteen times faster than the vector pipe.  An operand given as float32 (values_type /
 * dense_type = SPUTNIK_HIP_F32; the other, if half, has type tile_type) is not rounded to the
 * tile type: it enters as half planes whose sum is the value, at one more tile product per
 * plane pair
 * (float16: two planes of the operand times a power of two taken on the device from its
 * largest finite magnitude and undone exactly in the epilogue -- at least 22 bits of every
 * value down to 2^-28 of that magnitude, an absolute error below 2^-50 of it beneath, over
 * float32's whole range; an inf / NaN element stays non-finite (inf may come out as NaN)
 * and leaves the others' range alone.  bfloat16: three planes, 24 bits.)  The workspace
 * holds the planes and, for float16, their range.  sputnik_hip_spmm_typed takes this route
 * by itself for a half dense operand; this entry adds the float32 dense operand (the incoming
 * gradient of modules/sparse_linear.py:60-65 in a half-storage layer).
 * Returns SPUTNIK_HIP_UNSUPPORTED where the route does not serve the call (k not a
 * multiple of 64, n not of 8, a grid under 192 tiles, density under 0.06 per tile
 * product, too little workspace, ...): take sputnik_hip_spmm_typed / _batched then.
 * The float32 operators never come here.
 */
SPUTNIK_HIP_API size_t sputnik_hip_left_spmm_half_tiles_workspace_bytes(int m, int k, int n,
                              int nonzeros, int replicas, int values_type, int dense_type,
                              int tile_type);
SPUTNIK_HIP_API int sputnik_hip_left_spmm_half_tiles(int m, int k, int n, int nonzeros, int replicas,
                              const int* row_offsets, const int* column_indices,
                              const void* values, int values_type, const void* dense,
                              int dense_type, int64_t dense_stride, int tile_type,
                              const float* bias, int relu, float* out, int64_t out_stride,
                              void* workspace, size_t workspace_bytes,
                              sputnik_hip_stream_t stream);

/*
 * A sparse layer on half-stored activations, all three products on the matrix cores with NO
 * layout pass (round 5, csrc/sparse_linear_half.hip, csrc/mfma_gemm.h).  The reference's
 * SparseLinear runs x.transpose(1, 2).contiguous() in front of left_spmm and the
 * transposes back behind it (modules/sparse_linear.py:28,44-65,89); the tile kernel reads
 * every operand in the layout the caller has it:
 *   forward          y[b][o][s]  = sum_i W[o][i] x[b][s][i]            y float32 [batch, out, seq]
 *   weight gradient  dW[p]       = sum_b sum_s dy[b][o_p][s] x[b][s][i_p]   float32 [nonzeros]
 *   input gradient   dx[b][s][i] = sum_o dy[b][o][s] W[o][i]           [batch, seq, in], float32 or tile type
 * x [batch, seq, in] in `tile_type` (SPUTNIK_HIP_F16 / BF16).  W is given as its IMAGE: the
 * CSR values (float32 or tile_type) scattered into a zeroed [planes][out][in] array of the
 * tile type -- sputnik_hip_sparse_linear_half_image, one launch per step, shared
 * by the forward pass and the input gradient.  dy [batch, out, seq] is given either in the
 * tile type (grad_type = tile_type) or as the PLANES of the float32 tensor
 * (sputnik_hip_half_planes, grad_type = SPUTNIK_HIP_F32): float32 operands are not rounded
 * to the storage type -- they enter as half planes whose sum is the value
 * (float16: two planes of the operand times a power of two taken on the device from its
 * largest finite magnitude and undone exactly in the epilogue -- at least 22 bits of every
 * value down to 2^-28 of that magnitude, an absolute error below 2^-50 of it beneath, over
 * float32's whole range; an inf / NaN element stays non-finite (inf may come out as NaN)
 * and leaves the others' range alone.  bfloat16: three planes, 24 bits.)
 * The image and the planes (sputnik_hip_sparse_linear_half_image_bytes,
 * sputnik_hip_half_planes_bytes) carry that power of two behind the planes.  The weight gradient takes a plan
 * (sputnik_hip_sparse_linear_half_plan, topology only, may be NULL) and scratch for the
 * partial vectors of the workgroups that share a tile.
 * sputnik_hip_sparse_linear_half_supported: 1 where the three products take this route
 * (out, in, seq multiples of 64, a grid of at least 192 tiles, density from 0.06 per plane of
 * the values); an entry point returns SPUTNIK_HIP_UNSUPPORTED for a call it does not serve
 * (bfloat16 tiles with BOTH float32 values and a float32 dy in the input gradient: nine
 * plane pairs) -- use the typed operators then.  The float32 operators never come here.
 */
SPUTNIK_HIP_API int sputnik_hip_sparse_linear_half_supported(int out_features, int in_features, int seq,
                              int batch, int nonzeros, int values_type, int tile_type);
SPUTNIK_HIP_API size_t sputnik_hip_sparse_linear_half_image_bytes(int out_features, int in_features,
                              int values_type, int tile_type);
SPUTNIK_HIP_API int sputnik_hip_sparse_linear_half_image(int out_features, int in_features, int nonzeros,
                              const int* row_offsets, const int* column_indices, const void* values,
                              int values_type, int tile_type, void* image, size_t image_bytes,
                              sputnik_hip_stream_t stream);
SPUTNIK_HIP_API size_t sputnik_hip_half_planes_bytes(int64_t count, int tile_type);
SPUTNIK_HIP_API int sputnik_hip_half_planes(int64_t count, const float* in, int tile_type, void* planes,
                              sputnik_hip_stream_t stream);
SPUTNIK_HIP_API int sputnik_hip_sparse_linear_half_forward(int out_features, int in_features, int seq,
                              int batch, const void* image, int values_type, const void* x,
                              int tile_type, const float* bias, int relu, float* y,
                              sputnik_hip_stream_t stream);
SPUTNIK_HIP_API size_t sputnik_hip_sparse_linear_half_plan_bytes(int out_features, int in_features);
SPUTNIK_HIP_API int sputnik_hip_sparse_linear_half_plan(int out_features, int in_features,
                              const int* row_offsets, const int* column_indices, void* plan,
                              sputnik_hip_stream_t stream);
SPUTNIK_HIP_API size_t sputnik_hip_sparse_linear_half_scratch_bytes(int out_features, int in_features,
                              int seq, int batch, int nonzeros, int grad_type, int tile_type);
SPUTNIK_HIP_API int sputnik_hip_sparse_linear_half_weight_gradient(int out_features, int in_features,
                              int seq, int batch, int nonzeros, const int* row_offsets,
                              const int* column_indices, const void* grad_output, int grad_type,
                              const void* x, int tile_type, float* grad_values, const void* plan,
                              void* scratch, size_t scratch_bytes, sputnik_hip_stream_t stream);
SPUTNIK_HIP_API int sputnik_hip_sparse_linear_half_input_gradient(int out_features, int in_features,
                              int seq, int batch, const void* grad_output, int grad_type,
                              const void* image, int values_type, int tile_type, void* grad_input,
                              int grad_input_type, sputnik_hip_stream_t stream);

/*
 * The DENSE weight gradient of the layer (RigL's grow scores):
 *   dense_grad[o][i] = sum_b sum_s dy[b][o][s] x[b][s][i]     float32, row stride dense_ld
 * sputnik_hip_sparse_linear_half_weight_gradient_dense is the weight gradient above with a
 * second output: the sampled epilogue holds the whole 128 x 128 float32 tile in LDS and
 * stores the entries under the mask; here the tile is stored as well, so ONE launch gives
 * grad_values[nonzeros] and dense_grad[out, in], and grad_values[p] equals the image element
 * at entry p's (row, column) bit for bit.  Arguments and conditions as the weight gradient's
 * (seq a multiple of 64, in a multiple of 8, 16-byte aligned operands), and dense_grad
 * 16-byte aligned with dense_ld a multiple of 4, at least in_features.  Always one workgroup
 * per tile (a tile shared by several would need a partial image per split): no scratch.
 * Only elements with o < out_features and i < in_features are written.
 *
 * sputnik_hip_sparse_linear_dense_weight_gradient is the standalone form -- no mask, nothing
 * sampled -- for layers off the tile route and float32 layers.  grad_type and x_type are
 * each tile_type (the tensor itself) or SPUTNIK_HIP_F32 (the PLANES of the float32 tensor,
 * sputnik_hip_half_planes over the whole tensor).  x_layout: SPUTNIK_HIP_X_BSI, x
 * [batch, seq, in] (as the half layer has it), or SPUTNIK_HIP_X_BIS, x [batch, in, seq] (the
 * k-major operand of left_spmm).  Served (.._supported, host only, 1 / 0): seq a multiple of
 * 64, in a multiple of 8, out * in, out * seq and in * seq below 2^30, any density;
 * float16 tiles with any pair of operand types, bfloat16 tiles with at most one float32
 * operand (nine plane pairs are not built: SPUTNIK_HIP_UNSUPPORTED).  Operands 16-byte
 * aligned.  Neither form accumulates into dense_grad.
 */
#define SPUTNIK_HIP_X_BSI 0
#define SPUTNIK_HIP_X_BIS 1
SPUTNIK_HIP_API int sputnik_hip_sparse_linear_half_weight_gradient_dense(int out_features, int in_features,
                              int seq, int batch, int nonzeros, const int* row_offsets,
                              const int* column_indices, const void* grad_output, int grad_type,
                              const void* x, int tile_type, float* grad_values, const void* plan,
                              float* dense_grad, int64_t dense_ld, sputnik_hip_stream_t stream);
SPUTNIK_HIP_API int sputnik_hip_sparse_linear_dense_weight_gradient_supported(int out_features,
                              int in_features, int seq, int batch, int grad_type, int x_type,
                              int x_layout, int tile_type);
SPUTNIK_HIP_API int sputnik_hip_sparse_linear_dense_weight_gradient(int out_features, int in_features,
                              int seq, int batch, const void* grad_output, int grad_type,
                              const void* x, int x_type, int x_layout, int tile_type,
                              float* dense_grad, int64_t dense_ld, sputnik_hip_stream_t stream);

/*
 * The same layer's forward pass in ROW orientation, the layout attention wants:
 *   y[b][s][o] = sum_i x[b][s][i] W[o][i]
 * x: element (b, s, i) at x + b * x_batch_stride + s * x_row_stride + i, in `tile_type`;
 * y: element (b, s, o) at y + b * y_batch_stride + s * y_row_stride + o, stored as
 * `y_type` (SPUTNIK_HIP_F32 or tile_type) -- e.g. one third of a [batch, seq, 3 * out]
 * buffer.  W is the IMAGE of sputnik_hip_sparse_linear_half_image (it is this call's
 * workspace and plan; float32 values enter as its planes, their range shift undone in the
 * epilogue).  sputnik_hip_sparse_linear_half_rows_supported answers as
 * sputnik_hip_sparse_linear_half_supported (the same tiles, transposed); the forward
 * returns SPUTNIK_HIP_UNSUPPORTED for a call it does not serve (in not a multiple of 64,
 * x not 16-byte aligned or its strides not multiples of 8 elements, a row stride of
 * 2^24 elements or more) -- use the typed operators then.
 */
SPUTNIK_HIP_API int sputnik_hip_sparse_linear_half_rows_supported(int out_features, int in_features,
                              int seq, int batch, int nonzeros, int values_type, int tile_type);
SPUTNIK_HIP_API int sputnik_hip_sparse_linear_half_rows_forward(int out_features, int in_features,
                              int seq, int batch, const void* image, int values_type, const void* x,
                              int64_t x_batch_stride, int64_t x_row_stride, int tile_type, void* y,
                              int y_type, int64_t y_batch_stride, int64_t y_row_stride,
                              sputnik_hip_stream_t stream);

/* sum over the replicas (sputnik_hip_sddmm_sum_batched{,_planned}) on operands stored as
 * `in_type`; the partial vectors and the result are float32.  Workspace / scratch sizes as
 * the float form's (sputnik_hip_sddmm_sum_workspace_bytes / _scratch_bytes).
 * Round 5: half operands with a long reduction (replicas * k >= 1024) over a mask of
 * density >= 0.05 (m, n >= 128, k a multiple of 64) take the MATRIX CORES
 * (csrc/sddmm_mfma.hip): the product is then a sampled dense contraction -- every 128 x 128
 * tile of the mask is occupied -- and the half products are exact in float32 either way.
 * The float32 form stays on the vector kernels. */
SPUTNIK_HIP_API int sputnik_hip_sddmm_sum_typed(int m, int k, int n, int nonzeros, int replicas,
                              const int* row_indices, const int* row_offsets,
                              const int* column_indices, const void* lhs, int64_t lhs_stride,
                              const void* rhs, int64_t rhs_stride, int in_type, float* out,
                              void* workspace, size_t workspace_bytes, int planned,
                              void* scratch, size_t scratch_bytes, sputnik_hip_stream_t stream);

/* The same for a (float32, half) pair of operands -- the weight gradient of a layer whose
 * activations are stored in half precision while the incoming gradient is float32
 * (modules/sparse_linear.py:44-49 with the extension's storage types).  Where the
 * matrix-core route serves the shape (long reduction, mask density from 0.05: the dense
 * 128 x 128 tiles on v_mfma_f32_32x32x16_{f16,bf16}, sampled at the mask) the float32
 * operand is not rounded to the storage type: one pass splits it into half planes,
 * v = hi + lo, and the tiles accumulate hi * x + lo * x (exact products, float32 sums)
 * (float16: two planes of the operand times a power of two taken on the device from its
 * largest finite magnitude and undone exactly in the epilogue -- at least 22 bits of every
 * value down to 2^-28 of that magnitude, an absolute error below 2^-50 of it beneath, over
 * float32's whole range; an inf / NaN element stays non-finite (inf may come out as NaN)
 * and leaves the others' range alone.  bfloat16: three planes, 24 bits).
 * `scratch` holds sputnik_hip_sddmm_sum_mixed_scratch_bytes(...) bytes (the planes, then the
 * partial vectors); workspace / planned as sputnik_hip_sddmm_sum_typed.  Returns
 * SPUTNIK_HIP_UNSUPPORTED for every other shape and for a float32 operand whose replicas do
 * not lie back to back: widen the half operand and take sputnik_hip_sddmm_sum_typed then.
 * lhs_type == rhs_type is sputnik_hip_sddmm_sum_typed itself. */
SPUTNIK_HIP_API size_t sputnik_hip_sddmm_sum_mixed_scratch_bytes(int m, int k, int n, int nonzeros,
                              int replicas, int lhs_type, int rhs_type);
SPUTNIK_HIP_API int sputnik_hip_sddmm_sum_mixed(int m, int k, int n, int nonzeros, int replicas,
                              const int* row_indices, const int* row_offsets,
                              const int* column_indices, const void* lhs, int lhs_type,
                              int64_t lhs_stride, const void* rhs, int rhs_type,
                              int64_t rhs_stride, float* out, void* workspace,
                              size_t workspace_bytes, int planned, void* scratch,
                              size_t scratch_bytes, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sddmm_typed(int m, int k, int n, int nonzeros, int replicas,
                              const int* row_indices, const int* row_offsets,
                              const int* column_indices, const void* lhs, int64_t lhs_stride,
                              const void* rhs, int64_t rhs_stride, int in_type, void* out,
                              int64_t out_stride, int out_type, void* workspace,
                              size_t workspace_bytes, int planned, sputnik_hip_stream_t stream);

/* Sum of the replicas' products, out[nonzeros] = sum_r sddmm(lhs_r, rhs_r): the
 * gradient of sparse values shared by a batch.  The reference returns the
 * [replicas, nonzeros] products (tests/test_linear_3d.py:64-69,
 * tests/test_left_spmm.py:57-64) and leaves the sum over the batch to autograd;
 * here the (replica, k-panel) pairs of the tiled kernel run in ONE launch into
 * `scratch` and a second kernel adds them up in index order (deterministic).
 * `scratch` holds sputnik_hip_sddmm_sum_scratch_bytes(...) bytes (0: not
 * needed), 16-byte aligned.  `workspace` holds
 * sputnik_hip_sddmm_sum_workspace_bytes(...) bytes; the planned form takes one
 * that sputnik_hip_sddmm_sum_plan filled -- NOT a plan of sputnik_hip_sddmm_plan:
 * with its panels side by side the summed product may cut k (and with it the
 * mask's column slabs) differently from the plain one. */
SPUTNIK_HIP_API size_t sputnik_hip_sddmm_sum_workspace_bytes(int m, int k, int n, int nonzeros);

SPUTNIK_HIP_API int sputnik_hip_sddmm_sum_plan(int m, int k, int n, int nonzeros,
                              const int* row_indices, const int* row_offsets,
                              const int* column_indices, void* workspace,
                              size_t workspace_bytes, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API size_t sputnik_hip_sddmm_sum_scratch_bytes(int m, int k, int n, int nonzeros,
                                                           int replicas);

SPUTNIK_HIP_API int sputnik_hip_sddmm_sum_batched(int m, int k, int n, int nonzeros,
                              int replicas, const int* row_indices, const int* row_offsets,
                              const int* column_indices, const float* lhs,
                              int64_t lhs_stride, const float* rhs, int64_t rhs_stride,
                              float* out, void* workspace, size_t workspace_bytes,
                              void* scratch, size_t scratch_bytes,
                              sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sddmm_sum_batched_planned(int m, int k, int n, int nonzeros,
                              int replicas, const int* row_indices, const int* row_offsets,
                              const int* column_indices, const float* lhs,
                              int64_t lhs_stride, const float* rhs, int64_t rhs_stride,
                              float* out, const void* workspace, size_t workspace_bytes,
                              void* scratch, size_t scratch_bytes,
                              sputnik_hip_stream_t stream);

/* Up to four summed SDDMMs of ONE shape (m, k, n), replica count and operand strides in
 * one call -- the weight gradients of a group of projections that share their input
 * (modules/sparse_attention.py:108-110: dW_q, dW_k, dW_v = dY_q, dY_k, dY_v against the same
 * x): each problem runs as sputnik_hip_sddmm_sum_batched_planned does, its own planned
 * workspace and scratch, and ONE launch adds the partial vectors of all of them (a sum is
 * four microseconds of launch and little else).  Results are those of the single calls,
 * bit for bit. */
typedef struct sputnik_hip_sddmm_sum_problem {
  const int* row_indices;
  const int* row_offsets;
  const int* column_indices;
  const float* lhs;        /* [replicas][m][k] */
  const float* rhs;        /* [replicas][n][k] */
  float* out;              /* [nonzeros] */
  const void* workspace;   /* planned: sputnik_hip_sddmm_sum_plan */
  size_t workspace_bytes;
  void* scratch;           /* sputnik_hip_sddmm_sum_scratch_bytes */
  size_t scratch_bytes;
  int nonzeros;
} sputnik_hip_sddmm_sum_problem;

SPUTNIK_HIP_API int sputnik_hip_sddmm_sum_group_planned(int m, int k, int n, int replicas,
                              int count, const sputnik_hip_sddmm_sum_problem* problems,
                              int64_t lhs_stride, int64_t rhs_stride,
                              sputnik_hip_stream_t stream);

/* ------------------------------------------------------------------------
 * Sparse softmax: per CSR row, exp(x - max) / sum(exp(x - max)) over the
 * stored entries.  `n` is unused (the reference passes -1,
 * src/softmax_cuda.cu:22).
 * replaces sputnik::SparseSoftmax(m,n,nnz,values,row_indices,row_offsets,
 *          column_indices,out,stream)               src/softmax_cuda.cu:36-42
 * and the host loop src/softmax_cuda.cu:35-43 (batched form).
 * ---------------------------------------------------------------------- */
SPUTNIK_HIP_API int sputnik_hip_sparse_softmax(int m, int n, int nonzeros, const float* values,
                               const int* row_indices, const int* row_offsets,
                               const int* column_indices, float* out,
                               sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_softmax_batched(int m, int n, int nonzeros, int replicas,
                                       const float* values, int64_t values_stride,
                                       const int* row_indices,
                                       const int* row_offsets,
                                       const int* column_indices, float* out,
                                       int64_t out_stride,
                                       sputnik_hip_stream_t stream);

/*
 * csr_transpose of values stored as `values_type` (SPUTNIK_HIP_F32 / F16 / BF16); the
 * transposed values are float32 (what the products of the backward passes take,
 * modules/sparse_linear.py:52-63).  Half values are read through the permutation by
 * the one gather that moves them: no widened copy of the input.  The half forms need
 * `out_permutation` (nonzeros ints); workspace as sputnik_hip_csr_transpose; `checked`
 * != 0 = sputnik_hip_csr_transpose_checked's behaviour (waits for the stream, reports a
 * pattern the transpose is not defined for).
 */
SPUTNIK_HIP_API int sputnik_hip_csr_transpose_typed(int m, int n, int nonzeros, int replicas,
                              const void* values, int values_type, int64_t values_stride,
                              const int* row_offsets, const int* column_indices,
                              float* out_values, int64_t out_values_stride,
                              int* out_row_offsets, int* out_column_indices,
                              int* out_permutation, void* workspace, size_t workspace_bytes,
                              int checked, sputnik_hip_stream_t stream);

/* ------------------------------------------------------------------------
 * CSR transpose  CSR(m x n) -> CSR(n x m), stable (source rows ascend within
 * each output row: the ordering of cuSPARSE CSR2CSC_ALG1).
 * replaces cusparseCsr2cscEx2_bufferSize            src/transpose_cuda.cu:22-31
 *      and cusparseCsr2cscEx2                       src/transpose_cuda.cu:90-99
 * `replicas` value arrays (stride values_stride / out_values_stride elements)
 * share one permutation; the reference only ever has replicas = 1.
 * `out_permutation` (may be NULL) receives, for every output slot, the index
 * of the source nonzero, so a caller can reuse a static topology's transpose.
 * Preconditions (as for cusparseCsr2cscEx2 on valid CSR): column indices in
 * [0, n), a row stores a column at most once (order inside a row is free).
 * A violation is DETECTED on the device: the status word (the last 16 bytes of
 * the workspace) is non-zero afterwards, and the outputs are unspecified (a bad
 * entry leaves a slot of the permutation unwritten; no value is read through it).
 * sputnik_hip_csr_transpose is asynchronous and leaves the word to the caller;
 * sputnik_hip_csr_transpose_checked (same arguments) waits for the stream and
 * returns SPUTNIK_HIP_INVALID_ARGUMENT.
 * Workspace: the smaller of about 4 * (2 * ceil(m / 32) * n + n) bytes (mask / count
 * tables: 2 MiB at 2048 x 2048) and, where those would exceed eight table entries
 * per nonzero, 4 * (2 n + 3 nnz) bytes (histogram path, O(n + nnz) like the
 * buffer cusparseCsr2cscEx2_bufferSize asks for: 5.4 MiB at 65536^2, density
 * 1e-4, where the tables would be 1 GiB); + 16.
 * ---------------------------------------------------------------------- */
SPUTNIK_HIP_API size_t sputnik_hip_csr_transpose_workspace_bytes(int m, int n, int nonzeros);

SPUTNIK_HIP_API int sputnik_hip_csr_transpose_checked(int m, int n, int nonzeros, int replicas,
                              const float* values, int64_t values_stride,
                              const int* row_offsets, const int* column_indices,
                              float* out_values, int64_t out_values_stride,
                              int* out_row_offsets, int* out_column_indices,
                              int* out_permutation, void* workspace, size_t workspace_bytes,
                              sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_csr_transpose(int m, int n, int nonzeros, int replicas,
                              const float* values, int64_t values_stride,
                              const int* row_offsets, const int* column_indices,
                              float* out_values, int64_t out_values_stride,
                              int* out_row_offsets, int* out_column_indices,
                              int* out_permutation, void* workspace,
                              size_t workspace_bytes,
                              sputnik_hip_stream_t stream);

/* The launches sputnik_hip_csr_transpose makes for a call of this shape (transpose.hip); the
 * entry takes its decisions from the same function this reports.
 *   path   SPUTNIK_HIP_TRANSPOSE_NONE: an empty dimension or no entries, nothing launched;
 *          _GROUPED: mask and count tables, scatter by chunk and group of 256 columns (up to
 *          8192 columns); _WIDE: the tables, a scan of the column totals and the plain
 *          scatter over column ranges of 8192; _SPARSE: the O(n + nnz) path, taken where the
 *          tables would hold more than eight entries per nonzero (ceil(m / 32) * n >
 *          8 * nonzeros: the condition sputnik_hip_csr_transpose_workspace_bytes sizes by)
 *   chunks                  blocks of 32 source rows (_GROUPED, _WIDE)
 *   ranges                  column ranges of 8192 (_GROUPED: 1, _WIDE)
 *   groups                  column groups per chunk in the grouped scatter's grid, a multiple
 *                           of 8 (_GROUPED)
 *   parts                   workgroups per chunk and range in the plain scatter, 8 / 4 / 2 / 1
 *                           with 32 / parts rows each (_WIDE)
 *   scan_chunks_per_group   chunks each of the table scan's 16 groups walks (_GROUPED, _WIDE):
 *                           up to 8 stay in registers, more take the kernel's second loops
 *   long_rank_launch        1 if the bitmap ranking kernel for output rows of more than 2048
 *                           entries is launched (nonzeros > 2048), else 0 (_SPARSE)
 * Fields that do not apply to the path are -1.  Host only, launches nothing; any output pointer
 * may be NULL.  Returns SPUTNIK_HIP_INVALID_ARGUMENT for a negative size or a shape whose grid
 * does not exist (the entry returns the same).  For tests, which assert the route they mean
 * to reach. */
#define SPUTNIK_HIP_TRANSPOSE_NONE 0
#define SPUTNIK_HIP_TRANSPOSE_GROUPED 1
#define SPUTNIK_HIP_TRANSPOSE_WIDE 2
#define SPUTNIK_HIP_TRANSPOSE_SPARSE 3
SPUTNIK_HIP_API int sputnik_hip_csr_transpose_route(int m, int n, int nonzeros, int* path,
                                                    int* chunks, int* ranges, int* groups,
                                                    int* parts, int* scan_chunks_per_group,
                                                    int* long_rank_launch);

/* ========================================================================
 * Extensions around the five operators.  The reference binding
 * as committed (src/sputnik.cpp:36-42) has none of these; the call sites that
 * fix their meaning are cited per entry.
 * ====================================================================== */

/*
 * SpMM with a fused epilogue: out[i, :] = act(sum + bias[i]); `bias` ([m],
 * indexed by output row, may be NULL) and relu (0/1) are both optional.
 * Call site: torch_sputnik.spmm_bias(m, k, values, row_indices, row_offsets,
 * column_indices, bias, dense), tests/test_spmm_bias_relu.py:35-37; the
 * SparseLinear callers add the bias in a separate pass
 * (tests/test_linear_3d.py:47).
 */
SPUTNIK_HIP_API int sputnik_hip_spmm_bias_batched(int m, int k, int n, int nonzeros,
                             int replicas, const int* row_indices,
                             const float* values, int64_t values_stride,
                             const int* row_offsets, const int* column_indices,
                             const float* dense, int64_t dense_stride,
                             const float* bias, int relu, float* out,
                             int64_t out_stride, void* workspace,
                             size_t workspace_bytes, sputnik_hip_stream_t stream);

/*
 * SpMM over a topology whose values are stored in ANOTHER order of the same
 * entries: entry p of (row_offsets, column_indices) takes
 * values[value_permutation[p]].  This is the product with the TRANSPOSE of a
 * matrix whose transposed topology and permutation are known (cached), as the
 * backward passes need it (modules/spmm.py:59-66 transposes the values per
 * call): the gather happens inside the kernel, no permuted copy is made.
 * Served by the panel kernel only (k <= 4096, n a multiple of 4 and >= 64,
 * m >= 16, 16-byte aligned operands); anything else returns
 * SPUTNIK_HIP_UNSUPPORTED and the caller permutes first
 * (sputnik_hip_permute_last_batched / _banded_batched) and calls
 * sputnik_hip_spmm_batched.  `_supported` answers 1 where the gather inside the
 * kernel is also the FASTER form: one panel, k <= 512 (with two panels every
 * value is gathered twice: 162 us against 41 + 50 us at the attention shapes).
 */
SPUTNIK_HIP_API int sputnik_hip_spmm_permuted_supported(int m, int k, int n, int nonzeros);

SPUTNIK_HIP_API int sputnik_hip_spmm_permuted_batched(int m, int k, int n, int nonzeros,
                             int replicas, const int* row_indices, const float* values,
                             int64_t values_stride, const int* value_permutation,
                             const int* row_offsets, const int* column_indices,
                             const float* dense, int64_t dense_stride, float* out,
                             int64_t out_stride, sputnik_hip_stream_t stream);

/*
 * SpMM whose product C[m, n] is STORED TRANSPOSED in blocks of `block_rows` rows:
 *   out[(row / block_rows) * n * block_rows + col * block_rows + row % block_rows]
 * per replica, i.e. every block of block_rows rows of C as its transpose
 * [n][block_rows].  With block_rows = head_dim this is the head split that
 * follows every projection (`four_d_to_three_d` on a transposed view,
 * modules/sparse_attention.py:38-45,108-126); with block_rows = m it is C^T, the
 * head merge in front of the output projection -- layout passes that the
 * reference runs as separate strided copies.  The panel kernel writes its
 * 256 x 64 tile through LDS in that order.  `value_permutation` may be NULL or
 * as in sputnik_hip_spmm_permuted_batched; bias / relu as in
 * sputnik_hip_spmm_bias_batched.  Rows are processed in natural order (no
 * row_indices).  Served: what the panel kernel serves, with block_rows a
 * multiple of 64 that divides m and divides or is a multiple of 256; otherwise
 * SPUTNIK_HIP_UNSUPPORTED (the caller runs the product and
 * sputnik_hip_transpose_batched).  `_supported` also requires k <= 1024.
 */
SPUTNIK_HIP_API int sputnik_hip_spmm_transposed_out_supported(int m, int k, int n, int nonzeros,
                                                              int block_rows);

SPUTNIK_HIP_API int sputnik_hip_spmm_transposed_out_batched(int m, int k, int n, int nonzeros,
                             int replicas, const float* values, int64_t values_stride,
                             const int* value_permutation, const int* row_offsets,
                             const int* column_indices, const float* dense,
                             int64_t dense_stride, const float* bias, int relu,
                             int block_rows, float* out, int64_t out_stride,
                             sputnik_hip_stream_t stream);

/*
 * A GROUP of up to four SpMMs of one shape (m, k, n; values shared by the
 * replicas) in one launch: the projections of an attention block
 * (modules/sparse_attention.py:108-126 runs them one after the other).
 *   accumulate = 0: out_p[r] = A_p * dense_p[r] for every problem p.  Problems
 *     that name the same `dense` share one copy of its panel in LDS (the q, k
 *     and v projections of one input); with block_rows > 0 every product is
 *     stored head split as in sputnik_hip_spmm_transposed_out_batched.
 *   accumulate = 1: all problems name the SAME `out`, which receives
 *     sum_p A_p * dense_p[r] (overwritten, not added to): the input gradient
 *     sum_w W_w^T dY_w of those projections, accumulated in registers.
 * value_permutation: NULL in all problems or set in all (as in
 * sputnik_hip_spmm_permuted_batched).  row_indices: the processing order for
 * accumulate = 0 and block_rows = 0; ignored (may be NULL) otherwise.
 * Served: k <= 512, n a multiple of 4 and >= 64, m >= 16, 16-byte aligned
 * operands, at most 4 problems, and one of the combinations
 * (block_rows > 0, no permutation, accumulate = 0), (block_rows = 0, accumulate
 * = 1), (block_rows = 0, no permutation, accumulate = 0); anything else returns
 * SPUTNIK_HIP_UNSUPPORTED and the caller runs the products one by one.
 */
typedef struct sputnik_hip_spmm_problem {
  const int* row_indices;
  const int* row_offsets;
  const int* column_indices;
  const float* values;            /* [nonzeros] */
  const int* value_permutation;   /* NULL, or [nonzeros] */
  const float* dense;             /* [replicas][k][n], dense_stride apart */
  float* out;                     /* [replicas][m][n] (or its blocked transpose) */
  int nonzeros;
} sputnik_hip_spmm_problem;

SPUTNIK_HIP_API int sputnik_hip_spmm_group_supported(int m, int k, int n, int count,
                                                     int block_rows, int accumulate);

SPUTNIK_HIP_API int sputnik_hip_spmm_group_batched(int m, int k, int n, int replicas, int count,
                             const sputnik_hip_spmm_problem* problems,
                             int64_t dense_stride, int64_t out_stride, int block_rows,
                             int accumulate, sputnik_hip_stream_t stream);

/*
 * softmax(scale * x) per CSR row: folds the 1/sqrt(d) of
 * modules/sparse_attention.py:72 into the softmax pass.
 */
SPUTNIK_HIP_API int sputnik_hip_sparse_softmax_scaled_batched(int m, int n, int nonzeros,
                             int replicas, const float* values, int64_t values_stride,
                             const int* row_indices, const int* row_offsets,
                             const int* column_indices, float scale, float* out,
                             int64_t out_stride, sputnik_hip_stream_t stream);

/*
 * Gradient of y = softmax(scale * x):
 *   grad_values = scale * y * (grad_out - rowsum(grad_out * y)),
 * row sums over the stored entries.  The reference calls the raw op inside
 * attention (modules/sparse_attention.py:76), which cuts the gradient; the
 * intended autograd wrapper is tests/transformer/functions.py:70-120.
 * Aliasing: `grad_values` may be the very buffer `grad_out` (same pointer, same stride:
 * the gradient is overwritten in place) -- every entry of a row is read before any entry
 * of that row is written, and a row's result depends on its own entries only.  Any other
 * overlap of the output with an input is not supported.  The same holds for the _typed
 * and _many_mask forms.
 */
SPUTNIK_HIP_API int sputnik_hip_sparse_softmax_backward_batched(int m, int nonzeros,
                             int replicas, const float* softmax_out, int64_t out_stride,
                             const float* grad_out, int64_t grad_out_stride,
                             const int* row_offsets, float scale, float* grad_values,
                             int64_t grad_values_stride, sputnik_hip_stream_t stream);

/*
 * The softmax pair on values stored as `dtype` (SPUTNIK_HIP_F32 / F16 / BF16; inputs
 * and output alike; strides in elements).  Half types move 2 + 2 bytes per entry
 * forward, 2 + 2 + 2 backward -- half the HBM traffic of src/softmax_cuda.cu:38-42 --
 * and are widened / rounded to nearest even in registers; max, exp, sum and the
 * gradient's row dot product are float32.  The float entry points above are
 * dtype = SPUTNIK_HIP_F32 of these.
 */
SPUTNIK_HIP_API int sputnik_hip_sparse_softmax_typed(int m, int n, int nonzeros, int replicas,
                             const void* values, int64_t values_stride, const int* row_indices,
                             const int* row_offsets, const int* column_indices, float scale,
                             void* out, int64_t out_stride, int dtype,
                             sputnik_hip_stream_t stream);
SPUTNIK_HIP_API int sputnik_hip_sparse_softmax_backward_typed(int m, int nonzeros, int replicas,
                             const void* softmax_out, int64_t out_stride, const void* grad_out,
                             int64_t grad_out_stride, const int* row_offsets, float scale,
                             void* grad_values, int64_t grad_values_stride, int dtype,
                             sputnik_hip_stream_t stream);

/*
 * Fused sparse attention forward, one launch for
 *   out = spmm(softmax(scale * sddmm(q, k)), v)
 * i.e. the chain of modules/sparse_attention.py:66-82 (sddmm :68-71, the
 * division by sqrt(d) :72, sparse_softmax :76, spmm :79-82) without the
 * [replicas, nonzeros] intermediates.  q [m,d], k and v [n,d] per replica,
 * out [m,d]; `lse` (may be NULL) receives log(sum(exp(scale*score))) per row
 * for a later backward.  Served shapes: d = 64 with 16-byte aligned operands
 * (sputnik_hip_sparse_attention_supported); anything else returns
 * SPUTNIK_HIP_UNSUPPORTED and the caller composes the three operators.
 * Rows without entries produce zeros (and lse = -inf).
 */
SPUTNIK_HIP_API int sputnik_hip_sparse_attention_supported(int m, int n, int d, int nonzeros);

SPUTNIK_HIP_API size_t sputnik_hip_sparse_attention_workspace_bytes(int m, int n, int d,
                                                                    int nonzeros);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_forward(int m, int n, int d, int nonzeros,
                             int replicas, const int* row_indices, const int* row_offsets,
                             const int* column_indices, const float* q, int64_t q_stride,
                             const float* k, int64_t k_stride, const float* v,
                             int64_t v_stride, float scale, float* out, int64_t out_stride,
                             float* lse, int64_t lse_stride, void* workspace,
                             size_t workspace_bytes, sputnik_hip_stream_t stream);

/* The same in two steps for a static mask: plan once, run any number of times. */
SPUTNIK_HIP_API int sputnik_hip_sparse_attention_plan(int m, int n, int d, int nonzeros,
                             const int* row_indices, const int* row_offsets,
                             const int* column_indices, void* workspace,
                             size_t workspace_bytes, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_forward_planned(int m, int n, int d,
                             int nonzeros, int replicas, const int* row_indices,
                             const int* row_offsets, const int* column_indices, const float* q,
                             int64_t q_stride, const float* k, int64_t k_stride, const float* v,
                             int64_t v_stride, float scale, float* out, int64_t out_stride,
                             float* lse, int64_t lse_stride, const void* workspace,
                             size_t workspace_bytes, sputnik_hip_stream_t stream);

/*
 * The fused attention on float16 / bfloat16 storage (`dtype` SPUTNIK_HIP_F16 / BF16) with
 * every operand a strided HEAD VIEW: element (b, h, row, c) of q, k, v and out at
 *   base + b * batch_stride + h * head_stride + row * row_stride + c      (elements)
 * for b < batch, h < heads (replica r = b * heads + h), so that q, k, v and the context can
 * stay [B, S, E] tensors (head h = columns h*d .. h*d+d-1: batch_stride S*E, head_stride d,
 * row_stride E) -- no head split or merge pass.  Values are widened in registers; scores,
 * weights, the online softmax and every sum are float32.  `out` is stored as `out_type`:
 * SPUTNIK_HIP_F32 or `dtype`.  `lse` (may be NULL): lse[r * lse_stride + row], float32.
 * sputnik_hip_sparse_attention_heads_supported checks on the host everything the kernel
 * assumes: a shape sputnik_hip_sparse_attention_supported serves (d = 64, a mask with
 * entries), 16-byte aligned bases, strides non-negative and multiples of 16 bytes, and
 * every replica's extent ((rows - 1) * row_stride + d elements) below 2^32 bytes.  The
 * forward returns SPUTNIK_HIP_UNSUPPORTED for anything else: compose the typed operators
 * then.  The workspace and the plan are those of sputnik_hip_sparse_attention_* (the plan
 * is topology-only: sputnik_hip_sparse_attention_plan makes it for either kernel).
 * Rows without entries produce zeros (and lse = -inf).
 */
SPUTNIK_HIP_API int sputnik_hip_sparse_attention_heads_supported(int m, int n, int d, int nonzeros,
                             int batch, int heads, int dtype, int out_type, const void* q,
                             int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride,
                             const void* k, int64_t k_batch_stride, int64_t k_head_stride,
                             int64_t k_row_stride, const void* v, int64_t v_batch_stride,
                             int64_t v_head_stride, int64_t v_row_stride, const void* out,
                             int64_t out_batch_stride, int64_t out_head_stride,
                             int64_t out_row_stride);

SPUTNIK_HIP_API size_t sputnik_hip_sparse_attention_heads_workspace_bytes(int m, int n, int d,
                                                                          int nonzeros);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_heads_forward(int m, int n, int d, int nonzeros,
                             int batch, int heads, const int* row_indices, const int* row_offsets,
                             const int* column_indices, int dtype, const void* q,
                             int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride,
                             const void* k, int64_t k_batch_stride, int64_t k_head_stride,
                             int64_t k_row_stride, const void* v, int64_t v_batch_stride,
                             int64_t v_head_stride, int64_t v_row_stride, float scale, void* out,
                             int out_type, int64_t out_batch_stride, int64_t out_head_stride,
                             int64_t out_row_stride, float* lse, int64_t lse_stride,
                             void* workspace, size_t workspace_bytes, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_heads_forward_planned(int m, int n, int d,
                             int nonzeros, int batch, int heads, const int* row_indices,
                             const int* row_offsets, const int* column_indices, int dtype,
                             const void* q, int64_t q_batch_stride, int64_t q_head_stride,
                             int64_t q_row_stride, const void* k, int64_t k_batch_stride,
                             int64_t k_head_stride, int64_t k_row_stride, const void* v,
                             int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride,
                             float scale, void* out, int out_type, int64_t out_batch_stride,
                             int64_t out_head_stride, int64_t out_row_stride, float* lse,
                             int64_t lse_stride, const void* workspace, size_t workspace_bytes,
                             sputnik_hip_stream_t stream);

/*
 * The fused attention with one mask per batch element (the "many mask" layout below:
 * row_indices [masks * m], row_offsets [masks * (m + 1)] each starting at 0,
 * column_indices concatenated, `nonzeros` [masks] a HOST array).  `replicas` is a
 * multiple of `masks`; replica r uses mask r / (replicas / masks).  q [m,d], k and v
 * [n,d] per replica as in sputnik_hip_sparse_attention_forward; `lse` may be NULL.
 * All masks are served by one pre-pass launch and one attention launch, the heads of
 * the densest masks started first; nothing waits for the host, so the planned form can
 * be captured in a graph.  A mask without entries gives its replicas zeros (and
 * lse = -inf), as do rows without entries; rows whose columns do not ascend are served
 * in any order.
 * Returns SPUTNIK_HIP_UNSUPPORTED for what the kernel does not serve (d != 64, operands
 * or strides not 16-byte aligned, n * d * 4 bytes of 2^32 or more; the single-mask rules
 * applied to the largest mask; more than 65535 replicas, which one launch cannot hold) and
 * SPUTNIK_HIP_INVALID_ARGUMENT when replicas % masks != 0
 * or the workspace is smaller than
 * sputnik_hip_sparse_attention_many_mask_workspace_bytes(masks, m, n, d, max(nonzeros))
 * (0: not served).  `plan` runs the topology-only pre-pass into the workspace for
 * `forward_planned`; the plan is valid for both forms below while the topology tensors,
 * masks, m, n and max(nonzeros) do not change.
 */
SPUTNIK_HIP_API size_t sputnik_hip_sparse_attention_many_mask_workspace_bytes(int masks, int m, int n,
                             int d, int largest_nonzeros);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_many_mask_plan(int masks, int m, int n, int d,
                             const int* nonzeros, const int* row_indices, const int* row_offsets,
                             const int* column_indices, void* workspace, size_t workspace_bytes,
                             sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_many_mask_forward(int masks, int m, int n, int d,
                             const int* nonzeros, int replicas, const int* row_indices,
                             const int* row_offsets, const int* column_indices, const float* q,
                             int64_t q_stride, const float* k, int64_t k_stride, const float* v,
                             int64_t v_stride, float scale, float* out, int64_t out_stride,
                             float* lse, int64_t lse_stride, void* workspace,
                             size_t workspace_bytes, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_many_mask_forward_planned(int masks, int m, int n,
                             int d, const int* nonzeros, int replicas, const int* row_indices,
                             const int* row_offsets, const int* column_indices, const float* q,
                             int64_t q_stride, const float* k, int64_t k_stride, const float* v,
                             int64_t v_stride, float scale, float* out, int64_t out_stride,
                             float* lse, int64_t lse_stride, const void* workspace,
                             size_t workspace_bytes, sputnik_hip_stream_t stream);

/*
 * The same on float16 / bfloat16 head views (sputnik_hip_sparse_attention_heads_forward:
 * strides in elements, out_type SPUTNIK_HIP_F32 or `dtype`): batch element b uses mask b,
 * so `batch` must equal `masks` (else SPUTNIK_HIP_INVALID_ARGUMENT).  Served when
 * sputnik_hip_sparse_attention_heads_supported serves the views for the largest mask;
 * workspace and plan as above.
 */
SPUTNIK_HIP_API int sputnik_hip_sparse_attention_heads_many_mask_forward(int masks, int m, int n,
                             int d, const int* nonzeros, int batch, int heads,
                             const int* row_indices, const int* row_offsets,
                             const int* column_indices, int dtype, const void* q,
                             int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride,
                             const void* k, int64_t k_batch_stride, int64_t k_head_stride,
                             int64_t k_row_stride, const void* v, int64_t v_batch_stride,
                             int64_t v_head_stride, int64_t v_row_stride, float scale, void* out,
                             int out_type, int64_t out_batch_stride, int64_t out_head_stride,
                             int64_t out_row_stride, float* lse, int64_t lse_stride,
                             void* workspace, size_t workspace_bytes, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_heads_many_mask_forward_planned(int masks, int m,
                             int n, int d, const int* nonzeros, int batch, int heads,
                             const int* row_indices, const int* row_offsets,
                             const int* column_indices, int dtype, const void* q,
                             int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride,
                             const void* k, int64_t k_batch_stride, int64_t k_head_stride,
                             int64_t k_row_stride, const void* v, int64_t v_batch_stride,
                             int64_t v_head_stride, int64_t v_row_stride, float scale, void* out,
                             int out_type, int64_t out_batch_stride, int64_t out_head_stride,
                             int64_t out_row_stride, float* lse, int64_t lse_stride,
                             const void* workspace, size_t workspace_bytes,
                             sputnik_hip_stream_t stream);

/* ------------------------------------------------------------------------
 * Attention dropout.  Dropout on the attention probabilities (between the softmax and the
 * product with v), decided per stored entry by a counter-based generator so that the fused
 * kernels, sparse_dropout on a values array and a backward's replay all drop the same ones:
 *
 *   key     = (seed lo, seed hi)
 *   counter = (offset/4 lo, offset/4 hi, e >> 2, r)      Philox4x32-10, output word e & 3
 *   keep    = word < min(floor((1 - p) 2^32), 2^32 - 1)  (double), kept x float(1/(1 - p))
 *
 * r is the replica (b * heads + h for head views), e the entry's index in its replica's row
 * of the values array: the CSR position for one mask, the position inside the mask for many
 * masks (the column of the [replicas, max(nonzeros)] arrays).  This is ATen's
 * Philox4_32(seed, (r << 32) | (e >> 2), offset) for an offset that is a multiple of 4.
 * 0 <= p < 1; any other p gives SPUTNIK_HIP_INVALID_ARGUMENT.  p = 0 runs the forms without
 * dropout and touches neither the state nor rng_state_out.
 *
 * The state mirrors a PyTorch PhiloxCudaState: values, or (seed_ptr, offset_ptr) device
 * pointers read when the kernel runs (offset = *offset_ptr + offset_intragraph), which is how
 * a captured graph draws new masks on every replay.  `rng_state_out` (may be NULL), int64
 * [2] in device memory, receives the {seed, offset} the call used; handing it back as
 * {seed_ptr, offset_ptr} = {rng_state_out, rng_state_out + 1} replays the mask.
 * ------------------------------------------------------------------------ */
typedef struct sputnik_hip_philox_state {
  uint64_t seed;
  uint64_t offset;
  const int64_t* seed_ptr;     /* NULL: `seed` holds it */
  const int64_t* offset_ptr;   /* NULL: `offset` holds it */
  uint64_t offset_intragraph;
} sputnik_hip_philox_state;

/* out[r, e] = x[r, e] * keep(r, e) * scale for x [rows, width] (row strides in elements) of
 * `dtype` (SPUTNIK_HIP_F32 / F16 / BF16); out has x's type, the product is formed in float32
 * and rounded once.  Many-mask arrays go in at their full [replicas, max(nonzeros)] width:
 * zero padding stays zero.  `replica0` is the replica index of row 0. */
SPUTNIK_HIP_API int sputnik_hip_sparse_dropout_typed(int rows, int width, int replica0, int dtype,
                             const void* x, int64_t x_stride, void* out, int64_t out_stride,
                             double p, sputnik_hip_philox_state rng, int64_t* rng_state_out,
                             sputnik_hip_stream_t stream);

/* The fused forms with dropout: the arguments of the form without, then p, the state and
 * rng_state_out.  `lse` stays the log-sum-exp of the undropped scores (what a backward
 * needs to rebuild the weights); the output is (sum_kept e_j v_j) * scale / sum_all e_j. */
SPUTNIK_HIP_API int sputnik_hip_sparse_attention_forward_dropout(int m, int n, int d, int nonzeros,
                             int replicas, const int* row_indices, const int* row_offsets,
                             const int* column_indices, const float* q, int64_t q_stride,
                             const float* k, int64_t k_stride, const float* v,
                             int64_t v_stride, float scale, float* out, int64_t out_stride,
                             float* lse, int64_t lse_stride, double p, sputnik_hip_philox_state rng,
                             int64_t* rng_state_out, void* workspace, size_t workspace_bytes,
                             sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_forward_planned_dropout(int m, int n, int d,
                             int nonzeros, int replicas, const int* row_indices,
                             const int* row_offsets, const int* column_indices, const float* q,
                             int64_t q_stride, const float* k, int64_t k_stride, const float* v,
                             int64_t v_stride, float scale, float* out, int64_t out_stride,
                             float* lse, int64_t lse_stride, double p, sputnik_hip_philox_state rng,
                             int64_t* rng_state_out, const void* workspace,
                             size_t workspace_bytes, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_heads_forward_dropout(int m, int n, int d,
                             int nonzeros, int batch, int heads, const int* row_indices,
                             const int* row_offsets, const int* column_indices, int dtype,
                             const void* q, int64_t q_batch_stride, int64_t q_head_stride,
                             int64_t q_row_stride, const void* k, int64_t k_batch_stride,
                             int64_t k_head_stride, int64_t k_row_stride, const void* v,
                             int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride,
                             float scale, void* out, int out_type, int64_t out_batch_stride,
                             int64_t out_head_stride, int64_t out_row_stride, float* lse,
                             int64_t lse_stride, double p, sputnik_hip_philox_state rng,
                             int64_t* rng_state_out, void* workspace, size_t workspace_bytes,
                             sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_heads_forward_planned_dropout(int m, int n, int d,
                             int nonzeros, int batch, int heads, const int* row_indices,
                             const int* row_offsets, const int* column_indices, int dtype,
                             const void* q, int64_t q_batch_stride, int64_t q_head_stride,
                             int64_t q_row_stride, const void* k, int64_t k_batch_stride,
                             int64_t k_head_stride, int64_t k_row_stride, const void* v,
                             int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride,
                             float scale, void* out, int out_type, int64_t out_batch_stride,
                             int64_t out_head_stride, int64_t out_row_stride, float* lse,
                             int64_t lse_stride, double p, sputnik_hip_philox_state rng,
                             int64_t* rng_state_out, const void* workspace,
                             size_t workspace_bytes, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_many_mask_forward_dropout(int masks, int m, int n,
                             int d, const int* nonzeros, int replicas, const int* row_indices,
                             const int* row_offsets, const int* column_indices, const float* q,
                             int64_t q_stride, const float* k, int64_t k_stride, const float* v,
                             int64_t v_stride, float scale, float* out, int64_t out_stride,
                             float* lse, int64_t lse_stride, double p, sputnik_hip_philox_state rng,
                             int64_t* rng_state_out, void* workspace, size_t workspace_bytes,
                             sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_many_mask_forward_planned_dropout(int masks, int m,
                             int n, int d, const int* nonzeros, int replicas,
                             const int* row_indices, const int* row_offsets,
                             const int* column_indices, const float* q, int64_t q_stride,
                             const float* k, int64_t k_stride, const float* v, int64_t v_stride,
                             float scale, float* out, int64_t out_stride, float* lse,
                             int64_t lse_stride, double p, sputnik_hip_philox_state rng,
                             int64_t* rng_state_out, const void* workspace,
                             size_t workspace_bytes, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_heads_many_mask_forward_dropout(int masks, int m,
                             int n, int d, const int* nonzeros, int batch, int heads,
                             const int* row_indices, const int* row_offsets,
                             const int* column_indices, int dtype, const void* q,
                             int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride,
                             const void* k, int64_t k_batch_stride, int64_t k_head_stride,
                             int64_t k_row_stride, const void* v, int64_t v_batch_stride,
                             int64_t v_head_stride, int64_t v_row_stride, float scale, void* out,
                             int out_type, int64_t out_batch_stride, int64_t out_head_stride,
                             int64_t out_row_stride, float* lse, int64_t lse_stride, double p,
                             sputnik_hip_philox_state rng, int64_t* rng_state_out,
                             void* workspace, size_t workspace_bytes,
                             sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_heads_many_mask_forward_planned_dropout(int masks,
                             int m, int n, int d, const int* nonzeros, int batch, int heads,
                             const int* row_indices, const int* row_offsets,
                             const int* column_indices, int dtype, const void* q,
                             int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride,
                             const void* k, int64_t k_batch_stride, int64_t k_head_stride,
                             int64_t k_row_stride, const void* v, int64_t v_batch_stride,
                             int64_t v_head_stride, int64_t v_row_stride, float scale, void* out,
                             int out_type, int64_t out_batch_stride, int64_t out_head_stride,
                             int64_t out_row_stride, float* lse, int64_t lse_stride, double p,
                             sputnik_hip_philox_state rng, int64_t* rng_state_out,
                             const void* workspace, size_t workspace_bytes,
                             sputnik_hip_stream_t stream);

/*
 * Fused sparse attention backward: the gradients of sputnik_hip_sparse_attention_forward
 * (or its _dropout form) for one mask, without any [replicas, nonzeros] intermediate.
 * With D_i = <dO_i, O_i>, every stored entry (i, j) gives
 *   p  = exp(scale * <q_i, k_j> - lse_i)      pd = p * keep(r, e) / (1 - p_drop)
 *   dp = <dO_i, v_j> * keep(r, e) / (1 - p_drop)       ds = p * (dp - D_i) * scale
 *   dQ_i += ds * k_j     dK_j += ds * q_i     dV_j += pd * dO_i
 * (keep = 1 and no factor for p = 0).  Arguments:
 *   m, n, d, nonzeros, replicas, row_indices, row_offsets, column_indices, q, k, v, scale
 *                  as in the forward; q [m,d], k and v [n,d] per replica.
 *   t_row_indices, t_row_offsets, t_column_indices, permutation
 *                  the transposed mask (n rows of query indices; t_row_indices orders its
 *                  rows, e.g. by length) and the original entry of each of its slots, as
 *                  sputnik_hip_csr_transpose returns them.  Read only for dK / dV, the
 *                  permutation only with dropout.
 *   out, grad_out  the forward's output O and its gradient dO, [m,d] per replica.
 *   lse            the forward's log-sum-exp [replicas][lse_stride], of the undropped scores.
 *   grad_q, grad_k, grad_v
 *                  [m,d], [n,d], [n,d] per replica, each may be NULL when not wanted; every
 *                  row is written (rows and key columns without entries get zeros).
 *   p, rng         the forward's dropout p and a state that replays its mask (the
 *                  forward's rng_state_out as {seed_ptr, offset_ptr}); p = 0: none.
 *   workspace      at least sputnik_hip_sparse_attention_backward_workspace_bytes, 16-byte
 *                  aligned, per call (the D_i of every row; nothing is kept between calls).
 * Strides are per replica, in elements.  Two launches, no atomics (bitwise reproducible),
 * no host synchronisation.  Served: d = 64 or 128, m * d * 4 and n * d * 4 below 2^32, 16-byte
 * aligned operands and strides that are multiples of 4
 * (sputnik_hip_sparse_attention_backward_supported); anything else returns
 * SPUTNIK_HIP_UNSUPPORTED and the caller composes the backward from the operators.
 */
SPUTNIK_HIP_API int sputnik_hip_sparse_attention_backward_supported(int m, int n, int d,
                                                                    int nonzeros);

SPUTNIK_HIP_API size_t sputnik_hip_sparse_attention_backward_workspace_bytes(int m, int n, int d,
                                                                             int nonzeros,
                                                                             int replicas);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_backward(int m, int n, int d, int nonzeros,
                             int replicas, const int* row_indices, const int* row_offsets,
                             const int* column_indices, const int* t_row_indices,
                             const int* t_row_offsets, const int* t_column_indices,
                             const int* permutation, const float* q, int64_t q_stride,
                             const float* k, int64_t k_stride, const float* v, int64_t v_stride,
                             float scale, const float* out, int64_t out_stride,
                             const float* grad_out, int64_t grad_out_stride, const float* lse,
                             int64_t lse_stride, float* grad_q, int64_t grad_q_stride,
                             float* grad_k, int64_t grad_k_stride, float* grad_v,
                             int64_t grad_v_stride, double p, sputnik_hip_philox_state rng,
                             void* workspace, size_t workspace_bytes,
                             sputnik_hip_stream_t stream);

/*
 * Fused sparse attention forward in the row-group form: what
 * sputnik_hip_sparse_attention_forward_dropout computes -- out, and lse (the log-sum-exp of
 * the undropped scores; may be NULL) for sputnik_hip_sparse_attention_backward -- at head
 * dimension 128, which the LDS-staged forward does not serve.  One 16-lane row group per
 * query row gathers the K and V rows of the row's entries from L2 and keeps an online softmax
 * in registers; one launch (per 65535 replicas), no workspace, no plan, no atomics (bitwise
 * reproducible), no host synchronisation.  The order of a row's columns does not matter.
 * The arguments are those of sputnik_hip_sparse_attention_forward_dropout without the
 * workspace; p = 0 drops nothing and touches neither the state nor rng_state_out.
 * Served (sputnik_hip_sparse_attention_rows_supported): d = 128, m, n and nonzeros above 0,
 * m * d * 4 and n * d * 4 below 2^32, 16-byte aligned operands and strides that are multiples
 * of 4; anything else returns SPUTNIK_HIP_UNSUPPORTED before any launch.
 */
SPUTNIK_HIP_API int sputnik_hip_sparse_attention_rows_supported(int m, int n, int d, int nonzeros);

SPUTNIK_HIP_API int sputnik_hip_sparse_attention_rows_forward(int m, int n, int d, int nonzeros,
                             int replicas, const int* row_indices, const int* row_offsets,
                             const int* column_indices, const float* q, int64_t q_stride,
                             const float* k, int64_t k_stride, const float* v,
                             int64_t v_stride, float scale, float* out, int64_t out_stride,
                             float* lse, int64_t lse_stride, double p, sputnik_hip_philox_state rng,
                             int64_t* rng_state_out, sputnik_hip_stream_t stream);

/* ------------------------------------------------------------------------
 * "many mask" family: `masks` topologies of the same m x n shape, laid out
 * as tests/transformer/utils.py:17-38 builds them:
 *   row_indices    [masks * m]        local row ids of mask i at i*m
 *   row_offsets    [masks * (m + 1)]  each mask's offsets start at 0
 *   column_indices [sum nonzeros[i]]  concatenated
 *   nonzeros       [masks]            HOST array
 * `replicas` (a multiple of `masks`) value / dense slices; replica r uses
 * mask r / (replicas / masks), i.e. the heads of one batch element share its
 * mask (tests/test_attention_many_masks.py:107-150).  Replica r keeps its
 * nonzeros[mask] values at values + r * values_stride; the stride is at least
 * max(nonzeros), and anything past a replica's own count is never written (it
 * may be read: the rows are moved in aligned 16-byte pieces).
 * Call sites: torch_sputnik.{sddmm,sparse_softmax,spmm,csr_transpose}_many_mask,
 * tests/transformer/functions.py:20,41,50,59,81,135,156,165,177.
 * One launch per operator serves all masks (softmax pair; SDDMM; SpMM where the
 * panel-resident kernel applies, n = head_dim), see csrc/many_mask.hip.
 * Workspaces: the single-mask query at max(nonzeros); for SDDMM
 * sputnik_hip_sddmm_many_mask_workspace_bytes (one plan per mask; with less the
 * call still works, on the workspace-free kernel).
 * ---------------------------------------------------------------------- */
SPUTNIK_HIP_API size_t sputnik_hip_sddmm_many_mask_workspace_bytes(int masks, int m, int k, int n,
                                                                   int largest_nonzeros);

SPUTNIK_HIP_API int sputnik_hip_spmm_many_mask(int masks, int m, int k, int n,
                             const int* nonzeros, int replicas, const int* row_indices,
                             const float* values, int64_t values_stride,
                             const int* row_offsets, const int* column_indices,
                             const float* dense, int64_t dense_stride, float* out,
                             int64_t out_stride, void* workspace,
                             size_t workspace_bytes, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sddmm_many_mask(int masks, int m, int k, int n,
                             const int* nonzeros, int replicas, const int* row_indices,
                             const int* row_offsets, const int* column_indices,
                             const float* lhs, int64_t lhs_stride, const float* rhs,
                             int64_t rhs_stride, float* out, int64_t out_stride,
                             void* workspace, size_t workspace_bytes,
                             sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_softmax_many_mask(int masks, int m,
                             const int* nonzeros, int replicas, const float* values,
                             int64_t values_stride, const int* row_indices,
                             const int* row_offsets, const int* column_indices,
                             float scale, float* out, int64_t out_stride,
                             sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_sparse_softmax_backward_many_mask(int masks, int m,
                             const int* nonzeros, int replicas, const float* softmax_out,
                             int64_t out_stride, const float* grad_out,
                             int64_t grad_out_stride, const int* row_offsets, float scale,
                             float* grad_values, int64_t grad_values_stride,
                             sputnik_hip_stream_t stream);

/* out_row_offsets [masks][n + 1], out_column_indices / out_permutation
 * (may be NULL) laid out like column_indices.  With a workspace of
 * sputnik_hip_csr_transpose_many_mask_workspace_bytes (a region of tables and
 * room for the permutation per mask) all masks are transposed by the same three
 * launches, plus one gather for the values of all replicas when a mask has
 * several heads; with less, but at least
 * sputnik_hip_csr_transpose_workspace_bytes(m, n, largest), mask after mask. */
SPUTNIK_HIP_API size_t sputnik_hip_csr_transpose_many_mask_workspace_bytes(int masks, int m, int n,
                             int largest_nonzeros);
SPUTNIK_HIP_API int sputnik_hip_csr_transpose_many_mask(int masks, int m, int n,
                             const int* nonzeros, int replicas, const float* values,
                             int64_t values_stride, const int* row_offsets,
                             const int* column_indices, float* out_values,
                             int64_t out_values_stride, int* out_row_offsets,
                             int* out_column_indices, int* out_permutation,
                             void* workspace, size_t workspace_bytes,
                             sputnik_hip_stream_t stream);
/* What sputnik_hip_csr_transpose_many_mask does for a batch of `masks` masks whose largest
 * holds `largest_nonzeros` entries and which hold `total_nonzeros` together, with `heads`
 * value rows per mask (0: no values passed) at least `largest_nonzeros` wide, with or without
 * a permutation output, in a workspace of `workspace_bytes` (0: none); the entry takes its
 * decision from the same function this reports, and from nothing else.  (That function also
 * sends value rows NARROWER than `largest_nonzeros`, by either stride, mask after mask; the
 * query has no stride input and answers for rows that are wide enough.)
 *   one_launch   1: one launch per phase serves all masks; 0: mask after mask, each as
 *                sputnik_hip_csr_transpose_route says (fewer than two masks, more than 8192
 *                columns, a largest mask on the O(n + nnz) path, or a workspace without a
 *                region per mask -- plus room for the permutation behind the regions when
 *                several heads are moved and the caller takes no permutation)
 *   values_by    SPUTNIK_HIP_MANY_VALUES_NONE / _SCATTER (one head: the values ride in the
 *                scatter) / _GATHER (several heads: one gather through the permutation);
 *                -1 mask after mask
 * Host only, launches nothing; any output pointer may be NULL.  Returns
 * SPUTNIK_HIP_INVALID_ARGUMENT for a negative argument. */
#define SPUTNIK_HIP_MANY_VALUES_NONE 0
#define SPUTNIK_HIP_MANY_VALUES_SCATTER 1
#define SPUTNIK_HIP_MANY_VALUES_GATHER 2
SPUTNIK_HIP_API int sputnik_hip_csr_transpose_many_mask_route(int masks, int m, int n,
                             int largest_nonzeros, int64_t total_nonzeros, int heads,
                             int with_permutation, size_t workspace_bytes, int* one_launch,
                             int* values_by);

/* ========================================================================
 * CSR topologies from dense masks / matrices, built on the device (topology.hip).
 * What topology.dense_to_sparse, dense_to_sparse_3d, diffsort and
 * functional.diffsort_many_mask compute (modules/sparse_attention.py:12-36,
 * tests/transformer/utils.py:17-62 of the reference), in a fixed number of
 * launches for any number of masks.  No workspace.
 *
 * `dense` holds `masks` matrices of m x n elements of `element_bytes` (1, 2, 4 or 8)
 * bytes: element (i, r, c) at dense + i * batch_stride + r * row_stride + c, strides
 * in ELEMENTS and >= 0 (0: one matrix shared by all masks, or one row by all rows),
 * the last dimension dense.  An element is a nonzero exactly when torch's `x != 0`
 * says so, decided on its bits: `floating` = 0 (bool and integer types) any bit set,
 * `floating` = 1 (float16, bfloat16, float32, float64) any bit but the sign -- -0.0
 * is no entry, NaN, +-inf and denormals are.
 * ====================================================================== */

/* Phase 1.  row_offsets [masks][m + 1] (int32, each mask's starting at 0), nonzeros [masks]
 * (int32) and bases [masks] (int64: the entries of the masks in front, where a mask's
 * column_indices start in the concatenated many-mask layout), all on the device.  Three
 * launches (rows, a scan per mask, the bases); asynchronous.  The caller reads `nonzeros`
 * back to size column_indices -- the one synchronisation of a build.
 * SPUTNIK_HIP_INVALID_ARGUMENT: a negative size or stride, an element width other than
 * 1 / 2 / 4 / 8, m * n above INT_MAX (a mask's count must fit its int32 offsets), a grid
 * above INT_MAX workgroups, a pointer that is NULL or not aligned to its element. */
SPUTNIK_HIP_API int sputnik_hip_dense_to_csr_count(int masks, int m, int n, const void* dense,
                             int element_bytes, int floating, int64_t batch_stride,
                             int64_t row_stride, int* row_offsets, int* nonzeros, int64_t* bases,
                             sputnik_hip_stream_t stream);

/* Phase 2, given phase 1's row_offsets and bases: column_indices [sum of nonzeros] (int32),
 * ascending inside every row, the masks' arrays back to back; and, `values` not NULL, the
 * kept elements themselves, copied bit for bit in the source type, in the same order.  One
 * launch: per step of 64 elements a wave ballot and a lane prefix count place the kept
 * ones.  Arguments are checked as in phase 1. */
SPUTNIK_HIP_API int sputnik_hip_dense_to_csr_fill(int masks, int m, int n, const void* dense,
                             int element_bytes, int floating, int64_t batch_stride,
                             int64_t row_stride, const int* row_offsets, const int64_t* bases,
                             int* column_indices, void* values, sputnik_hip_stream_t stream);

/* The instance count and fill run for a call of this shape; both entries take their
 * decisions from the same function this reports, and from nothing else.
 *   elements_per_lane    elements of one 16-byte load: 16 / element_bytes
 *   rows_per_wave        16 / 8 / 4 / 2 / 1: a group of 64 / rows_per_wave lanes walks a row,
 *                        (64 / rows_per_wave) * elements_per_lane columns per step; the most
 *                        rows whose group still covers n columns in one step, i.e. it halves
 *                        above n = 4, 8, 16 and 32 times elements_per_lane
 *   rows_per_workgroup   4 waves: 4 * rows_per_wave
 *   grid                 masks * ceil(m / rows_per_workgroup) workgroups of 256 threads
 * Host only, launches nothing; any output pointer may be NULL.  Returns
 * SPUTNIK_HIP_INVALID_ARGUMENT where the entries would for these sizes. */
SPUTNIK_HIP_API int sputnik_hip_dense_to_csr_launch_shape(int masks, int m, int n, int element_bytes,
                             int* rows_per_wave, int* elements_per_lane,
                             int* rows_per_workgroup, int* grid);

/* row_indices [masks][m] (int32): the rows of each mask by ascending length
 * row_offsets[i][r + 1] - row_offsets[i][r], ties by ascending row -- exactly
 * torch.argsort(lengths, stable=True), the reference's diffsort (modules/spmm.py:4-6).
 * row_offsets [masks][m + 1] may come from anywhere (phase 1, a transpose).  ONE launch for all
 * masks, one workgroup per mask sorting the unique 64-bit keys (length, row) in LDS; nothing
 * on the host depends on the data, so the launch can be captured in a graph.  `n` bounds no
 * length (every int32 length fits the key); it is validated only.  Serves m <= 16384:
 * SPUTNIK_HIP_INVALID_ARGUMENT beyond, and for a negative size or a NULL pointer. */
SPUTNIK_HIP_API int sputnik_hip_csr_row_order(int masks, int m, int n, const int* row_offsets,
                             int* row_indices, sputnik_hip_stream_t stream);

/* Whether sputnik_hip_csr_row_order serves a call of this shape, and with which instance; the
 * entry takes its decisions from the same function this reports, and from nothing else.
 *   served      1 for m <= 16384, else 0 (the other fields are -1 then)
 *   capacity    keys the instance holds in LDS: 2048 (m <= 2048) or 16384
 *   threads     its workgroup: 256 or 1024
 *   sort_size   keys the network sorts: the power of two at or above m
 * Host only, launches nothing; any output pointer may be NULL.  Returns
 * SPUTNIK_HIP_INVALID_ARGUMENT for a negative size. */
SPUTNIK_HIP_API int sputnik_hip_csr_row_order_route(int masks, int m, int n, int* served,
                             int* capacity, int* threads, int* sort_size);

/* ------------------------------------------------------------------------
 * Top-k selection over a dense floating matrix, written straight out as a CSR topology:
 * magnitude pruning and the regrowth step of SET / RigL (topology.magnitude_prune,
 * SparseLinear.update_topology).
 *
 * `scores` is m x n elements of `element_bytes` = 2 (float16, bfloat16) or 4 (float32),
 * element (r, c) at scores + r * row_stride + c (elements; row_stride >= 0).  An element's
 * KEY is its bit pattern with the sign bit cleared, read as an unsigned integer: ranking by
 * key is ranking by |x|; -0.0 and 0.0 tie, denormals rank by their bits whatever the float
 * unit's denormal mode, inf ranks above every finite value and NaN above inf.
 *   total_mode = 0   every row keeps its `count` (0 <= count <= n) largest keys, ties to the
 *                    lowest column
 *   total_mode = 1   the matrix keeps its `count` (0 <= count <= m * n) largest keys, ties to
 *                    the lowest flat (row-major) index
 * Exactly that many elements are kept; zeros are kept where the count demands it.
 *
 * Outputs (device): row_offsets [m + 1], row_indices [m] (the rows by ascending length, ties by
 * row), column_indices [nonzeros] ascending inside a row, nonzeros = m * count or count; and,
 * `values` not NULL, values [nonzeros]: the elements of `values_from` (m x n elements of
 * `value_bytes` = 2 or 4, row stride `values_row_stride`) at the kept positions, bit for bit.
 * Every size is known before the first launch: the call never synchronises.
 *
 * Launches: per row, one select launch (an MSB-first radix select with 8-bit digits per row,
 * histograms in LDS) and the fill.  Total: a clear of the 256-bin histograms in `workspace`
 * (on the stream), one histogram launch per digit (integer atomic adds, so the result does
 * not depend on their order), a rows launch, a scan launch, the fill and the row order.
 * `workspace`: sputnik_hip_topk_to_csr_workspace_bytes(m, n, total_mode) bytes, 4-byte
 * aligned, the call's own until its launches have run (it need not be cleared).
 *
 * SPUTNIK_HIP_INVALID_ARGUMENT: an element width other than 2 / 4, a negative size or stride,
 * m * n above INT_MAX, a count out of range, total mode with more rows than
 * sputnik_hip_csr_row_order serves (16384), a missing or misaligned pointer, a workspace too
 * small.
 * ---------------------------------------------------------------------- */
SPUTNIK_HIP_API int sputnik_hip_topk_to_csr(int m, int n, const void* scores, int element_bytes,
                             int64_t row_stride, int total_mode, int64_t count,
                             const void* values_from, int value_bytes, int64_t values_row_stride,
                             void* workspace, size_t workspace_bytes, int* row_indices,
                             int* row_offsets, int* column_indices, void* values,
                             sputnik_hip_stream_t stream);

SPUTNIK_HIP_API size_t sputnik_hip_topk_to_csr_workspace_bytes(int m, int n, int total_mode);

/* The instance sputnik_hip_topk_to_csr runs for a call of this shape; the entry takes its
 * decisions from the same function this reports, and from nothing else.
 *   served               1, or 0 in total mode with m above 16384 (the row-order limit; per-row
 *                        mode has rows of equal length and needs no sort)
 *   rows_per_wave, elements_per_lane, rows_per_workgroup, grid
 *                        the walk of every launch over the matrix: that of
 *                        sputnik_hip_dense_to_csr_launch_shape(1, m, n, element_bytes)
 *   digit_passes         8-bit digits of a key: 2 or 4
 * Host only, launches nothing; any output pointer may be NULL.  Returns
 * SPUTNIK_HIP_INVALID_ARGUMENT where the entry would for these sizes. */
SPUTNIK_HIP_API int sputnik_hip_topk_to_csr_launch_shape(int m, int n, int element_bytes, int total_mode,
                             int* served, int* rows_per_wave, int* elements_per_lane,
                             int* rows_per_workgroup, int* digit_passes, int* grid);

/* ------------------------------------------------------------------------
 * A uniformly random CSR topology with its initial values, drawn on the device
 * (topology.random_csr, SparseLinear.random): how a sparse layer starts when there is no
 * trained dense weight (SET, RigL).  It is sputnik_hip_topk_to_csr over a key matrix that is
 * never stored.  With the Philox4x32-10 and the state of "Attention dropout" above (the
 * offset a multiple of 4), replica = row and entry = column:
 *   w        = philox(key (seed lo, seed hi), counter (offset/4 lo, offset/4 hi, c >> 2, r))
 *   key(r,c) = w[c & 3] & key_mask                key_mask <= 0x7fffffff; 0x7fffffff in use,
 *                                                 smaller masks force ties (tests)
 *   total_mode = 0   every row keeps its `count` (0 <= count <= n) largest keys, ties to the
 *                    lowest column
 *   total_mode = 1   the matrix keeps its `count` (0 <= count <= m * n) largest keys, ties to
 *                    the lowest flat (row-major) index
 * Exactly that many positions are kept.  The value of a kept position:
 *   v          = philox(..., counter (offset/4 lo, offset/4 hi, c >> 2, r | 0x80000000))
 *   q          = int(v[c & 3] >> 8) - 2^23                       in [-2^23, 2^23)
 *   value(r,c) = float32(q) * scale                              one conversion, one multiply
 * rounded to nearest even into `dtype` (SPUTNIK_HIP_F32 / F16 / BF16): uniform on
 * [-bound, bound) for scale = float32(bound / 2^23).
 *
 * Outputs (device): row_offsets [m + 1], row_indices [m], column_indices [nonzeros] ascending
 * inside a row and values [nonzeros], nonzeros = m * count or count, as
 * sputnik_hip_topk_to_csr writes them; `rng_state_out` (may be NULL), int64 [2], receives the
 * {seed, offset} the call resolved -- a call whose state points at it draws the same pattern.
 * Every size is known before the first launch: the call never synchronises and is captured
 * into a graph whole.
 *
 * Launches: per row ONE (a row's lanes select it in LDS, fill it and write its offset and its
 * place in the row order).  Total: nine -- the clear, four digit passes, the rows launch, the
 * scan, the fill, the row order.  A count of 0 launches no selection.  `workspace`:
 * sputnik_hip_random_csr_workspace_bytes(m, n, total_mode) bytes (0 per row), 4-byte aligned.
 *
 * SPUTNIK_HIP_INVALID_ARGUMENT: a negative size, m * n above INT_MAX, a count out of range,
 * total mode with more than 16384 rows, a key_mask above 0x7fffffff, an unknown dtype, a
 * missing or misaligned pointer, a workspace too small.
 * ---------------------------------------------------------------------- */
SPUTNIK_HIP_API int sputnik_hip_random_csr(int m, int n, int total_mode, int64_t count, int dtype,
                             float scale, unsigned key_mask, sputnik_hip_philox_state rng,
                             int64_t* rng_state_out, void* workspace, size_t workspace_bytes,
                             int* row_indices, int* row_offsets, int* column_indices, void* values,
                             sputnik_hip_stream_t stream);

SPUTNIK_HIP_API size_t sputnik_hip_random_csr_workspace_bytes(int m, int n, int total_mode);

/* The instance sputnik_hip_random_csr runs: served (0 in total mode above 16384 rows), the
 * walk of sputnik_hip_dense_to_csr_launch_shape(1, m, n, 4) (four generated 32-bit keys per
 * lane and step), digit_passes = 4 and the launches of a call with count > 0 (1 or 9).  Host
 * only; any output pointer may be NULL. */
SPUTNIK_HIP_API int sputnik_hip_random_csr_launch_shape(int m, int n, int total_mode, int* served,
                             int* rows_per_wave, int* elements_per_lane, int* rows_per_workgroup,
                             int* digit_passes, int* grid, int* launches);

/* ------------------------------------------------------------------------
 * Attention patterns built straight to CSR on the device (topology.AttentionPattern,
 * SparseAttention(pattern=...)): sliding and dilated windows, block-local attention, summary
 * columns, global tokens, random blocks and the causal form of each, with no dense mask.
 *
 * The rule.  A pattern over m query rows and n key columns with an integer `offset`: row r
 * sits at position p = r + offset, and d = c - p.  Entry (r, c), 0 <= r < m, 0 <= c < n, is
 * kept iff (not causal or d <= 0) and at least one component keeps it:
 *   window    -window_left <= d <= window_right and d mod dilation == 0 (floor-mod);
 *             window_left = left * dilation and window_right = right * dilation, the products
 *             formed by the caller and clamped to 2^33 (beyond every |d|), as a dilation
 *             above 2^33 is.  window_left < 0: no window.
 *   block     c / block == p / block in floor division (a negative p matches no column);
 *             block = 0: none
 *   summary   c mod summary_stride >= summary_first, summary_first = stride - width;
 *             summary_stride = 0: none
 *   global    flag[c] != 0, or, with global_rows, 0 <= p < n and flag[p] != 0 (a full row);
 *             global_flags: n bytes on the device, 4-byte aligned; NULL: none
 *   random    key(r / random_block, c / random_block) < random_threshold (0 .. 2^31) with
 *             key(R, C) = philox(key (seed lo, seed hi), counter (offset/4 lo, offset/4 hi,
 *             C >> 2, R))[C & 3] & 0x7fffffff: the key stream of sputnik_hip_random_csr under
 *             the state `rng` (the offset a multiple of 4); random_block = 0: none
 * Columns ascend inside a row and an entry appears once however many components keep it.  A
 * row without an entry is legal.
 *
 * sputnik_hip_attention_pattern_count writes row_offsets [m + 1] and nonzeros [1] (device):
 * one rows launch -- a group of lanes walks a row in steps of group_lanes * 4 columns, a lane
 * evaluates the rule at its 4 consecutive columns; the flag vector is the only memory it
 * reads -- and the scan of sputnik_hip_dense_to_csr_count.  With random blocks the resolved
 * {seed, offset} goes to rng_state_out (int64 [2], may be NULL).  The caller reads nonzeros
 * back, allocates column_indices [nonzeros], and sputnik_hip_attention_pattern_fill, given the
 * same rule and state, writes them (the same walk, the slots by wave ballots) and row_indices
 * [m] (sputnik_hip_csr_row_order): four launches and one synchronisation in all.  Nothing of
 * size m * n exists.  m = 0 and n = 0 give empty results.
 *
 * Served (sputnik_hip_attention_pattern_launch_shape, host only, any output pointer may be
 * NULL): m <= 16384 (the row order's limit), m * n <= INT_MAX and |offset| < 2^30; the fields
 * behind `served` -- the rows of a wave, the columns of a lane and step (4), the rows of a
 * workgroup, the grid of the rows launches and the launches of a build (4) -- are -1 where it
 * does not serve.
 *
 * SPUTNIK_HIP_INVALID_ARGUMENT: a negative size, a shape that is not served, a rule with a
 * field outside its range, a missing or misaligned pointer.  (A rule without a component keeps
 * nothing.)
 * ---------------------------------------------------------------------- */
typedef struct sputnik_hip_attention_pattern_args {
  int64_t offset;
  int64_t window_left;
  int64_t window_right;
  int64_t dilation;
  int block;
  int summary_stride;
  int summary_first;
  int random_block;
  unsigned random_threshold;
  int causal;
  int global_rows;
  const unsigned char* global_flags;
} sputnik_hip_attention_pattern_args;

SPUTNIK_HIP_API int sputnik_hip_attention_pattern_launch_shape(int m, int n, int64_t offset, int* served,
                             int* rows_per_wave, int* columns_per_lane, int* rows_per_workgroup,
                             int* grid, int* launches);

SPUTNIK_HIP_API int sputnik_hip_attention_pattern_count(int m, int n,
                             const sputnik_hip_attention_pattern_args* pattern,
                             sputnik_hip_philox_state rng, int64_t* rng_state_out, int* row_offsets,
                             int* nonzeros, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_attention_pattern_fill(int m, int n,
                             const sputnik_hip_attention_pattern_args* pattern,
                             sputnik_hip_philox_state rng, int nonzeros, const int* row_offsets,
                             int* row_indices, int* column_indices, sputnik_hip_stream_t stream);

/* ------------------------------------------------------------------------
 * Per-row drop-and-grow of a CSR topology (topology.regrow_per_row,
 * SparseLinear.update_topology(..., per_row=True)): every row keeps its length, drops its
 * entries of smallest magnitude and grows as many where a dense score matrix is largest.
 *
 * Inputs (device): the pattern of an m x n matrix -- row_offsets [m + 1], column_indices
 * [nonzeros], ascending inside a row, int32 --, values [nonzeros] of `value_bytes` = 2 or 4,
 * drop_counts [m] (int32) and `scores`, m x n elements of `score_bytes` = 2 (float16, bfloat16)
 * or 4 (float32), element (r, c) at scores + r * scores_row_stride + c (elements; stride >= 0).
 * KEYS are those of sputnik_hip_topk_to_csr: the bit pattern without the sign.  For row r of
 * len_r entries, d_r = clamp(drop_counts[r], 0, len_r) and c_r = len_r - d_r:
 *   Kept_r    the c_r entries of largest value key, ties to the lower column
 *   Grown_r   the d_r columns outside Kept_r of largest score key, ties to the lowest column;
 *             a score key is clamped to `score_key_limit` (the key of the dtype's largest
 *             finite value: 0x7f7fffff float32, 0x7bff float16, 0x7f7f bfloat16 -- NaN and inf
 *             count as that value).  Columns dropped in this call are eligible.
 * The new row is Kept_r and Grown_r in ascending column order in the row's own slots
 * [row_offsets[r], row_offsets[r + 1]): out_column_indices [nonzeros]; out_values [nonzeros]:
 * a kept entry's old value bit for bit, all bits zero for a grown one; out_source [nonzeros]
 * (int64): a kept entry's old index, -1 for a grown one.  row_offsets is not written.
 *
 * ONE launch, one group of lanes per row: a radix select over the row's old values, the old and
 * the kept columns marked in an LDS bitmap, a radix select over the score row outside the kept
 * columns, and the fill, in which a running count of old bits is the old entry index.  Every
 * count is an integer and every store a vector store to a slot one lane owns: two calls give
 * equal arrays.  Nothing is read back; `workspace` is
 * sputnik_hip_csr_regrow_workspace_bytes(...) bytes (0 today: it may be NULL).
 * m = 0 or nonzeros = 0 launches nothing.  A column index outside 0 .. n - 1, a column stored
 * twice or offsets that do not ascend inside 0 .. nonzeros are caller errors with an
 * unspecified result, but nothing outside the arrays is read or written.
 *
 * SPUTNIK_HIP_INVALID_ARGUMENT: an element width other than 2 / 4, a negative size or stride,
 * m * n above INT_MAX, n above the served limit (sputnik_hip_csr_regrow_launch_shape), a
 * missing or misaligned pointer, a workspace too small.
 * ---------------------------------------------------------------------- */
SPUTNIK_HIP_API int sputnik_hip_csr_regrow(int m, int n, int nonzeros, const int* row_offsets,
                             const int* column_indices, const void* values, int value_bytes,
                             const int* drop_counts, const void* scores, int score_bytes,
                             int64_t scores_row_stride, unsigned score_key_limit, void* workspace,
                             size_t workspace_bytes, int* out_column_indices, void* out_values,
                             int64_t* out_source, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API size_t sputnik_hip_csr_regrow_workspace_bytes(int m, int n, int nonzeros);

/* The instance sputnik_hip_csr_regrow runs for a call of this shape; the entry takes its
 * decisions from the same function this reports, and from nothing else.
 *   served               1 for n <= max_n, else 0 (every field but max_n is -1 then)
 *   max_n                the widest row served: 4 rows per workgroup, each with a 256-bin
 *                        histogram and two bits per column, in the 64 KiB of LDS a launch gets
 *                        without asking for more: 32 * ((65536 / 4 - 1024) / 8) = 61440
 *   elements_per_lane    score elements of one 16-byte load: 16 / score_bytes
 *   rows_per_wave        8 / 4 / 2 / 1: that of sputnik_hip_dense_to_csr_launch_shape(1, m, n,
 *                        score_bytes), but at most 8 (64 rows of histogram and bitmap do not
 *                        fit 64 KiB)
 *   rows_per_workgroup   4 waves: 4 * rows_per_wave
 *   value_digit_passes, score_digit_passes
 *                        8-bit digits of a value key and of a score key: the element bytes
 *   lds_bytes            dynamic LDS of the launch: rows_per_workgroup * (1024 + 8 * ceil(n / 32))
 *   grid                 ceil(m / rows_per_workgroup) workgroups of 256 threads
 * Host only, launches nothing; any output pointer may be NULL.  Returns
 * SPUTNIK_HIP_INVALID_ARGUMENT for a negative size, an element width other than 2 / 4 and
 * m * n above INT_MAX. */
SPUTNIK_HIP_API int sputnik_hip_csr_regrow_launch_shape(int m, int n, int score_bytes, int value_bytes,
                             int* served, int* rows_per_wave, int* elements_per_lane,
                             int* rows_per_workgroup, int* value_digit_passes,
                             int* score_digit_passes, int* lds_bytes, int* max_n, int* grid);

/* ------------------------------------------------------------------------
 * Matrix-wide drop-and-grow of a CSR topology (topology.regrow_total,
 * SparseLinear.update_topology / rigl_update with per_row=False): the layer-wise rule of SET and
 * RigL.  The number of entries stays, the row lengths change.
 *
 * Inputs (device): the pattern, values and scores of sputnik_hip_csr_regrow, and a HOST count
 * `drop` = d, 0 <= d <= nonzeros.  KEYS are those of sputnik_hip_topk_to_csr.
 *   Kept    the nonzeros - d entries of largest value key, ties to the lower entry index
 *   Grown   the d positions outside Kept of largest score key, ties to the lower flat (row-major)
 *           index; a score key is clamped to `score_key_limit` as in sputnik_hip_csr_regrow.
 *           Positions dropped in this call are eligible.
 * Outputs (device): the CSR pattern of Kept and Grown, exactly `nonzeros` entries:
 * out_row_offsets [m + 1], out_row_indices [m] (the rows by ascending new length, ties by row),
 * out_column_indices [nonzeros] ascending inside a row, out_values [nonzeros] (a kept entry's old
 * value bit for bit, all bits zero for a grown one), out_source [nonzeros] (int64: a kept entry's
 * old index, -1 for a grown one).  d = 0 reproduces the pattern.
 *
 * Every size is known up front: the call enqueues its launches, reads nothing back and can be
 * captured in a graph.  Launches (sputnik_hip_csr_regrow_total_launch_shape counts them): a clear
 * launch for the bins of both selections; over the flat values array the digit launches, the
 * rows launch and the scan of sputnik_hip_csr_topk's total mode with count nonzeros - d; a planes
 * launch that marks every row's old and kept columns in two bit planes (built in LDS, written to
 * the workspace by the lanes that own the row); over the dense score rows one digit launch per
 * score digit with the kept plane as a mask and the keys clamped, a rows launch and the scan that
 * gives the new offsets; the fill; the row order.  All counting is integer, every store a vector
 * store to a slot one lane owns: two calls give equal arrays.  `workspace`:
 * sputnik_hip_csr_regrow_total_workspace_bytes(...) bytes, 4-byte aligned, the call's own until
 * its launches have run (it need not be cleared): two sets of 4 x 256 bins, thresholds, quotas
 * and tie counts per row, the kept lengths, and the planes, 2 * m * ceil(n / 32) words.
 * m = 0 or nonzeros = 0 writes the zero offsets and the row order and nothing else.  A column
 * index outside 0 .. n - 1, a column stored twice or offsets that do not ascend inside
 * 0 .. nonzeros are caller errors with an unspecified result, but nothing outside the arrays is
 * read or written.
 *
 * SPUTNIK_HIP_INVALID_ARGUMENT, before any launch: an element width other than 2 / 4, a negative
 * size or stride, d outside 0 .. nonzeros, m above 16384 (the row order and the scan), n above
 * 65536 (the LDS planes), m * n above INT_MAX, a missing or misaligned pointer, a workspace too
 * small.
 * ---------------------------------------------------------------------- */
SPUTNIK_HIP_API int sputnik_hip_csr_regrow_total(int m, int n, int nonzeros, const int* row_offsets,
                             const int* column_indices, const void* values, int value_bytes,
                             int64_t drop, const void* scores, int score_bytes,
                             int64_t scores_row_stride, unsigned score_key_limit, void* workspace,
                             size_t workspace_bytes, int* out_row_indices, int* out_row_offsets,
                             int* out_column_indices, void* out_values, int64_t* out_source,
                             sputnik_hip_stream_t stream);

SPUTNIK_HIP_API size_t sputnik_hip_csr_regrow_total_workspace_bytes(int m, int n, int nonzeros);

/* The instances sputnik_hip_csr_regrow_total runs for a call of this shape; the entry takes its
 * decisions from the same function this reports, and from nothing else.
 *   served               1 for m <= max_m and n <= max_n, else 0 (every field but the two limits
 *                        is -1 then)
 *   max_m                16384: the rows sputnik_hip_csr_row_order and the scan serve
 *   max_n                65536: four rows per workgroup, two bits per column each, in the 64 KiB
 *                        of LDS the planes launch gets without asking for more
 *   rows_per_wave, elements_per_lane, rows_per_workgroup, grid
 *                        the walk of every launch over the score rows (and of the planes launch):
 *                        that of sputnik_hip_dense_to_csr_launch_shape(1, m, n, score_bytes)
 *   value_digit_passes, score_digit_passes
 *                        8-bit digits of a value key and of a score key: the element bytes
 *   lds_bytes            dynamic LDS of the planes launch: rows_per_workgroup * 8 * ceil(n / 32)
 *   value_rows_per_wave, value_rows_grid, flat_grid
 *                        the launches over the old entries: rows_per_wave, rows_grid and flat_grid
 *                        of sputnik_hip_csr_topk_launch_shape(m, n, nonzeros, value_bytes, 1)
 *   launches             kernels one call enqueues: 8 + value_digit_passes + score_digit_passes;
 *                        1 (the row order) for nonzeros = 0, 0 for m = 0
 * Host only, launches nothing; any output pointer may be NULL.  Returns
 * SPUTNIK_HIP_INVALID_ARGUMENT for a negative size, an element width other than 2 / 4 and
 * m * n above INT_MAX. */
SPUTNIK_HIP_API int sputnik_hip_csr_regrow_total_launch_shape(int m, int n, int nonzeros, int score_bytes,
                             int value_bytes, int* served, int* rows_per_wave, int* elements_per_lane,
                             int* rows_per_workgroup, int* value_digit_passes, int* score_digit_passes,
                             int* lds_bytes, int* max_m, int* max_n, int* grid,
                             int* value_rows_per_wave, int* value_rows_grid, int* flat_grid,
                             int* launches);

/* ------------------------------------------------------------------------
 * Drop-and-grow of a CSR topology under random scores that are never stored
 * (topology.regrow_per_row_random / regrow_total_random, SparseLinear.set_update): the step of
 * SET (Mocanu et al. 2018), without an [m, n] array.
 *
 * THE RULE.  With the Philox4x32-10 and the state {seed, offset} of "Attention dropout" above
 * (the offset a multiple of 4), replica = row and entry = column, as in sputnik_hip_random_csr:
 *   key(r,c) = philox(key (seed lo, seed hi), counter (offset/4 lo, offset/4 hi, c >> 2, r))[c & 3]
 *              & key_mask                          key_mask <= 0x3fffffff (30 bits); 0x3fffffff in
 *                                                  use, smaller masks force ties (tests)
 * A masked key read as float32 bits is a finite, non-negative number, so the clamp of the
 * regrow rule to the largest finite score never acts: the step is EXACTLY
 * sputnik_hip_csr_regrow (sputnik_hip_csr_regrow_total) under dense float32 scores whose bit
 * patterns are key(r, c).  Kept entries, the tie rule (lowest column per row, lowest flat index
 * matrix-wide), the eligibility of dropped positions, ascending columns, out_source and (matrix-
 * wide) the row order are those of that contract.  A grown entry's value:
 *   grow_values = 0   all bits zero (+0.0), as the stored-score steps write it (RigL's choice)
 *   grow_values = 1   value(r, c) of sputnik_hip_random_csr under scale = grow_scale:
 *                     float32(int(v[c & 3] >> 8) - 2^23) * grow_scale with v from the value
 *                     stream (r | 0x80000000 in the counter), rounded to nearest even into
 *                     `dtype`: uniform on [-bound, bound) for grow_scale = float32(bound / 2^23)
 *                     (SET re-initialises what it grows)
 * out_source is -1 for a grown entry either way.
 *
 * The arguments are those of sputnik_hip_csr_regrow / sputnik_hip_csr_regrow_total with the
 * score pointer, width, stride and key limit replaced by the Philox arguments of
 * sputnik_hip_random_csr, the mask and the grow flag and scale; the values are given by `dtype`
 * (SPUTNIK_HIP_F32 / F16 / BF16), which says how a grown value is rounded.  `rng_state_out` (may
 * be NULL), int64 [2], receives the {seed, offset} the call resolved, written by one lane of
 * one launch (the per-row kernel, the matrix-wide fill; a call without entries launches one lane
 * for it).  The launches are those of the stored-score steps, the score half instantiated on
 * generated keys: per row ONE, matrix-wide 8 + value digits + 4.  A key is recomputed per pass
 * and never stored: per four columns of a row 5 Philox calls per row, 6 matrix-wide, and one
 * more of the value stream where a piece grows an entry under grow_values = 1.  Nothing is read
 * back: a call is captured into a graph whole, and with a state that points into the device
 * generator every replay draws new scores.  `workspace`:
 * sputnik_hip_csr_regrow_random_workspace_bytes(m, n, nonzeros, total_mode) bytes (0 per row,
 * sputnik_hip_csr_regrow_total_workspace_bytes matrix-wide), 4-byte aligned.
 *
 * SPUTNIK_HIP_INVALID_ARGUMENT: what the stored-score entry returns it for at 4-byte scores (per
 * row n above 61440; matrix-wide m above 16384 or n above 65536), an unknown dtype, a key_mask
 * above 0x3fffffff, grow_values != 0 with a grow_scale that is negative or not finite.
 * ---------------------------------------------------------------------- */
SPUTNIK_HIP_API int sputnik_hip_csr_regrow_random(int m, int n, int nonzeros, const int* row_offsets,
                             const int* column_indices, const void* values, int dtype,
                             const int* drop_counts, sputnik_hip_philox_state rng,
                             int64_t* rng_state_out, unsigned key_mask, int grow_values,
                             float grow_scale, void* workspace, size_t workspace_bytes,
                             int* out_column_indices, void* out_values, int64_t* out_source,
                             sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_csr_regrow_total_random(int m, int n, int nonzeros, const int* row_offsets,
                             const int* column_indices, const void* values, int dtype, int64_t drop,
                             sputnik_hip_philox_state rng, int64_t* rng_state_out, unsigned key_mask,
                             int grow_values, float grow_scale, void* workspace,
                             size_t workspace_bytes, int* out_row_indices, int* out_row_offsets,
                             int* out_column_indices, void* out_values, int64_t* out_source,
                             sputnik_hip_stream_t stream);

SPUTNIK_HIP_API size_t sputnik_hip_csr_regrow_random_workspace_bytes(int m, int n, int nonzeros,
                             int total_mode);

/* The instances the two entries above run: total_mode = 0 reports
 * sputnik_hip_csr_regrow_launch_shape(m, n, 4, value_bytes), total_mode = 1
 * sputnik_hip_csr_regrow_total_launch_shape(m, n, nonzeros, 4, value_bytes) -- the walk of
 * sputnik_hip_dense_to_csr_launch_shape(1, m, n, 4), four generated 32-bit keys per lane and
 * step, score_digit_passes = 4.
 *   served     per row: n <= max_n = 61440; matrix-wide: m <= max_m = 16384 and n <= max_n =
 *              65536 (max_m is -1 per row: no limit of its own); the other fields are -1 where
 *              the shape is not served
 *   launches   kernels of one call that publishes its state: per row 1; matrix-wide
 *              8 + value_digit_passes + 4, and without entries the row order (m > 0) plus the
 *              lane that publishes the state
 * Host only, launches nothing; any output pointer may be NULL.  Returns
 * SPUTNIK_HIP_INVALID_ARGUMENT for a negative size, a value width other than 2 / 4, a
 * total_mode other than 0 / 1 and m * n above INT_MAX. */
SPUTNIK_HIP_API int sputnik_hip_csr_regrow_random_launch_shape(int m, int n, int nonzeros, int value_bytes,
                             int total_mode, int* served, int* rows_per_wave, int* elements_per_lane,
                             int* rows_per_workgroup, int* value_digit_passes, int* score_digit_passes,
                             int* lds_bytes, int* max_m, int* max_n, int* grid, int* launches);

/* ------------------------------------------------------------------------
 * Top-k over the entries of a CSR pattern, written out as a smaller CSR pattern
 * (topology.prune_csr, SparseLinear.prune_to): gradual magnitude pruning of a layer that has
 * no dense weight any more.
 *
 * Inputs (device): the pattern of an m x n matrix -- row_offsets [m + 1], column_indices
 * [nonzeros], ascending inside a row, int32 -- and values [nonzeros] of `value_bytes` = 2 or 4.
 * KEYS are those of sputnik_hip_topk_to_csr: the bit pattern without the sign.  Among equal
 * keys the lower entry index wins (the lower column inside a row, the lower flat index across
 * rows).
 *   total_mode = 1   the `count` (0 <= count <= nonzeros) entries of largest key are kept
 *   total_mode = 0   row r of len_r entries keeps its min(len_r, count) entries of largest key
 *                    (0 <= count <= n)
 * Outputs (device): out_row_offsets [m + 1]; out_row_indices [m] (the rows by ascending new
 * length, ties by row); and for every kept entry, in the order of the old arrays:
 * out_column_indices, out_values (the old value bit for bit) and out_source (int64: its index in
 * the old arrays; it ascends).  The three hold `out_capacity` entries; a slot at or beyond it
 * is not written.  n enters the argument check alone.
 *
 * Total mode: the new size is `count`, known up front (out_capacity >= count): one call that
 * never synchronises and can be captured in a graph.  Launches: a clear launch for the 256-bin
 * histograms in `workspace` (a kernel: every replay of a captured call clears them), one
 * histogram launch per digit over the FLAT values array (16-byte loads, LDS histogram, integer
 * atomic adds into the global bins), a rows launch that counts the entries above and at the
 * threshold, a scan launch (offsets, the rows' shares of the tie quota), the fill, the row order.
 * Per-row mode: the new size sum min(len_r, count) is on the device.  A caller that has room
 * for `nonzeros` entries makes one call.  A caller that wants the size first makes two, as
 * with sputnik_hip_dense_to_csr_count / _fill:
 *   out_column_indices == NULL   out_row_offsets (one scan launch) and out_row_indices only;
 *                                out_row_offsets[m] is the size
 *   out_row_indices == NULL      the fill alone, under the out_row_offsets the former call wrote
 * The fill is ONE launch: the group of lanes that walks a row's entries selects the row's
 * threshold (histogram in LDS) and places the kept entries by wave ballot.
 * A row's entries are walked in 16-byte pieces by a group of 64 / rows_per_wave lanes
 * (sputnik_hip_csr_topk_launch_shape: from the mean row length nonzeros / m); a longer row
 * takes more steps, any length is served.  Every count is an integer and every store a vector
 * store to a slot one lane owns: two calls give equal arrays.  `workspace`:
 * sputnik_hip_csr_topk_workspace_bytes(...) bytes (0 per row: it may be NULL), 4-byte aligned,
 * the call's own until its launches have run.
 * m = 0, nonzeros = 0 and count = 0 write the zero offsets and the row order and nothing else.
 * Offsets that do not ascend inside 0 .. nonzeros are a caller error with an unspecified result,
 * but nothing outside the arrays is read or written.
 *
 * SPUTNIK_HIP_INVALID_ARGUMENT: a value width other than 2 / 4, a negative size, a count out of
 * range, m above the rows sputnik_hip_csr_row_order serves (16384), out_capacity below count
 * (total mode), a missing or misaligned pointer, a workspace too small.
 * ---------------------------------------------------------------------- */
SPUTNIK_HIP_API int sputnik_hip_csr_topk(int m, int n, int nonzeros, const int* row_offsets,
                             const int* column_indices, const void* values, int value_bytes,
                             int total_mode, int64_t count, void* workspace, size_t workspace_bytes,
                             int* out_row_indices, int* out_row_offsets, int* out_column_indices,
                             void* out_values, int64_t* out_source, int64_t out_capacity,
                             sputnik_hip_stream_t stream);

SPUTNIK_HIP_API size_t sputnik_hip_csr_topk_workspace_bytes(int m, int n, int nonzeros, int total_mode);

/* The instance sputnik_hip_csr_topk runs for a call of this shape; the entry takes its
 * decisions from the same function this reports, and from nothing else.
 *   served               1, or 0 for m above 16384 (the row-order limit; every other field is
 *                        -1 then)
 *   elements_per_lane    values of one 16-byte load: 16 / value_bytes
 *   rows_per_wave        16 / 8 / 4 / 2 / 1: the most whose group of lanes covers a row of the
 *                        mean length nonzeros / m (integer division; 0 for m = 0) in one step
 *   group_lanes          64 / rows_per_wave; one step covers group_lanes * elements_per_lane
 *                        entries
 *   rows_per_workgroup   4 waves: 4 * rows_per_wave
 *   digit_passes         8-bit digits of a key: the value bytes
 *   rows_grid            ceil(m / rows_per_workgroup) workgroups of 256 threads: every launch
 *                        that walks rows
 *   flat_grid            total mode: workgroups of a digit pass over the flat values array,
 *                        ceil((nonzeros / elements_per_lane + 2) / (8 * 256)); 0 per row and
 *                        for nonzeros = 0
 * Host only, launches nothing; any output pointer may be NULL.  Returns
 * SPUTNIK_HIP_INVALID_ARGUMENT for a negative size, a value width other than 2 / 4 and a
 * total_mode other than 0 / 1. */
SPUTNIK_HIP_API int sputnik_hip_csr_topk_launch_shape(int m, int n, int nonzeros, int value_bytes,
                             int total_mode, int* served, int* rows_per_wave, int* group_lanes,
                             int* elements_per_lane, int* rows_per_workgroup, int* digit_passes,
                             int* rows_grid, int* flat_grid);

/* ------------------------------------------------------------------------
 * ONE top-k across the entries of several CSR patterns, each written out as a smaller CSR
 * pattern (topology.prune_csr_global, topology.prune_layers_to): global magnitude pruning, the
 * layers of a model ranked together.
 *
 * Inputs: `layers` patterns in the caller's order.  HOST arrays of `layers` elements: rows
 * (m_l), nonzeros (nnz_l), and the DEVICE pointers row_offsets[l] [m_l + 1], column_indices[l]
 * [nnz_l] (int32, ascending inside a row) and values[l] [nnz_l], all of `value_bytes` = 2 or 4.
 * The pointer arrays are read on the host during the call and travel to the kernels as
 * arguments; nothing is copied to the device.
 * The `count` (0 <= count <= sum nnz_l) entries of largest KEY over all layers are kept; the
 * keys are those of sputnik_hip_csr_topk.  Among equal keys the entry of the lower layer wins,
 * then the lower entry index.  With layers = 1 the result is sputnik_hip_csr_topk's in total
 * mode.
 *
 * How many entries a layer keeps is on the device, so the call has two halves around ONE read
 * of out_nonzeros, whatever `layers` is:
 *   _select   a clear launch for the 256-bin histograms in `workspace` (a kernel, as in
 *             sputnik_hip_csr_topk); per digit, one launch per `layers_per_launch` layers over
 *             their FLAT values arrays -- a workgroup finds its layer and its pieces in a table
 *             among its arguments, and every launch adds into the same bins; per layer a rows
 *             launch (entries above and at the one threshold) and, in layer order, a scan
 *             launch that hands the layer its share of the tie quota (what the layers in front
 *             left of it), writes out_row_offsets[l] [m_l + 1] and out_nonzeros[l].
 *             out_nonzeros: device, int32 [layers].  Never synchronises.
 *   _fill     with out_capacity[l] (host) = the out_nonzeros[l] read back: per layer the fill of
 *             out_column_indices[l], out_values[l] (the old value bit for bit) and out_source[l]
 *             (int64: the index in the layer's old arrays; it ascends), out_capacity[l] entries
 *             each -- a slot at or beyond it is not written --, and the row order
 *             out_row_indices[l] [m_l] of out_row_offsets[l].  A layer with out_capacity[l] = 0
 *             takes no fill launch and its three pointers may be NULL.
 * Both halves take the same layers, the same `workspace`
 * (sputnik_hip_csr_topk_global_workspace_bytes(layers, rows) bytes, 4-byte aligned, the call's
 * own from _select until _fill's launches have run) and the same out_row_offsets.
 * Every count is an integer and every store a vector store to a slot one lane owns: two calls
 * give equal arrays.  A layer may have no rows or no entries, and may keep none.
 * Offsets that do not ascend inside 0 .. nnz_l are a caller error with an unspecified result,
 * but nothing outside the arrays is read or written.
 *
 * SPUTNIK_HIP_INVALID_ARGUMENT: a value width other than 2 / 4, a negative size, a count out of
 * range, a layer of more rows than sputnik_hip_csr_row_order serves (16384), sum nnz_l above
 * INT_MAX, an out_capacity[l] outside 0 .. nnz_l, a missing or misaligned pointer, a workspace
 * too small.
 * ---------------------------------------------------------------------- */
SPUTNIK_HIP_API int sputnik_hip_csr_topk_global_select(int layers, const int* rows, const int* nonzeros,
                             const int* const* row_offsets, const void* const* values, int value_bytes,
                             int64_t count, void* workspace, size_t workspace_bytes,
                             int* const* out_row_offsets, int* out_nonzeros, sputnik_hip_stream_t stream);

SPUTNIK_HIP_API int sputnik_hip_csr_topk_global_fill(int layers, const int* rows, const int* nonzeros,
                             const int* const* row_offsets, const int* const* column_indices,
                             const void* const* values, int value_bytes, void* workspace,
                             size_t workspace_bytes, const int64_t* out_capacity,
                             int* const* out_row_indices, int* const* out_row_offsets,
                             int* const* out_column_indices, void* const* out_values,
                             int64_t* const* out_source, sputnik_hip_stream_t stream);

/* 4 * (4 * 256 + 2 + 2 * sum rows[l]) bytes: the bins, the threshold, the ties handed out so
 * far, and per row its quota and its ties.  0 for a negative size. */
SPUTNIK_HIP_API size_t sputnik_hip_csr_topk_global_workspace_bytes(int layers, const int* rows);

/* The instance sputnik_hip_csr_topk_global_select runs for these layers (HOST arrays rows and
 * nonzeros of `layers` elements); the entries take their decisions from the same function this
 * reports, and from nothing else.
 *   served                   1, or 0 where a layer has more than 16384 rows or sum nnz_l is
 *                            above INT_MAX (every other field is -1 then)
 *   digit_passes             8-bit digits of a key: the value bytes
 *   layers_per_launch        layers one digit launch takes in its argument table (32)
 *   elements_per_workgroup   entries one workgroup of the flat walk covers: 8 * 256 16-byte
 *                            pieces = 2048 * 16 / value_bytes; layer l takes
 *                            ceil((nnz_l / (16 / value_bytes) + 2) / 2048) workgroups, none for
 *                            nnz_l = 0
 *   digit_launches           argument tables per digit: ceil(layers / layers_per_launch); a table
 *                            whose layers are all empty is not launched
 * Per layer, the rows, scan and fill launches are those sputnik_hip_csr_topk_launch_shape
 * reports for (m_l, nnz_l) in total mode.
 * Host only, launches nothing; any output pointer may be NULL.  Returns
 * SPUTNIK_HIP_INVALID_ARGUMENT for a negative size and a value width other than 2 / 4. */
SPUTNIK_HIP_API int sputnik_hip_csr_topk_global_launch_shape(int layers, const int* rows, const int* nonzeros,
                             int value_bytes, int* served, int* digit_passes, int* layers_per_launch,
                             int* elements_per_workgroup, int* digit_launches);

/*
 * out[r][i] = in[r][permutation[i]], i < n, for `rows` value arrays (strides in
 * elements) that share one permutation: the values of a static pattern in the
 * order of its transpose, given the permutation sputnik_hip_csr_transpose
 * returned once (out_permutation).  Replaces the per-backward csr_transpose of
 * modules/spmm.py:59-62, modules/sddmm.py:60-63 and
 * modules/sparse_linear.py:52-55 for topologies that do not change.
 */
SPUTNIK_HIP_API int sputnik_hip_permute_last_batched(int n, int rows, const float* in, int64_t in_stride,
                                     const int* permutation, float* out,
                                     int64_t out_stride, sputnik_hip_stream_t stream);

/*
 * The same permutation for MANY rows (attention weights: one row per batch x
 * head), through LDS.  The caller regroups the permutation once per topology by
 * the band of B = sputnik_hip_permute_band_size() consecutive SOURCE entries a
 * value comes from: `dest_list` holds the output positions i, band after band
 * (band b = list positions [b*B, min((b+1)*B, n)): exactly the positions whose
 * source permutation[i] lies in [b*B, (b+1)*B)), ascending inside a band, and
 * `source_in_band[t] = permutation[dest_list[t]] - (t / B) * B`.  (A stable sort
 * of the positions by permutation[i] / B, or one counting pass on the host.)
 *   out[r][dest_list[t]] = in[r][(t / B) * B + source_in_band[t]]
 */
SPUTNIK_HIP_API int sputnik_hip_permute_band_size(void);

SPUTNIK_HIP_API int sputnik_hip_permute_banded_batched(int n, int rows, const float* in,
                                     int64_t in_stride, const int* dest_list,
                                     const int* source_in_band, float* out,
                                     int64_t out_stride, sputnik_hip_stream_t stream);

/*
 * The library's developer / test knobs (SPUTNIK_HIP_* environment variables:
 * kernel choice for small inputs, timing experiments) are read once, at first
 * use, never on the launch path; this re-reads them.  Not to be called while
 * other threads issue launches.  (tests/conftest.py steers the parity tests
 * onto every kernel with it.)
 */
SPUTNIK_HIP_API void sputnik_hip_reload_options(void);

/*
 * Batched 2-D transpose  out[b][c][r] = in[b][r][c]  (row-major, fp32; batch
 * strides in elements).  The layout pass of the reference's modules:
 * `x.transpose(1, 2).contiguous()` in front of left_spmm
 * (modules/sparse_linear.py:89), the same behind every projection and the head
 * split / merge copies of modules/sparse_attention.py:108-126 are all this
 * operation (the head split [B, H*D, S] -> [B*H, S, D] is a transpose of B*H
 * matrices of D x S).  No workspace, no synchronisation.
 */
SPUTNIK_HIP_API int sputnik_hip_transpose_batched(int batches, int rows, int cols, const float* in,
                                  int64_t in_batch_stride, float* out,
                                  int64_t out_batch_stride,
                                  sputnik_hip_stream_t stream);

/*
 * The same with a change of storage type on the way (in_type / out_type:
 * SPUTNIK_HIP_F32 / F16 / BF16; supported: equal types, half -> float,
 * float -> half).  BASELINE.json's config 5 stores activations in fp16 while the
 * operators compute and return fp32 (src/spmm_cuda.cu:42): the widening happens
 * inside the layout pass in front of left_spmm, the narrowing of the gradient
 * inside the pass behind it -- no pass of its own.
 */
SPUTNIK_HIP_API int sputnik_hip_transpose_cast_batched(int batches, int rows, int cols, const void* in,
                                       int in_type, int64_t in_batch_stride, void* out,
                                       int out_type, int64_t out_batch_stride,
                                       sputnik_hip_stream_t stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* SPUTNIK_HIP_H_ */
