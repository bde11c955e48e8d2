// Host side of the drop-in: the reference's five operators
// (src/sputnik.cpp:36-42) registered with TORCH_LIBRARY as
// torch.ops.torch_sputnik.{spmm,left_spmm,sddmm,sparse_softmax,csr_transpose}
// for HIP tensors only, on top of the C ABI in include/sputnik_hip.h.
//
// Each op mirrors one host wrapper of the reference:
//   spmm            src/spmm_cuda.cu:9-60
//   left_spmm       src/left_replicated_spmm.cu:8-44
//   sddmm           src/sddmm_cuda.cu:7-57
//   sparse_softmax  src/softmax_cuda.cu:7-46
//   csr_transpose   src/transpose_cuda.cu:45-102
// Same argument order and meaning; differences, all on purpose:
//   - the reference's shape `assert`s (no-ops under NDEBUG) are TORCH_CHECKs,
//     so a bad call raises RuntimeError instead of being undefined;
//   - the replica loop is one launch, outputs are at::empty (every element is
//     written by the kernels) instead of torch::zeros;
//   - integer tensors may be int64 (the reference's own SparseLinear backward
//     hands an int64 row_indices to left_spmm, modules/sparse_linear.py:57-65)
//     and are cast to int32 here; non-contiguous inputs are made contiguous;
//   - a device guard on the inputs' device (the reference has none).
// There is no CPU kernel: CPU tensors raise from the dispatcher.  Autograd is
// not registered here; the Python autograd.Functions stay the callers.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <ATen/hip/HIPGeneratorImpl.h>   // at::CUDAGeneratorImpl on ROCm
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <algorithm>
#include <limits>
#include <mutex>
#include <tuple>
#include <vector>

#include "../../include/sputnik_hip.h"

namespace {

using at::Tensor;

void check_status(int status, const char* what) {
  TORCH_CHECK(status == 0, "torch_sputnik::", what, ": kernel library returned error ", status,
              status == SPUTNIK_HIP_INVALID_ARGUMENT ? " (invalid argument)" : " (hipError_t)");
}

sputnik_hip_stream_t current_stream(const Tensor& t) {
  return reinterpret_cast<sputnik_hip_stream_t>(
      c10::hip::getCurrentHIPStream(t.device().index()).stream());
}

Tensor as_index(const Tensor& t, const char* name, const Tensor& like) {
  TORCH_CHECK(t.scalar_type() == at::kInt || t.scalar_type() == at::kLong, name,
              " must be an int32 (or int64) tensor, got ", t.scalar_type());
  TORCH_CHECK(t.device() == like.device(), name, " must be on ", like.device(), ", got ",
              t.device());
  TORCH_CHECK(t.dim() == 1, name, " should have 1 dimension, got ", t.dim());
  return t.to(at::kInt).contiguous();
}

// float32 is the reference's only dtype (data_ptr<float>(), src/spmm_cuda.cu:51);
// float16 / bfloat16 STORAGE is accepted as an extension (BASELINE.json config 5
// names fp16), all arithmetic accumulates in float32.  THE RESULT-TYPE RULE, per op
// (one place that says it):
//   spmm, left_spmm, spmm_bias*, the planned / permuted / transposed-store / group
//   forms, sddmm, sddmm_sum, csr_transpose (values_t), sparse_attention*, every
//   many-mask op                         -> float32 results whatever the operand type
//                                           (the reference's rule, src/spmm_cuda.cu:42);
//   sparse_softmax, sparse_softmax_scaled, sparse_softmax_backward
//                                        -> the type of `values` (an elementwise map of
//                                           the stored values: half in, half out; float32
//                                           in, float32 out exactly as the reference);
//   sddmm_narrow                         -> the operands' (half) type, on request only;
//   transpose_last2_as                   -> the type its out_type argument names.
// Ops that take float32 only in their kernels widen half operands once with as_float
// below; the ops whose kernels read half storage natively take as_storage.  The SpMM ops
// choose per call: THE NATIVE-HALF RULE at check_spmm says which.
int type_code(at::ScalarType t) {   // -1: not a storage type of the library
  return t == at::kFloat ? SPUTNIK_HIP_F32 : t == at::kHalf ? SPUTNIK_HIP_F16
         : t == at::kBFloat16 ? SPUTNIK_HIP_BF16 : -1;
}
Tensor as_float(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU (HIP) tensor, got ", t.device());
  TORCH_CHECK(type_code(t.scalar_type()) >= 0, name, " must be float32 (or float16 / bfloat16 storage), got ",
              t.scalar_type());
  return t.to(at::kFloat).contiguous();
}

// Operands of the natively typed kernels (softmax pair, SDDMM): float32, float16 or
// bfloat16 storage is handed to the kernel as it is -- no widening copy.
Tensor as_storage(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU (HIP) tensor, got ", t.device());
  TORCH_CHECK(type_code(t.scalar_type()) >= 0, name, " must be float32, float16 or bfloat16, got ",
              t.scalar_type());
  return t.contiguous();
}

struct Topology {
  Tensor row_indices, row_offsets, column_indices;
  int nonzeros;
};

Topology check_topology(int64_t m, const Tensor& row_indices, const Tensor& row_offsets,
                        const Tensor& column_indices, const Tensor& like) {
  Topology t;
  t.row_indices = as_index(row_indices, "row_indices", like);
  t.row_offsets = as_index(row_offsets, "row_offsets", like);
  t.column_indices = as_index(column_indices, "column_indices", like);
  TORCH_CHECK(t.row_indices.size(0) + 1 == t.row_offsets.size(0),
              "row_offsets should have one more entry than row_indices, got ",
              t.row_offsets.size(0), " and ", t.row_indices.size(0));
  TORCH_CHECK(t.row_indices.size(0) == m, "number of row_indices (", t.row_indices.size(0),
              ") and m (", m, ") must match");
  TORCH_CHECK(t.column_indices.size(0) < (int64_t{1} << 31), "too many nonzeros");
  t.nonzeros = static_cast<int>(t.column_indices.size(0));
  return t;
}

int to_int(int64_t v, const char* name) {
  TORCH_CHECK(v >= 0 && v < (int64_t{1} << 31), name, " out of range: ", v);
  return static_cast<int>(v);
}

// ---- the argument contract of the topology ops (dense_to_csr ... csr_topk_global, below):
// every message names the op and the argument it turns away ----

// One CSR pattern with its values as the topology kernels read it: `values` [nnz] of a storage
// type on the GPU, row_offsets [m + 1] and column_indices [nnz] 1-D int32 on its device, all
// contiguous.
struct CsrValues {
  Tensor values, row_offsets, column_indices;
  int m, nonzeros, value_bytes;
};

void check_index(const char* op, const char* name, const Tensor& t, const Tensor& values) {
  TORCH_CHECK(t.device() == values.device(), "torch_sputnik::", op, ": ", name, " must be on ", values.device(),
              " with values, got ", t.device());
  TORCH_CHECK(t.scalar_type() == at::kInt && t.dim() == 1, "torch_sputnik::", op, ": ", name,
              " must be a 1-D int32 tensor, got ", t.scalar_type(), " ", t.sizes());
}

CsrValues check_csr_values(const char* op, const Tensor& values, const Tensor& row_offsets,
                           const Tensor& column_indices) {
  TORCH_CHECK(values.is_cuda(), "torch_sputnik::", op, ": values must be a GPU (HIP) tensor, got ", values.device());
  TORCH_CHECK(type_code(values.scalar_type()) >= 0, "torch_sputnik::", op,
              ": values must be float32, float16 or bfloat16, got ", values.scalar_type());
  check_index(op, "row_offsets", row_offsets, values);
  check_index(op, "column_indices", column_indices, values);
  TORCH_CHECK(row_offsets.numel() >= 1, "torch_sputnik::", op, ": row_offsets should be [m + 1], got ",
              row_offsets.sizes());
  TORCH_CHECK(values.dim() == 1 && values.numel() == column_indices.numel(), "torch_sputnik::", op,
              ": values should be [nnz] like column_indices ", column_indices.sizes(), ", got ", values.sizes());
  return {values.contiguous(), row_offsets.contiguous(), column_indices.contiguous(),
          to_int(row_offsets.numel() - 1, "m"), to_int(values.numel(), "nnz"),
          static_cast<int>(values.element_size())};
}

// A dense [..., m, n] operand whose rows the kernels read in place: the tensor itself where its
// last dimension is dense, else a contiguous copy, and its row stride (0 for at most one row).
struct DenseRows {
  Tensor tensor;
  int64_t row_stride;
};

DenseRows rows_in_place(const Tensor& t) {
  Tensor rows = t.size(-1) > 1 && t.stride(-1) != 1 ? t.contiguous() : t;
  return {rows, rows.size(-2) > 1 ? rows.stride(-2) : 0};
}

// Dense [m, n] scores of a storage type on the GPU, rows read in place; with a pattern, on its
// device and of its m rows.
DenseRows check_scores(const char* op, const Tensor& scores, const CsrValues* csr = nullptr) {
  TORCH_CHECK(scores.is_cuda(), "torch_sputnik::", op, ": scores must be a GPU (HIP) tensor, got ", scores.device());
  TORCH_CHECK(scores.dim() == 2, "torch_sputnik::", op, ": expected [m, n] scores, got ", scores.sizes());
  TORCH_CHECK(type_code(scores.scalar_type()) >= 0, "torch_sputnik::", op,
              ": scores must be float32, float16 or bfloat16, got ", scores.scalar_type());
  if (csr != nullptr) {
    TORCH_CHECK(scores.device() == csr->values.device(), "torch_sputnik::", op, ": scores must be on ",
                csr->values.device(), " with values, got ", scores.device());
    TORCH_CHECK(scores.size(0) == csr->m, "torch_sputnik::", op, ": row_offsets should be [m + 1] for [m, n] scores ",
                scores.sizes(), ", got ", csr->row_offsets.sizes());
  }
  return rows_in_place(scores);
}

// per_row / total, the other one -1 -> which mode and its count
struct Selection {
  int total_mode;
  int64_t count;
};

Selection parse_selection(const char* op, int64_t per_row, int64_t total) {
  TORCH_CHECK((per_row >= 0) != (total >= 0), "torch_sputnik::", op, ": give exactly one of per_row / total");
  return {total >= 0 ? 1 : 0, total >= 0 ? total : per_row};
}

void check_count(const char* op, const char* name, int64_t count, int64_t most) {
  TORCH_CHECK(count >= 0 && count <= most, "torch_sputnik::", op, ": ", name, " = ", count, " is outside 0 .. ", most);
}

// The key of the largest finite value of a storage type: what NaN and inf grow scores count as.
unsigned key_limit(at::ScalarType t) {
  return t == at::kFloat ? 0x7f7fffffu : t == at::kHalf ? 0x7bffu : 0x7f7fu;
}

// A call's own workspace, on the stream's allocator: no other call can be writing it.
Tensor workspace_like(const Tensor& like, size_t bytes) {
  return at::empty({static_cast<int64_t>(bytes)}, like.options().dtype(at::kByte));
}

// The `served` answer of a *_launch_shape / *_route query: raise unless the kernels serve the sizes.
void check_served(const char* op, int served, const char* query, const char* fallback) {
  TORCH_CHECK(served, "torch_sputnik::", op, ": the sizes are beyond what the kernels serve (", query,
              " states the limits); take ", fallback);
}

// A plan is the workspace of the matching *_workspace_bytes query after the
// topology-only pre-pass ran in it (spmm_plan / sddmm_plan / sparse_attention_plan).
void check_plan(const Tensor& plan, size_t bytes, const Tensor& like) {
  TORCH_CHECK(plan.scalar_type() == at::kByte && plan.is_contiguous() && plan.dim() == 1,
              "plan must be the uint8 tensor a *_plan op returned");
  TORCH_CHECK(plan.device() == like.device(), "plan must be on ", like.device());
  TORCH_CHECK(static_cast<size_t>(plan.numel()) >= bytes,
              "plan is too small for this call (", plan.numel(), " < ", bytes,
              " bytes): it was made for other sizes");
}

// The workspace of a call: the plan where one is given (checked against `bytes`), else fresh
// memory that `keep` holds for the call; no pointer where the call needs no workspace.
struct Workspace {
  void* ptr;
  int planned;
  Tensor keep;
};

Workspace plan_or_workspace(const c10::optional<Tensor>& plan, size_t bytes, const Tensor& like) {
  if (plan.has_value()) {
    check_plan(*plan, bytes, like);
    return {bytes ? plan->data_ptr() : nullptr, 1, Tensor()};
  }
  if (bytes == 0) return {nullptr, 0, Tensor()};
  Tensor fresh = workspace_like(like, bytes);
  return {fresh.data_ptr(), 0, fresh};
}

Tensor permute_last(const Tensor& values_in, const Tensor& permutation);
Tensor transpose_last2(const Tensor& x);

// ---------------------------------------------------------------------------
// The SpMM host stack: one operand contract (check_spmm), one product with its
// ladder of routes (spmm_product), and on top of it the transposed-store form and the groups.
// ---------------------------------------------------------------------------

// Entry p of the topology takes values[..., permutation[p]]: int32 [nonzeros], contiguous, on
// `like`'s device.
void check_permutation(const Tensor& permutation, int64_t nonzeros, const Tensor& like) {
  TORCH_CHECK(permutation.scalar_type() == at::kInt && permutation.dim() == 1 &&
                  permutation.is_contiguous() && permutation.device() == like.device() &&
                  permutation.size(0) == nonzeros,
              "permutation must be a contiguous int32 vector of ", nonzeros, " entries on ",
              like.device());
}

// One value per output row -> float32 [m] on `like`'s device.
Tensor check_bias(const Tensor& bias_in, int m, const Tensor& like) {
  const Tensor bias = as_float(bias_in, "bias");
  TORCH_CHECK(bias.device() == like.device() && bias.dim() == 1 && bias.size(0) == m,
              "bias should have m = ", m, " elements on ", like.device(), ", got ", bias.sizes());
  return bias;
}

bool is_half(const Tensor& t) {
  return t.scalar_type() == at::kHalf || t.scalar_type() == at::kBFloat16;
}

// THE NATIVE-HALF RULE.  A product with a float16 / bfloat16 operand -- one of them, or both of ONE
// half type -- goes to the typed kernels as it is stored (sputnik_hip_spmm_typed: no widening
// copy).  A float16 x bfloat16 mix widens both to float32, and so does a permutation (the permuted
// forms, which the modules reach with float32 operands, gather float32 values).  The
// transposed-store form asks the same question without its block_rows: its fused launch reads
// float32 and widens such operands for itself, and where that launch does not serve the call the
// product it falls back to reads the operands as they came, half included.
bool native_half(const Tensor& values, const Tensor& dense, bool permuted) {
  return (is_half(values) || is_half(dense)) && !permuted &&
         !(is_half(values) && is_half(dense) && values.scalar_type() != dense.scalar_type());
}

// The operands of spmm (values [nnz] against dense [k, n], or [R, nnz] against [R, k, n]) and
// left_spmm (values [nnz], shared, against dense [k, n] / [R, k, n]) after every check: contiguous,
// on one device, as stored (native_half) or float32; the product is [replicas, m, n] float32,
// [m, n] for the one replica of a spmm.
struct SpmmCall {
  const char* what;
  Tensor values, dense;
  c10::optional<Tensor> permutation;
  Topology topo;
  int m, k, n, replicas;
  int64_t values_stride;   // 0: one row of values for every replica
  bool left, native_half;
};

SpmmCall check_spmm(const char* what, int64_t m64, int64_t k64, const Tensor& values_in,
                    const Tensor& row_indices, const Tensor& row_offsets,
                    const Tensor& column_indices, const Tensor& dense_in, bool left,
                    const c10::optional<Tensor>& permutation = c10::nullopt) {
  SpmmCall c;
  c.what = what;
  c.left = left;
  c.m = to_int(m64, "m");
  c.k = to_int(k64, "k");
  c.native_half = native_half(values_in, dense_in, permutation.has_value());
  c.values = c.native_half ? as_storage(values_in, "values") : as_float(values_in, "values");
  c.dense = c.native_half ? as_storage(dense_in, "dense") : as_float(dense_in, "dense");
  const Tensor& values = c.values;
  const Tensor& dense = c.dense;
  TORCH_CHECK(dense.device() == values.device(), "values and dense must be on one device");
  TORCH_CHECK(dense.dim() == 2 || dense.dim() == 3, "dense should have 2 or 3 dimensions, got ",
              dense.dim());
  if (left) {
    TORCH_CHECK(values.dim() == 1, "left_spmm: values should have 1 dimension, got ",
                values.dim());
  } else {
    TORCH_CHECK(values.dim() == 1 || values.dim() == 2,
                "values should have 1 or 2 dimensions, got ", values.dim());
    TORCH_CHECK(values.dim() == dense.dim() - 1,
                "values and dense must be replicated the same: values.dim()=", values.dim(),
                ", dense.dim()=", dense.dim());
  }
  c.topo = check_topology(c.m, row_indices, row_offsets, column_indices, values);
  const int dim_offset = static_cast<int>(dense.dim()) - 2;
  c.replicas = dim_offset == 1 ? to_int(dense.size(0), "replicas") : 1;
  c.n = to_int(dense.size(dim_offset + 1), "n");
  TORCH_CHECK(values.size(-1) == c.topo.nonzeros, "number of values (", values.size(-1),
              ") must equal the number of column_indices (", c.topo.nonzeros, ")");
  TORCH_CHECK(dense.size(dim_offset) == c.k, "inner matrix dimensions must match: dense has ",
              dense.size(dim_offset), " rows, k = ", c.k);
  if (!left && values.dim() == 2) {
    TORCH_CHECK(values.size(0) == c.replicas, "first dim of values (", values.size(0),
                ") and dense (", c.replicas, ") must match");
  }
  c.values_stride = (left || values.dim() == 1) ? 0 : c.topo.nonzeros;
  if (permutation.has_value()) {
    check_permutation(*permutation, c.topo.nonzeros, values);
    c.permutation = permutation;
  }
  return c;
}

// The product of a checked call: the ladder  permuted -> native half -> planned -> per call.
// `bias_in` / `relu` come from spmm_bias* alone: no permutation and no plan with them.
Tensor spmm_product(const SpmmCall& c, const c10::optional<Tensor>& plan,
                    const c10::optional<Tensor>& bias_in = c10::nullopt, bool relu = false) {
  TORCH_INTERNAL_ASSERT(!bias_in.has_value() || (!plan.has_value() && !c.permutation.has_value()));
  const int m = c.m, k = c.k, n = c.n, nonzeros = c.topo.nonzeros, replicas = c.replicas;
  const int* row_indices = c.topo.row_indices.data_ptr<int>();
  const int* row_offsets = c.topo.row_offsets.data_ptr<int>();
  const int* column_indices = c.topo.column_indices.data_ptr<int>();
  const int64_t dense_stride = static_cast<int64_t>(k) * n, out_stride = static_cast<int64_t>(m) * n;
  const sputnik_hip_stream_t stream = current_stream(c.values);
  const auto options = c.values.options().dtype(at::kFloat);   // the product is float32
  Tensor out = (replicas == 1 && !c.left) ? at::empty({m, n}, options)
                                          : at::empty({replicas, m, n}, options);
  Tensor values = c.values;
  if (c.permutation.has_value()) {
    // values are those of ANOTHER ordering of the same entries (the topology here is its
    // transpose).  One kernel where the panel kernel serves the shape in one pass; otherwise
    // the values are permuted first and the call goes on as usual.
    if (sputnik_hip_spmm_permuted_supported(m, k, n, nonzeros)) {
      const int st = sputnik_hip_spmm_permuted_batched(
          m, k, n, nonzeros, replicas, row_indices, values.data_ptr<float>(), c.values_stride,
          c.permutation->data_ptr<int>(), row_offsets, column_indices, c.dense.data_ptr<float>(),
          dense_stride, out.data_ptr<float>(), out_stride, stream);
      if (st != SPUTNIK_HIP_UNSUPPORTED) {
        check_status(st, c.what);
        return out;
      }
    }
    values = permute_last(values, *c.permutation);
  }
  Tensor bias;
  if (bias_in.has_value()) bias = check_bias(*bias_in, m, values);
  const float* bias_ptr = bias.defined() ? bias.data_ptr<float>() : nullptr;
  if (c.native_half) {   // (a plan has nothing to add: the half-reading kernels have no pre-pass)
    const int values_type = type_code(values.scalar_type()), dense_type = type_code(c.dense.scalar_type());
    const size_t typed_ws = sputnik_hip_spmm_typed_workspace_bytes(
        m, k, n, nonzeros, replicas, values_type, c.values_stride, dense_type);
    Tensor workspace;
    char* ws = nullptr;
    if (typed_ws > 0) {
      workspace = workspace_like(values, typed_ws + 256);
      ws = static_cast<char*>(workspace.data_ptr());
      ws += (256 - reinterpret_cast<uintptr_t>(ws) % 256) % 256;
    }
    check_status(sputnik_hip_spmm_typed(m, k, n, nonzeros, replicas, row_indices, values.data_ptr(),
                                        values_type, c.values_stride, row_offsets, column_indices,
                                        c.dense.data_ptr(), dense_type, dense_stride, bias_ptr,
                                        relu ? 1 : 0, out.data_ptr<float>(), out_stride, ws, typed_ws,
                                        stream),
                 c.what);
    return out;
  }
  const size_t ws_bytes = sputnik_hip_spmm_workspace_bytes(m, k, n, nonzeros);
  const Workspace ws = plan_or_workspace(plan, ws_bytes, values);
  if (ws.planned) {   // static topology: the pre-pass ran once (spmm_plan); kernels only
    check_status(sputnik_hip_spmm_batched_planned(
                     m, k, n, nonzeros, replicas, row_indices, values.data_ptr<float>(),
                     c.values_stride, row_offsets, column_indices, c.dense.data_ptr<float>(),
                     dense_stride, out.data_ptr<float>(), out_stride, ws.ptr, ws_bytes, stream),
                 c.what);
    return out;
  }
  check_status(sputnik_hip_spmm_bias_batched(
                   m, k, n, nonzeros, replicas, row_indices, values.data_ptr<float>(),
                   c.values_stride, row_offsets, column_indices, c.dense.data_ptr<float>(),
                   dense_stride, bias_ptr, relu ? 1 : 0, out.data_ptr<float>(), out_stride, ws.ptr,
                   ws_bytes, stream),
               c.what);
  return out;
}

// The product stored as the transposes of its blocks of `block_rows` rows,
// [replicas * m / block_rows, n, block_rows]: the head split behind a projection
// (modules/sparse_attention.py:38-45) or the whole C^T (block_rows = m), written by the panel
// kernel's store phase where it serves the shape (float32: half operands are widened for it);
// elsewhere the product of the operands as they came, then the tiled transpose kernel.
Tensor spmm_transposed_store(const SpmmCall& c, int64_t block_rows,
                             const c10::optional<Tensor>& plan) {
  TORCH_CHECK(c.m % block_rows == 0, "block_rows (", block_rows, ") must divide m = ", c.m);
  const int64_t blocks = c.replicas * (c.m / block_rows);
  const int nonzeros = c.topo.nonzeros;
  if ((!c.permutation.has_value() || sputnik_hip_spmm_permuted_supported(c.m, c.k, c.n, nonzeros)) &&
      sputnik_hip_spmm_transposed_out_supported(c.m, c.k, c.n, nonzeros, static_cast<int>(block_rows))) {
    const Tensor values = c.native_half ? c.values.to(at::kFloat) : c.values;
    const Tensor dense = c.native_half ? c.dense.to(at::kFloat) : c.dense;
    Tensor out = at::empty({blocks, c.n, block_rows}, values.options());
    const int st = sputnik_hip_spmm_transposed_out_batched(
        c.m, c.k, c.n, nonzeros, c.replicas, values.data_ptr<float>(), c.values_stride,
        c.permutation.has_value() ? c.permutation->data_ptr<int>() : nullptr,
        c.topo.row_offsets.data_ptr<int>(), c.topo.column_indices.data_ptr<int>(),
        dense.data_ptr<float>(), static_cast<int64_t>(c.k) * c.n, nullptr, 0,
        static_cast<int>(block_rows), out.data_ptr<float>(), static_cast<int64_t>(c.m) * c.n,
        current_stream(values));
    if (st != SPUTNIK_HIP_UNSUPPORTED) {
      check_status(st, c.what);
      return out;
    }
  }
  return transpose_last2(spmm_product(c, plan).reshape({blocks, block_rows, c.n}));
}

// One op: the operands checked, then the product or (block_rows > 0) its transposed store.
Tensor spmm_op(const char* what, int64_t m, int64_t k, const Tensor& values,
               const Tensor& row_indices, const Tensor& row_offsets, const Tensor& column_indices,
               const Tensor& dense, bool left, const c10::optional<Tensor>& permutation = c10::nullopt,
               const c10::optional<Tensor>& plan = c10::nullopt, int64_t block_rows = 0,
               const c10::optional<Tensor>& bias = c10::nullopt, bool relu = false) {
  const SpmmCall c = check_spmm(what, m, k, values, row_indices, row_offsets, column_indices, dense,
                                left, permutation);
  const c10::DeviceGuard guard(c.values.device());
  return block_rows > 0 ? spmm_transposed_store(c, block_rows, plan)
                        : spmm_product(c, plan, bias, relu);
}

// The registered ops.  spmm / left_spmm (`left`): plain, through a plan, and over a topology whose
// values are given in another order (values_here[p] = values[permutation[p]]: the transposed
// products of the backward passes, modules/spmm.py:59-66, without the permuted copy).
template <bool left>
Tensor spmm_plain(int64_t m, int64_t k, const Tensor& values, const Tensor& row_indices,
                  const Tensor& row_offsets, const Tensor& column_indices, const Tensor& dense) {
  return spmm_op(left ? "left_spmm" : "spmm", m, k, values, row_indices, row_offsets, column_indices,
                 dense, left);
}
constexpr auto spmm = &spmm_plain<false>;   // (the composed attention routes call it)

template <bool left>
Tensor spmm_planned(int64_t m, int64_t k, const Tensor& values, const Tensor& row_indices,
                    const Tensor& row_offsets, const Tensor& column_indices, const Tensor& dense,
                    const Tensor& plan) {
  return spmm_op(left ? "left_spmm_planned" : "spmm_planned", m, k, values, row_indices, row_offsets,
                 column_indices, dense, left, c10::nullopt, plan);
}

template <bool left>
Tensor spmm_permuted(int64_t m, int64_t k, const Tensor& values, const Tensor& permutation,
                     const Tensor& row_indices, const Tensor& row_offsets,
                     const Tensor& column_indices, const Tensor& dense,
                     const c10::optional<Tensor>& plan) {
  return spmm_op(left ? "left_spmm_permuted" : "spmm_permuted", m, k, values, row_indices,
                 row_offsets, column_indices, dense, left, permutation, plan);
}

template <bool relu>
Tensor spmm_bias(int64_t m, int64_t k, const Tensor& values, const Tensor& row_indices,
                 const Tensor& row_offsets, const Tensor& column_indices, const Tensor& bias,
                 const Tensor& dense) {
  return spmm_op(relu ? "spmm_bias_relu" : "spmm_bias", m, k, values, row_indices, row_offsets,
                 column_indices, dense, false, c10::nullopt, c10::nullopt, 0, bias, relu);
}

// spmm / left_spmm stored as spmm_transposed_store writes it; `permutation` as in spmm_permuted.
Tensor spmm_transposed_out(int64_t m, int64_t k, const Tensor& values,
                           const c10::optional<Tensor>& permutation, const Tensor& row_indices,
                           const Tensor& row_offsets, const Tensor& column_indices,
                           const Tensor& dense, int64_t block_rows, bool left,
                           const c10::optional<Tensor>& plan) {
  TORCH_CHECK(block_rows > 0, "block_rows must be positive, got ", block_rows);
  return spmm_op("spmm_transposed_out", m, k, values, row_indices, row_offsets, column_indices,
                 dense, left, permutation, plan, block_rows);
}

// ---------------------------------------------------------------------------
// Groups of projections in one launch (sputnik_hip.h: sputnik_hip_spmm_group_batched):
// float32 throughout; a group the kernel does not take runs one by one through spmm_op.
// ---------------------------------------------------------------------------
// One checked left_spmm call per weight, widened to float32, all of one shape on one device;
// `dense`: one input per weight, or one that every weight shares.
std::vector<SpmmCall> check_group(const char* what, int64_t m, int64_t k, at::TensorList values,
                                  at::TensorList permutations, at::TensorList row_indices,
                                  at::TensorList row_offsets, at::TensorList column_indices,
                                  at::TensorList dense) {
  const size_t count = values.size();
  TORCH_CHECK(count >= 1, what, ": expected at least one matrix");
  TORCH_CHECK(row_indices.size() == count && row_offsets.size() == count &&
                  column_indices.size() == count && (dense.size() == count || dense.size() == 1) &&
                  (permutations.empty() || permutations.size() == count),
              what, ": the lists must have one entry per matrix");
  std::vector<Tensor> wide;
  for (const Tensor& d : dense) {
    wide.push_back(as_float(d, "dense"));
    TORCH_CHECK(d.dim() == 3 && d.sizes() == dense[0].sizes() && d.device() == dense[0].device(), what,
                ": the dense operands should be [B, k, n] of one shape on one device, got ", d.sizes());
  }
  std::vector<SpmmCall> calls;
  for (size_t p = 0; p < count; ++p)
    calls.push_back(check_spmm(
        what, m, k, as_float(values[p], "values"), row_indices[p], row_offsets[p], column_indices[p],
        wide[wide.size() == 1 ? 0 : p], true,
        permutations.empty() ? c10::optional<Tensor>() : c10::optional<Tensor>(permutations[p])));
  return calls;
}

// Weight p's problem: its own output, or the one the group sums into.
std::vector<sputnik_hip_spmm_problem> group_problems(const std::vector<SpmmCall>& calls,
                                                     const std::vector<Tensor>& outs) {
  std::vector<sputnik_hip_spmm_problem> problems;
  for (const SpmmCall& c : calls)
    problems.push_back({c.topo.row_indices.data_ptr<int>(), c.topo.row_offsets.data_ptr<int>(),
                        c.topo.column_indices.data_ptr<int>(), c.values.data_ptr<float>(),
                        c.permutation.has_value() ? c.permutation->data_ptr<int>() : nullptr,
                        c.dense.data_ptr<float>(),
                        outs[outs.size() == 1 ? 0 : problems.size()].data_ptr<float>(), c.topo.nonzeros});
  return problems;
}

// The group's one launch into `outs`.  False: not this group (a weight without entries, or the
// library turns it down) -- the caller runs it one by one.
bool group_launch(const char* what, const std::vector<SpmmCall>& calls, const std::vector<Tensor>& outs,
                  int64_t block_rows, int accumulate) {
  for (const SpmmCall& c : calls)
    if (c.topo.nonzeros == 0) return false;
  const SpmmCall& c = calls[0];
  const std::vector<sputnik_hip_spmm_problem> problems = group_problems(calls, outs);
  const int st = sputnik_hip_spmm_group_batched(
      c.m, c.k, c.n, c.replicas, static_cast<int>(problems.size()), problems.data(),
      static_cast<int64_t>(c.k) * c.n, static_cast<int64_t>(c.m) * c.n, static_cast<int>(block_rows),
      accumulate, current_stream(c.dense));
  if (st == SPUTNIK_HIP_UNSUPPORTED) return false;
  check_status(st, what);
  return true;
}

// One input, several sparse weights, every product stored head split
// ([B * m / block_rows, n, block_rows] each; block_rows = 0: plain [B, m, n]).
std::vector<Tensor> left_spmm_group(int64_t m, int64_t k, at::TensorList values,
                                    at::TensorList row_indices, at::TensorList row_offsets,
                                    at::TensorList column_indices, const Tensor& dense,
                                    int64_t block_rows) {
  const std::vector<SpmmCall> calls = check_group("left_spmm_group", m, k, values, {}, row_indices,
                                                  row_offsets, column_indices, {dense});
  const SpmmCall& c = calls[0];
  const c10::DeviceGuard guard(c.dense.device());
  std::vector<Tensor> outs;
  if (sputnik_hip_spmm_group_supported(c.m, c.k, c.n, static_cast<int>(calls.size()),
                                       static_cast<int>(block_rows), 0)) {
    for (const SpmmCall& each : calls)
      outs.push_back(block_rows > 0
                         ? at::empty({c.replicas * (c.m / block_rows), c.n, block_rows}, each.values.options())
                         : at::empty({c.replicas, c.m, c.n}, each.values.options()));
    if (group_launch("left_spmm_group", calls, outs, block_rows, 0)) return outs;
    outs.clear();
  }
  for (size_t p = 0; p < calls.size(); ++p)   // one by one
    outs.push_back(spmm_op("left_spmm_group", m, k, values[p], row_indices[p], row_offsets[p],
                           column_indices[p], dense, true, c10::nullopt, c10::nullopt, block_rows));
  return outs;
}

// sum over the matrices of  A_p @ dense_p  (values gathered through
// `permutations` when given): the input gradient of a group of projections.
Tensor left_spmm_group_sum(int64_t m, int64_t k, at::TensorList values, at::TensorList permutations,
                           at::TensorList row_indices, at::TensorList row_offsets,
                           at::TensorList column_indices, at::TensorList dense) {
  const std::vector<SpmmCall> calls = check_group("left_spmm_group_sum", m, k, values, permutations,
                                                  row_indices, row_offsets, column_indices, dense);
  TORCH_CHECK(dense.size() == values.size(), "left_spmm_group_sum: one dense operand per matrix");
  const SpmmCall& c = calls[0];
  const c10::DeviceGuard guard(c.dense.device());
  if (sputnik_hip_spmm_group_supported(c.m, c.k, c.n, static_cast<int>(calls.size()), 0, 1)) {
    Tensor out = at::empty({c.replicas, c.m, c.n}, c.values.options());
    if (group_launch("left_spmm_group_sum", calls, {out}, 0, 1)) return out;
  }
  Tensor total;
  for (size_t p = 0; p < calls.size(); ++p) {   // one by one
    const Tensor part = spmm_op("left_spmm_group_sum", m, k, values[p], row_indices[p], row_offsets[p],
                                column_indices[p], dense[p], true, calls[p].permutation);
    total = p == 0 ? part : total + part;
  }
  return total;
}

// left_spmm as a dense contraction on half tiles (sputnik_hip.h: left_spmm_half_tiles):
// values [nnz] and dense [R, k, n] float32 or of the tile type (1 float16 / 2 bfloat16).
// An EMPTY tensor says the route does not serve the call: take left_spmm then.
Tensor left_spmm_half_tiles(int64_t m64, int64_t k64, const Tensor& values_in,
                            const Tensor& row_offsets, const Tensor& column_indices,
                            const Tensor& dense_in, int64_t tile_type) {
  const int m = to_int(m64, "m"), k = to_int(k64, "k");
  const Tensor values = as_storage(values_in, "values");
  const Tensor dense = as_storage(dense_in, "dense");
  TORCH_CHECK(values.dim() == 1, "left_spmm_half_tiles: values should have 1 dimension");
  TORCH_CHECK(dense.dim() == 3 && dense.size(1) == k, "left_spmm_half_tiles: dense must be [R, k, n]");
  TORCH_CHECK(dense.device() == values.device(), "values and dense must be on one device");
  const c10::DeviceGuard guard(values.device());
  const Tensor ro = as_index(row_offsets, "row_offsets", values);
  const Tensor ci = as_index(column_indices, "column_indices", values);
  TORCH_CHECK(ro.size(0) == m + 1, "row_offsets should have m + 1 entries");
  TORCH_CHECK(values.size(0) == ci.size(0), "number of values and column_indices must match");
  const int nonzeros = to_int(ci.size(0), "nonzeros");
  const int replicas = to_int(dense.size(0), "replicas"), n = to_int(dense.size(2), "n");
  const int vt = type_code(values.scalar_type()), dt = type_code(dense.scalar_type());
  const size_t ws_bytes = sputnik_hip_left_spmm_half_tiles_workspace_bytes(
      m, k, n, nonzeros, replicas, vt, dt, static_cast<int>(tile_type));
  const auto options = values.options().dtype(at::kFloat);
  if (ws_bytes == 0) return at::empty({0}, options);
  Tensor workspace = at::empty({static_cast<int64_t>(ws_bytes)}, values.options().dtype(at::kByte));
  Tensor out = at::empty({replicas, m, n}, options);
  const int st = sputnik_hip_left_spmm_half_tiles(
      m, k, n, nonzeros, replicas, ro.data_ptr<int>(), ci.data_ptr<int>(), values.data_ptr(), vt,
      dense.data_ptr(), dt, static_cast<int64_t>(k) * n, static_cast<int>(tile_type), nullptr, 0,
      out.data_ptr<float>(), static_cast<int64_t>(m) * n, workspace.data_ptr(), ws_bytes,
      current_stream(values));
  if (st == SPUTNIK_HIP_UNSUPPORTED) return at::empty({0}, options);
  check_status(st, "left_spmm_half_tiles");
  return out;
}

// ---- a sparse layer on half-stored activations: the three products on the matrix cores,
// no layout pass (sputnik_hip.h: sparse_linear_half_*) ----
int tile_code_of(const Tensor& x) {
  const int code = type_code(x.scalar_type());
  TORCH_CHECK(code == SPUTNIK_HIP_F16 || code == SPUTNIK_HIP_BF16,
              "expected float16 / bfloat16 activations, got ", x.scalar_type());
  return code;
}

// The weight's image [planes][out][in] in the tile type (uint8 tensor).
Tensor half_linear_image(int64_t out64, int64_t in64, const Tensor& values_in, const Tensor& row_offsets,
                         const Tensor& column_indices, int64_t tile_type) {
  const int out_f = to_int(out64, "out"), in_f = to_int(in64, "in");
  const Tensor values = as_storage(values_in, "values");
  const c10::DeviceGuard guard(values.device());
  const Tensor ro = as_index(row_offsets, "row_offsets", values);
  const Tensor ci = as_index(column_indices, "column_indices", values);
  TORCH_CHECK(ro.size(0) == out_f + 1 && values.dim() == 1 && values.size(0) == ci.size(0),
              "half_linear_image: CSR arrays do not match");
  const int vt = type_code(values.scalar_type());
  const size_t bytes = sputnik_hip_sparse_linear_half_image_bytes(out_f, in_f, vt, static_cast<int>(tile_type));
  Tensor image = at::empty({static_cast<int64_t>(bytes)}, values.options().dtype(at::kByte));
  check_status(sputnik_hip_sparse_linear_half_image(out_f, in_f, to_int(ci.size(0), "nonzeros"),
                                                    ro.data_ptr<int>(), ci.data_ptr<int>(),
                                                    values.data_ptr(), vt, static_cast<int>(tile_type),
                                                    image.data_ptr(), bytes, current_stream(values)),
               "half_linear_image");
  return image;
}

// float32 tensor -> its half planes (uint8 tensor, planes x numel x 2 bytes).
Tensor half_planes(const Tensor& t_in, int64_t tile_type) {
  TORCH_CHECK(t_in.is_cuda() && t_in.scalar_type() == at::kFloat, "half_planes: expected a float32 GPU tensor");
  const Tensor t = t_in.contiguous();
  TORCH_CHECK(t.numel() % 4 == 0, "half_planes: element count must be a multiple of 4");
  const c10::DeviceGuard guard(t.device());
  const size_t bytes = sputnik_hip_half_planes_bytes(t.numel(), static_cast<int>(tile_type));
  Tensor planes = at::empty({static_cast<int64_t>(bytes)}, t.options().dtype(at::kByte));
  check_status(sputnik_hip_half_planes(t.numel(), t.data_ptr<float>(), static_cast<int>(tile_type),
                                       planes.data_ptr(), current_stream(t)),
               "half_planes");
  return planes;
}

// y [batch, out, seq] float32 = W x^T per batch element, x [batch, seq, in] half.
Tensor half_linear_forward(int64_t out64, const Tensor& image, int64_t values_type, const Tensor& x_in) {
  const Tensor x = x_in.contiguous();
  TORCH_CHECK(x.is_cuda() && x.dim() == 3, "half_linear_forward: x must be a GPU tensor [batch, seq, in]");
  const int tile = tile_code_of(x);
  const c10::DeviceGuard guard(x.device());
  const int out_f = to_int(out64, "out"), batch = to_int(x.size(0), "batch"), seq = to_int(x.size(1), "seq"),
            in_f = to_int(x.size(2), "in");
  TORCH_CHECK(static_cast<size_t>(image.numel()) >=
                  sputnik_hip_sparse_linear_half_image_bytes(out_f, in_f, static_cast<int>(values_type), tile),
              "half_linear_forward: the image was made for another shape");
  Tensor y = at::empty({batch, out_f, seq}, x.options().dtype(at::kFloat));
  check_status(sputnik_hip_sparse_linear_half_forward(out_f, in_f, seq, batch, image.data_ptr(),
                                                      static_cast<int>(values_type), x.data_ptr(), tile,
                                                      nullptr, 0, y.data_ptr<float>(), current_stream(x)),
               "half_linear_forward");
  return y;
}

Tensor half_linear_plan(int64_t out64, int64_t in64, const Tensor& row_offsets, const Tensor& column_indices) {
  const int out_f = to_int(out64, "out"), in_f = to_int(in64, "in");
  TORCH_CHECK(row_offsets.is_cuda(), "half_linear_plan: expected GPU index tensors");
  const c10::DeviceGuard guard(row_offsets.device());
  const Tensor ro = as_index(row_offsets, "row_offsets", row_offsets);
  const Tensor ci = as_index(column_indices, "column_indices", row_offsets);
  const size_t bytes = sputnik_hip_sparse_linear_half_plan_bytes(out_f, in_f);
  Tensor plan = at::empty({static_cast<int64_t>(bytes)}, row_offsets.options().dtype(at::kByte));
  check_status(sputnik_hip_sparse_linear_half_plan(out_f, in_f, ro.data_ptr<int>(), ci.data_ptr<int>(),
                                                   plan.data_ptr(), current_stream(row_offsets)),
               "half_linear_plan");
  return plan;
}

// grad: the planes of the float32 dy (half_planes; grad_is_planes) or dy in x's type.
Tensor half_linear_weight_gradient(int64_t out64, const Tensor& row_offsets, const Tensor& column_indices,
                                   const Tensor& grad, bool grad_is_planes, const Tensor& x_in,
                                   const c10::optional<Tensor>& plan) {
  const Tensor x = x_in.contiguous();
  const int tile = tile_code_of(x);
  const c10::DeviceGuard guard(x.device());
  const int out_f = to_int(out64, "out"), batch = to_int(x.size(0), "batch"), seq = to_int(x.size(1), "seq"),
            in_f = to_int(x.size(2), "in");
  const Tensor ro = as_index(row_offsets, "row_offsets", x);
  const Tensor ci = as_index(column_indices, "column_indices", x);
  const int nonzeros = to_int(ci.size(0), "nonzeros");
  const int grad_type = grad_is_planes ? SPUTNIK_HIP_F32 : tile;
  const Tensor g = grad.contiguous();
  const size_t want = grad_is_planes
                          ? sputnik_hip_half_planes_bytes(static_cast<int64_t>(batch) * out_f * seq, tile)
                          : static_cast<size_t>(batch) * out_f * seq * 2;
  TORCH_CHECK(static_cast<size_t>(g.numel()) * g.element_size() >= want,
              "half_linear_weight_gradient: grad does not hold [batch, out, seq]");
  const size_t scratch_bytes = sputnik_hip_sparse_linear_half_scratch_bytes(out_f, in_f, seq, batch,
                                                                            nonzeros, grad_type, tile);
  Tensor scratch;
  if (scratch_bytes) scratch = at::empty({static_cast<int64_t>(scratch_bytes)}, x.options().dtype(at::kByte));
  Tensor out = at::empty({nonzeros}, x.options().dtype(at::kFloat));
  check_status(sputnik_hip_sparse_linear_half_weight_gradient(
                   out_f, in_f, seq, batch, nonzeros, ro.data_ptr<int>(), ci.data_ptr<int>(), g.data_ptr(),
                   grad_type, x.data_ptr(), tile, out.data_ptr<float>(),
                   plan.has_value() ? plan->data_ptr() : nullptr,
                   scratch_bytes ? scratch.data_ptr() : nullptr, scratch_bytes, current_stream(x)),
               "half_linear_weight_gradient");
  return out;
}

// The weight gradient and, from the same tiles, the dense one: (grad_values [nnz], dense
// [out, in]), both float32, one launch; grad_values[p] == dense[row_p, col_p] bit for bit.
std::tuple<Tensor, Tensor> half_linear_weight_gradient_dense(int64_t out64, const Tensor& row_offsets,
                                                             const Tensor& column_indices, const Tensor& grad,
                                                             bool grad_is_planes, const Tensor& x_in,
                                                             const c10::optional<Tensor>& plan) {
  const Tensor x = x_in.contiguous();
  TORCH_CHECK(x.is_cuda() && x.dim() == 3,
              "half_linear_weight_gradient_dense: x must be a GPU tensor [batch, seq, in]");
  const int tile = tile_code_of(x);
  const c10::DeviceGuard guard(x.device());
  const int out_f = to_int(out64, "out"), batch = to_int(x.size(0), "batch"), seq = to_int(x.size(1), "seq"),
            in_f = to_int(x.size(2), "in");
  const Tensor ro = as_index(row_offsets, "row_offsets", x);
  const Tensor ci = as_index(column_indices, "column_indices", x);
  TORCH_CHECK(ro.size(0) == out_f + 1, "half_linear_weight_gradient_dense: row_offsets do not match out_features");
  const int nonzeros = to_int(ci.size(0), "nonzeros");
  const int grad_type = grad_is_planes ? SPUTNIK_HIP_F32 : tile;
  const Tensor g = grad.contiguous();
  const size_t want = grad_is_planes
                          ? sputnik_hip_half_planes_bytes(static_cast<int64_t>(batch) * out_f * seq, tile)
                          : static_cast<size_t>(batch) * out_f * seq * 2;
  TORCH_CHECK(static_cast<size_t>(g.numel()) * g.element_size() >= want,
              "half_linear_weight_gradient_dense: grad does not hold [batch, out, seq]");
  Tensor out = at::empty({nonzeros}, x.options().dtype(at::kFloat));
  Tensor dense = at::empty({out_f, in_f}, x.options().dtype(at::kFloat));
  check_status(sputnik_hip_sparse_linear_half_weight_gradient_dense(
                   out_f, in_f, seq, batch, nonzeros, ro.data_ptr<int>(), ci.data_ptr<int>(), g.data_ptr(),
                   grad_type, x.data_ptr(), tile, out.data_ptr<float>(),
                   plan.has_value() ? plan->data_ptr() : nullptr, dense.data_ptr<float>(), in_f,
                   current_stream(x)),
               "half_linear_weight_gradient_dense");
  return std::make_tuple(out, dense);
}

// dense [out, in] float32 = sum over (batch, s) of dy x; either operand in the tile type or
// as the planes of its float32 tensor (half_planes); x_layout 0: x [batch, seq, in], 1: x
// [batch, in, seq].  The caller has asked sputnik_hip_sparse_linear_dense_weight_gradient_supported.
Tensor dense_weight_gradient(const Tensor& grad, bool grad_is_planes, const Tensor& x_in, bool x_is_planes,
                             int64_t x_layout, int64_t tile_type, int64_t out64, int64_t in64, int64_t seq64,
                             int64_t batch64) {
  TORCH_CHECK(grad.is_cuda() && x_in.is_cuda() && grad.device() == x_in.device(),
              "dense_weight_gradient: expected GPU operands on one device");
  const int tile = static_cast<int>(tile_type);
  const c10::DeviceGuard guard(grad.device());
  const int out_f = to_int(out64, "out"), in_f = to_int(in64, "in"), seq = to_int(seq64, "seq"),
            batch = to_int(batch64, "batch");
  TORCH_CHECK(out_f > 0 && in_f > 0 && seq > 0 && batch > 0, "dense_weight_gradient: empty operand");
  const Tensor g = grad.contiguous(), x = x_in.contiguous();
  const auto holds = [&](const Tensor& t, bool planes, int64_t count) {
    const size_t want = planes ? sputnik_hip_half_planes_bytes(count, tile) : static_cast<size_t>(count) * 2;
    return want > 0 && static_cast<size_t>(t.numel()) * t.element_size() >= want &&
           (planes || type_code(t.scalar_type()) == tile);
  };
  TORCH_CHECK(holds(g, grad_is_planes, static_cast<int64_t>(batch) * out_f * seq),
              "dense_weight_gradient: grad does not hold [batch, out, seq]");
  TORCH_CHECK(holds(x, x_is_planes, static_cast<int64_t>(batch) * seq * in_f),
              "dense_weight_gradient: x does not hold [batch, seq, in]");
  Tensor dense = at::empty({out_f, in_f}, g.options().dtype(at::kFloat));
  check_status(sputnik_hip_sparse_linear_dense_weight_gradient(
                   out_f, in_f, seq, batch, g.data_ptr(), grad_is_planes ? SPUTNIK_HIP_F32 : tile, x.data_ptr(),
                   x_is_planes ? SPUTNIK_HIP_F32 : tile, static_cast<int>(x_layout), tile,
                   dense.data_ptr<float>(), in_f, current_stream(g)),
               "dense_weight_gradient");
  return dense;
}

// dx [batch, seq, in] in `like`'s type (the activations'), or an EMPTY tensor where the
// route does not serve the call.
Tensor half_linear_input_gradient(int64_t out64, int64_t in64, const Tensor& grad, bool grad_is_planes,
                                  const Tensor& image, int64_t values_type, const Tensor& like,
                                  int64_t batch64, int64_t seq64) {
  const int tile = tile_code_of(like);
  const c10::DeviceGuard guard(like.device());
  const int out_f = to_int(out64, "out"), in_f = to_int(in64, "in"), batch = to_int(batch64, "batch"),
            seq = to_int(seq64, "seq");
  const Tensor g = grad.contiguous();
  Tensor dx = at::empty({batch, seq, in_f}, like.options());
  const int st = sputnik_hip_sparse_linear_half_input_gradient(
      out_f, in_f, seq, batch, g.data_ptr(), grad_is_planes ? SPUTNIK_HIP_F32 : tile, image.data_ptr(),
      static_cast<int>(values_type), tile, dx.data_ptr(), tile, current_stream(like));
  if (st == SPUTNIK_HIP_UNSUPPORTED) return at::empty({0}, like.options());
  check_status(st, "half_linear_input_gradient");
  return dx;
}

// sddmm_sum on one float32 and one half operand (3-D, contiguous).  False: the library
// does not serve the pair on this shape -- the caller widens the half operand.
bool sddmm_sum_mixed(int m, int n, const Tensor& row_indices, const Tensor& row_offsets,
                     const Tensor& column_indices, const Tensor& lhs_in, const Tensor& rhs_in,
                     const c10::optional<Tensor>& plan, Tensor* result) {
  if (!((lhs_in.scalar_type() == at::kFloat && is_half(rhs_in)) ||
        (rhs_in.scalar_type() == at::kFloat && is_half(lhs_in))))
    return false;
  if (!lhs_in.is_cuda() || lhs_in.dim() != 3 || rhs_in.dim() != 3 ||
      lhs_in.device() != rhs_in.device() || lhs_in.size(0) != rhs_in.size(0) ||
      lhs_in.size(-1) != rhs_in.size(-1) || lhs_in.size(1) != m || rhs_in.size(1) != n)
    return false;   // (the plain path reports what is wrong with the shapes)
  const Tensor lhs = lhs_in.contiguous(), rhs = rhs_in.contiguous();
  const c10::DeviceGuard guard(lhs.device());
  const Topology topo = check_topology(m, row_indices, row_offsets, column_indices, lhs);
  const int replicas = to_int(lhs.size(0), "replicas"), k = to_int(lhs.size(2), "k");
  const int lhs_code = type_code(lhs.scalar_type()), rhs_code = type_code(rhs.scalar_type());
  const size_t scratch_bytes = sputnik_hip_sddmm_sum_mixed_scratch_bytes(
      m, k, n, topo.nonzeros, replicas, lhs_code, rhs_code);
  if (scratch_bytes == 0) return false;
  const size_t ws_bytes = sputnik_hip_sddmm_sum_workspace_bytes(m, k, n, topo.nonzeros);
  const Workspace ws = plan_or_workspace(plan, ws_bytes, lhs);
  Tensor scratch = workspace_like(lhs, scratch_bytes);
  Tensor out = at::empty({topo.nonzeros}, lhs.options().dtype(at::kFloat));
  const int status = sputnik_hip_sddmm_sum_mixed(
      m, k, n, topo.nonzeros, replicas, topo.row_indices.data_ptr<int>(),
      topo.row_offsets.data_ptr<int>(), topo.column_indices.data_ptr<int>(), lhs.data_ptr(), lhs_code,
      static_cast<int64_t>(m) * k, rhs.data_ptr(), rhs_code, static_cast<int64_t>(n) * k,
      out.data_ptr<float>(), ws.ptr, ws_bytes, ws.planned, scratch.data_ptr(),
      scratch_bytes, current_stream(lhs));
  if (status == SPUTNIK_HIP_UNSUPPORTED) return false;
  check_status(status, "sddmm_sum (float32 x half)");
  *result = out;
  return true;
}

// lhs / rhs float32, float16 or bfloat16 (handed to the kernels as they are; operands
// of different types take the wider one).  out_type: -1 / SPUTNIK_HIP_F32 = float32 --
// the reference's output type (src/sddmm_cuda.cu:43) --, or the operands' half type.
Tensor sddmm_impl(int64_t m64, int64_t n64, const Tensor& row_indices, const Tensor& row_offsets,
                  const Tensor& column_indices, const Tensor& lhs_in, const Tensor& rhs_in,
                  const c10::optional<Tensor>& plan, bool sum_replicas = false,
                  int64_t out_type = -1) {
  const int m = to_int(m64, "m"), n = to_int(n64, "n");
  if (sum_replicas && lhs_in.scalar_type() != rhs_in.scalar_type()) {
    // a (float32, half) pair: the matrix-core route takes the float32 operand as two half
    // planes instead of widening the half one (sputnik_hip.h: sddmm_sum_mixed)
    Tensor mixed;
    if (sddmm_sum_mixed(m, n, row_indices, row_offsets, column_indices, lhs_in, rhs_in, plan, &mixed))
      return mixed;
  }
  const auto st = at::promote_types(lhs_in.scalar_type(), rhs_in.scalar_type());
  const Tensor lhs = as_storage(lhs_in, "lhs_matrix").to(st);
  const Tensor rhs = as_storage(rhs_in, "rhs_matrix").to(st);
  const int in_code = type_code(st);
  TORCH_CHECK(lhs.device() == rhs.device(), "lhs_matrix and rhs_matrix must be on one device");
  TORCH_CHECK(lhs.dim() == 2 || lhs.dim() == 3, "expected 2-dim or 3-dim lhs_matrix, got ",
              lhs.dim());
  TORCH_CHECK(rhs.dim() == lhs.dim(), "rhs_matrix and lhs_matrix must match number of dims");
  TORCH_CHECK(lhs.size(-1) == rhs.size(-1), "last dim of input matrices must match: ",
              lhs.size(-1), " vs ", rhs.size(-1));
  const c10::DeviceGuard guard(lhs.device());
  const Topology topo = check_topology(m, row_indices, row_offsets, column_indices, lhs);

  const int dim_offset = static_cast<int>(lhs.dim()) - 2;
  const int replicas = dim_offset == 1 ? to_int(lhs.size(0), "replicas") : 1;
  const int k = to_int(lhs.size(dim_offset + 1), "k");
  TORCH_CHECK(lhs.size(dim_offset) == m, "first dim of lhs_matrix (", lhs.size(dim_offset),
              ") must match output rows m = ", m);
  TORCH_CHECK(rhs.size(dim_offset) == n, "first dim of rhs_matrix (", rhs.size(dim_offset),
              ") must match output cols n = ", n);
  TORCH_CHECK(replicas == 1 || rhs.size(0) == replicas,
              "first dim of lhs_matrix and rhs_matrix must match");
  const int out_code = out_type < 0 ? SPUTNIK_HIP_F32 : static_cast<int>(out_type);
  TORCH_CHECK(out_code == SPUTNIK_HIP_F32 || (out_code == in_code && !sum_replicas),
              "sddmm: the output is float32 or has the operands' (half) type");
  const auto out_options = lhs.options().dtype(out_code == SPUTNIK_HIP_F32 ? at::kFloat : st);

  // 1-D whenever there is a single replica, as src/sddmm_cuda.cu:43 does.
  Tensor out = (replicas == 1 || sum_replicas)
                   ? at::empty({topo.nonzeros}, out_options)
                   : at::empty({replicas, topo.nonzeros}, out_options);
  const size_t ws_bytes = sum_replicas
                              ? sputnik_hip_sddmm_sum_workspace_bytes(m, k, n, topo.nonzeros)
                              : sputnik_hip_sddmm_workspace_bytes(m, k, n, topo.nonzeros);
  const Workspace workspace = plan_or_workspace(plan, ws_bytes, lhs);
  void* const ws = workspace.ptr;
  const int planned = workspace.planned;
  if (sum_replicas) {
    // sum over the batch inside the call (sputnik_hip.h: sddmm_sum_batched)
    const size_t scratch_bytes =
        sputnik_hip_sddmm_sum_scratch_bytes(m, k, n, topo.nonzeros, replicas);
    Tensor scratch;
    if (scratch_bytes > 0)
      scratch = at::empty({static_cast<int64_t>(scratch_bytes)}, lhs.options().dtype(at::kByte));
    check_status(sputnik_hip_sddmm_sum_typed(
                     m, k, n, topo.nonzeros, replicas, topo.row_indices.data_ptr<int>(),
                     topo.row_offsets.data_ptr<int>(), topo.column_indices.data_ptr<int>(),
                     lhs.data_ptr(), static_cast<int64_t>(m) * k, rhs.data_ptr(),
                     static_cast<int64_t>(n) * k, in_code, out.data_ptr<float>(), ws, ws_bytes,
                     planned, scratch_bytes ? scratch.data_ptr() : nullptr, scratch_bytes,
                     current_stream(lhs)),
                 planned ? "sddmm_sum_planned" : "sddmm_sum");
    return out;
  }
  const int status = sputnik_hip_sddmm_typed(
      m, k, n, topo.nonzeros, replicas, topo.row_indices.data_ptr<int>(),
      topo.row_offsets.data_ptr<int>(), topo.column_indices.data_ptr<int>(), lhs.data_ptr(),
      static_cast<int64_t>(m) * k, rhs.data_ptr(), static_cast<int64_t>(n) * k, in_code,
      out.data_ptr(), topo.nonzeros, out_code, ws, ws_bytes, planned, current_stream(lhs));
  if (status == SPUTNIK_HIP_UNSUPPORTED && out_code != SPUTNIK_HIP_F32) {
    // a half output of a product that takes several passes: float32 result, rounded once
    return sddmm_impl(m64, n64, row_indices, row_offsets, column_indices, lhs, rhs, plan, false,
                      SPUTNIK_HIP_F32).to(st);
  }
  check_status(status, planned ? "sddmm_planned" : "sddmm");
  return out;
}

// sddmm with the result stored in the operands' half type (float32 operands: as sddmm)
Tensor sddmm_narrow(int64_t m, int64_t n, const Tensor& row_indices, const Tensor& row_offsets,
                    const Tensor& column_indices, const Tensor& lhs, const Tensor& rhs) {
  const int code = type_code(at::promote_types(lhs.scalar_type(), rhs.scalar_type()));
  return sddmm_impl(m, n, row_indices, row_offsets, column_indices, lhs, rhs, c10::nullopt, false,
                    code);
}

Tensor sddmm(int64_t m, int64_t n, const Tensor& row_indices, const Tensor& row_offsets,
             const Tensor& column_indices, const Tensor& lhs, const Tensor& rhs) {
  return sddmm_impl(m, n, row_indices, row_offsets, column_indices, lhs, rhs, c10::nullopt);
}

// ---------------------------------------------------------------------------
// Static topologies: run the topology-only pre-pass once, keep the result (a
// uint8 "plan" tensor) and hand it to the *_planned ops.  The reference
// re-derives everything per call (src/spmm_cuda.cu:48-57).
// ---------------------------------------------------------------------------
Tensor make_plan_tensor(size_t bytes, const Tensor& like) {
  return at::empty({static_cast<int64_t>(std::max<size_t>(bytes, 16))},
                   like.options().dtype(at::kByte));
}

// The plan of one m-row topology for the sizes (m, a, b), in the library's order ((m, k, n) for
// the products, (m, n, d) for the attention): `bytes_of` sizes it, `prepass` fills it -- unless
// `served` is given and says the kernels do not take the shape (the plan is then never read).
using PlanBytes = size_t (*)(int, int, int, int);
using PlanServed = int (*)(int, int, int, int);
using PlanPrepass = int (*)(int, int, int, int, const int*, const int*, const int*, void*, size_t,
                            sputnik_hip_stream_t);

Tensor make_plan(const char* what, int m, int a, int b, const Tensor& row_indices,
                 const Tensor& row_offsets, const Tensor& column_indices, PlanBytes bytes_of,
                 PlanPrepass prepass, PlanServed served = nullptr) {
  TORCH_CHECK(row_offsets.is_cuda(), "row_offsets must be a GPU (HIP) tensor");
  const c10::DeviceGuard guard(row_offsets.device());
  const Topology topo = check_topology(m, row_indices, row_offsets, column_indices, row_offsets);
  const size_t bytes = bytes_of(m, a, b, topo.nonzeros);
  Tensor plan = make_plan_tensor(bytes, row_offsets);
  if (served == nullptr || served(m, a, b, topo.nonzeros))
    check_status(prepass(m, a, b, topo.nonzeros, topo.row_indices.data_ptr<int>(),
                         topo.row_offsets.data_ptr<int>(), topo.column_indices.data_ptr<int>(),
                         bytes ? plan.data_ptr() : nullptr, bytes, current_stream(row_offsets)),
                 what);
  return plan;
}

Tensor spmm_plan(int64_t m, int64_t k, int64_t n, const Tensor& row_indices,
                 const Tensor& row_offsets, const Tensor& column_indices) {
  return make_plan("spmm_plan", to_int(m, "m"), to_int(k, "k"), to_int(n, "n"), row_indices,
                   row_offsets, column_indices, sputnik_hip_spmm_workspace_bytes, sputnik_hip_spmm_plan);
}

Tensor sddmm_plan(int64_t m, int64_t n, int64_t k, const Tensor& row_indices,
                  const Tensor& row_offsets, const Tensor& column_indices) {
  return make_plan("sddmm_plan", to_int(m, "m"), to_int(k, "k"), to_int(n, "n"), row_indices,
                   row_offsets, column_indices, sputnik_hip_sddmm_workspace_bytes, sputnik_hip_sddmm_plan);
}

// Several summed products of one shape in one call: the weight gradients of a group of
// projections (sputnik_hip.h: sddmm_sum_group_planned).  float32, 3-D contiguous operands,
// one planned workspace per weight; rhs is shared.
std::vector<Tensor> sddmm_sum_group_planned(int64_t m64, int64_t n64,
                                            const std::vector<Tensor>& row_indices,
                                            const std::vector<Tensor>& row_offsets,
                                            const std::vector<Tensor>& column_indices,
                                            const std::vector<Tensor>& lhs_in, const Tensor& rhs_in,
                                            const std::vector<Tensor>& plans) {
  const int m = to_int(m64, "m"), n = to_int(n64, "n");
  const size_t count = lhs_in.size();
  TORCH_CHECK(count >= 1 && count <= 4, "sddmm_sum_group: one to four products, got ", count);
  TORCH_CHECK(row_indices.size() == count && row_offsets.size() == count &&
                  column_indices.size() == count && plans.size() == count,
              "sddmm_sum_group: one topology, lhs and plan per product");
  const Tensor rhs = as_float(rhs_in, "rhs_matrix");
  TORCH_CHECK(rhs.dim() == 3 && rhs.size(1) == n, "sddmm_sum_group: rhs_matrix should be [replicas, n = ",
              n, ", k]");
  const int replicas = to_int(rhs.size(0), "replicas"), k = to_int(rhs.size(2), "k");
  const c10::DeviceGuard guard(rhs.device());
  std::vector<Tensor> lhs(count), outs(count), scratch(count);
  std::vector<Topology> topo;
  std::vector<sputnik_hip_sddmm_sum_problem> problems(count);
  for (size_t p = 0; p < count; ++p) {
    lhs[p] = as_float(lhs_in[p], "lhs_matrix");
    TORCH_CHECK(lhs[p].device() == rhs.device() && lhs[p].dim() == 3 && lhs[p].size(0) == replicas &&
                    lhs[p].size(1) == m && lhs[p].size(2) == k,
                "sddmm_sum_group: lhs_matrix ", p, " should be [", replicas, ", ", m, ", ", k, "] on ",
                rhs.device());
    topo.push_back(check_topology(m, row_indices[p], row_offsets[p], column_indices[p], lhs[p]));
    const int nnz = topo[p].nonzeros;
    outs[p] = at::empty({nnz}, rhs.options());
    const size_t ws_bytes = sputnik_hip_sddmm_sum_workspace_bytes(m, k, n, nnz);
    check_plan(plans[p], ws_bytes, rhs);
    const size_t scratch_bytes = sputnik_hip_sddmm_sum_scratch_bytes(m, k, n, nnz, replicas);
    if (scratch_bytes > 0)
      scratch[p] = at::empty({static_cast<int64_t>(scratch_bytes)}, rhs.options().dtype(at::kByte));
    sputnik_hip_sddmm_sum_problem& q = problems[p];
    q.row_indices = topo[p].row_indices.data_ptr<int>();
    q.row_offsets = topo[p].row_offsets.data_ptr<int>();
    q.column_indices = topo[p].column_indices.data_ptr<int>();
    q.lhs = lhs[p].data_ptr<float>();
    q.rhs = rhs.data_ptr<float>();
    q.out = outs[p].data_ptr<float>();
    q.workspace = ws_bytes ? plans[p].data_ptr() : nullptr;
    q.workspace_bytes = ws_bytes;
    q.scratch = scratch_bytes ? scratch[p].data_ptr() : nullptr;
    q.scratch_bytes = scratch_bytes;
    q.nonzeros = nnz;
  }
  check_status(sputnik_hip_sddmm_sum_group_planned(m, k, n, replicas, static_cast<int>(count),
                                                   problems.data(), static_cast<int64_t>(m) * k,
                                                   static_cast<int64_t>(n) * k, current_stream(rhs)),
               "sddmm_sum_group_planned");
  return outs;
}

// the summed product has a plan of its own (sputnik_hip.h: sddmm_sum_plan)
Tensor sddmm_sum_plan(int64_t m, int64_t n, int64_t k, const Tensor& row_indices,
                      const Tensor& row_offsets, const Tensor& column_indices) {
  return make_plan("sddmm_sum_plan", to_int(m, "m"), to_int(k, "k"), to_int(n, "n"), row_indices,
                   row_offsets, column_indices, sputnik_hip_sddmm_sum_workspace_bytes,
                   sputnik_hip_sddmm_sum_plan);
}

Tensor sddmm_planned(int64_t m, int64_t n, const Tensor& row_indices, const Tensor& row_offsets,
                     const Tensor& column_indices, const Tensor& lhs, const Tensor& rhs,
                     const Tensor& plan) {
  return sddmm_impl(m, n, row_indices, row_offsets, column_indices, lhs, rhs, plan);
}

// sum over the replicas of sddmm: the gradient of values shared by a batch
Tensor sddmm_sum(int64_t m, int64_t n, const Tensor& row_indices, const Tensor& row_offsets,
                 const Tensor& column_indices, const Tensor& lhs, const Tensor& rhs) {
  return sddmm_impl(m, n, row_indices, row_offsets, column_indices, lhs, rhs, c10::nullopt, true);
}

Tensor sddmm_sum_planned(int64_t m, int64_t n, const Tensor& row_indices,
                         const Tensor& row_offsets, const Tensor& column_indices,
                         const Tensor& lhs, const Tensor& rhs, const Tensor& plan) {
  return sddmm_impl(m, n, row_indices, row_offsets, column_indices, lhs, rhs, plan, true);
}

Tensor sparse_softmax_scaled(const Tensor& values_in, const Tensor& row_indices,
                             const Tensor& row_offsets, const Tensor& column_indices,
                             double scale) {
  // float16 / bfloat16 values are read and written as such (half the traffic of
  // src/softmax_cuda.cu:38-42), the result has the values' type
  const Tensor values = as_storage(values_in, "values");
  TORCH_CHECK(values.dim() == 1 || values.dim() == 2,
              "values should have 1 or 2 dimensions, got ", values.dim());
  const c10::DeviceGuard guard(values.device());
  const int m = to_int(row_indices.size(0), "m");
  const Topology topo = check_topology(m, row_indices, row_offsets, column_indices, values);
  TORCH_CHECK(values.size(-1) == topo.nonzeros, "number of values (", values.size(-1),
              ") must equal the number of column_indices (", topo.nonzeros, ")");
  const int replicas = values.dim() == 2 ? to_int(values.size(0), "replicas") : 1;

  Tensor out = at::empty_like(values);
  check_status(sputnik_hip_sparse_softmax_typed(
                   m, /*n=*/-1, topo.nonzeros, replicas, values.data_ptr(), topo.nonzeros,
                   topo.row_indices.data_ptr<int>(), topo.row_offsets.data_ptr<int>(),
                   topo.column_indices.data_ptr<int>(), static_cast<float>(scale),
                   out.data_ptr(), topo.nonzeros, type_code(values.scalar_type()),
                   current_stream(values)),
               "sparse_softmax");
  return out;
}

Tensor sparse_softmax(const Tensor& values, const Tensor& row_indices, const Tensor& row_offsets,
                      const Tensor& column_indices) {
  return sparse_softmax_scaled(values, row_indices, row_offsets, column_indices, 1.0);
}

// grad of softmax(scale * x) w.r.t. x; softmax_out / grad_out [nnz] or [R,nnz].
Tensor sparse_softmax_backward(const Tensor& softmax_out_in, const Tensor& grad_out_in,
                               const Tensor& row_offsets_in, double scale) {
  // one storage type for both operands and the result (the wider one if they differ)
  const auto st = at::promote_types(softmax_out_in.scalar_type(), grad_out_in.scalar_type());
  const Tensor y = as_storage(softmax_out_in, "softmax_out").to(st);
  const Tensor g = as_storage(grad_out_in, "grad_out").to(st);
  TORCH_CHECK(y.sizes() == g.sizes(), "softmax_out and grad_out must have one shape, got ",
              y.sizes(), " and ", g.sizes());
  TORCH_CHECK(y.dim() == 1 || y.dim() == 2, "softmax_out should have 1 or 2 dimensions, got ",
              y.dim());
  TORCH_CHECK(y.device() == g.device(), "softmax_out and grad_out must be on one device");
  const c10::DeviceGuard guard(y.device());
  const Tensor row_offsets = as_index(row_offsets_in, "row_offsets", y);
  TORCH_CHECK(row_offsets.size(0) >= 1, "row_offsets must not be empty");
  const int m = to_int(row_offsets.size(0) - 1, "m");
  const int nonzeros = to_int(y.size(-1), "nonzeros");
  const int replicas = y.dim() == 2 ? to_int(y.size(0), "replicas") : 1;
  Tensor out = at::empty_like(y);
  check_status(sputnik_hip_sparse_softmax_backward_typed(
                   m, nonzeros, replicas, y.data_ptr(), nonzeros, g.data_ptr(), nonzeros,
                   row_offsets.data_ptr<int>(), static_cast<float>(scale), out.data_ptr(),
                   nonzeros, type_code(st), current_stream(y)),
               "sparse_softmax_backward");
  return out;
}

// Returns {values_t, row_offsets_t, column_indices_t} (+ {permutation} when
// asked).  values may be [nnz] (reference contract) or [R,nnz] (extension).
std::vector<Tensor> csr_transpose_impl(int64_t m64, int64_t n64, const Tensor& values_in,
                                       const Tensor& row_offsets_in,
                                       const Tensor& column_indices_in, bool want_permutation,
                                       bool checked) {
  const int m = to_int(m64, "m"), n = to_int(n64, "n");
  // float16 / bfloat16 values are read as they are by the gather that moves them
  // (sputnik_hip_csr_transpose_typed); the transposed values are float32 either way
  const Tensor values = as_storage(values_in, "values");
  const bool half_values = values.scalar_type() != at::kFloat;
  TORCH_CHECK(values.dim() == 1 || values.dim() == 2,
              "values should have 1 (or, as an extension, 2) dimensions, got ", values.dim());
  const c10::DeviceGuard guard(values.device());
  const Tensor row_offsets = as_index(row_offsets_in, "row_offsets", values);
  const Tensor column_indices = as_index(column_indices_in, "column_indices", values);
  TORCH_CHECK(values.size(-1) == column_indices.size(0),
              "expected same number of values and indices, got ", values.size(-1), " and ",
              column_indices.size(0));
  TORCH_CHECK(row_offsets.size(0) == m + 1, "expected m+1 row offsets, got ",
              row_offsets.size(0), " for m = ", m);
  const int nonzeros = to_int(column_indices.size(0), "nonzeros");
  const int replicas = values.dim() == 2 ? to_int(values.size(0), "replicas") : 1;

  const auto index_options = values.options().dtype(at::kInt);
  Tensor out_values = at::empty(values.sizes(), values.options().dtype(at::kFloat));
  Tensor out_row_offsets = at::empty({n + 1}, index_options);
  Tensor out_column_indices = at::empty({nonzeros}, index_options);
  Tensor permutation;
  if (want_permutation || half_values) permutation = at::empty({nonzeros}, index_options);

  const size_t ws_bytes = sputnik_hip_csr_transpose_workspace_bytes(m, n, nonzeros);
  Tensor workspace =
      at::empty({static_cast<int64_t>(ws_bytes)}, values.options().dtype(at::kByte));
  // csr_transpose itself is asynchronous like the reference's (src/transpose_cuda.cu:90-99:
  // no host round trip).  The form that also returns the permutation takes a `checked` flag:
  // a cache that is going to KEEP the result (once per static topology) sets it and gets the
  // checked entry, which waits for the stream and reports a pattern the transpose is not
  // defined for (a row storing a column twice, a column out of range) instead of handing out
  // a silently wrong permutation; a per-call user leaves it off and stays asynchronous and
  // capturable (the wait is illegal inside a stream capture).
  checked = checked && want_permutation;
  int status;
  if (half_values) {
    status = sputnik_hip_csr_transpose_typed(
        m, n, nonzeros, replicas, values.data_ptr(), type_code(values.scalar_type()), nonzeros,
        row_offsets.data_ptr<int>(), column_indices.data_ptr<int>(), out_values.data_ptr<float>(),
        nonzeros, out_row_offsets.data_ptr<int>(), out_column_indices.data_ptr<int>(),
        permutation.data_ptr<int>(), workspace.data_ptr(), ws_bytes, checked ? 1 : 0,
        current_stream(values));
  } else {
    const auto entry =
        checked ? sputnik_hip_csr_transpose_checked : sputnik_hip_csr_transpose;
    status = entry(m, n, nonzeros, replicas, values.data_ptr<float>(), nonzeros,
                   row_offsets.data_ptr<int>(), column_indices.data_ptr<int>(),
                   out_values.data_ptr<float>(), nonzeros, out_row_offsets.data_ptr<int>(),
                   out_column_indices.data_ptr<int>(),
                   want_permutation ? permutation.data_ptr<int>() : nullptr, workspace.data_ptr(),
                   ws_bytes, current_stream(values));
  }
  TORCH_CHECK(!(checked && status == SPUTNIK_HIP_INVALID_ARGUMENT),
              "torch_sputnik::csr_transpose_with_permutation: the pattern is not a valid CSR "
              "matrix for a transpose (a row stores a column twice, or a column index is out of "
              "range)");
  check_status(status, "csr_transpose");
  std::vector<Tensor> out{out_values, out_row_offsets, out_column_indices};
  if (want_permutation) out.push_back(permutation);
  return out;
}

std::vector<Tensor> csr_transpose(int64_t m, int64_t n, const Tensor& values,
                                  const Tensor& row_offsets, const Tensor& column_indices) {
  return csr_transpose_impl(m, n, values, row_offsets, column_indices, false, false);
}

std::vector<Tensor> csr_transpose_with_permutation(int64_t m, int64_t n, const Tensor& values,
                                                   const Tensor& row_offsets,
                                                   const Tensor& column_indices, bool checked) {
  return csr_transpose_impl(m, n, values, row_offsets, column_indices, true, checked);
}

// ---- attention dropout (sputnik_hip.h, "Attention dropout") ----
// One call's dropout: p, the Philox state and the int64 [2] device tensor that receives the
// {seed, offset} the kernels resolve.  Fresh draws come from the device's default generator,
// as torch.nn.functional.dropout's do: philox_cuda_state(4) under the generator's mutex gives
// the offset before the call and advances it by 4, or, during graph capture, the seed and
// offset pointers every replay refreshes.  A replay (`rng_state` given) reads the state from
// that tensor and consumes nothing.
struct Drop {
  double p = 0.0;
  sputnik_hip_philox_state rng{};
  Tensor rng_state;
  int64_t* rng_state_out = nullptr;   // NULL on a replay: the state is the input
};

void check_p(double p) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout probability must lie in [0, 1), got ", p);
}

// The Philox state of one call on `like`'s device: the replay of `rng_state`, or a fresh draw
// of 4 from the device's default generator.
Drop draw_state(const c10::optional<Tensor>& rng_state, const Tensor& like) {
  Drop d;
  if (rng_state.has_value() && rng_state->defined()) {
    const Tensor& st = *rng_state;
    TORCH_CHECK(st.scalar_type() == at::kLong && st.numel() == 2 && st.is_contiguous() &&
                    st.device() == like.device(),
                "rng_state must be a contiguous int64 [2] tensor on ", like.device());
    d.rng_state = st;
    d.rng.seed_ptr = st.data_ptr<int64_t>();
    d.rng.offset_ptr = st.data_ptr<int64_t>() + 1;
    return d;
  }
  d.rng_state = at::empty({2}, like.options().dtype(at::kLong));
  d.rng_state_out = d.rng_state.data_ptr<int64_t>();
  auto* gen = at::get_generator_or_default<at::CUDAGeneratorImpl>(
      c10::nullopt, at::cuda::detail::getDefaultCUDAGenerator(like.device().index()));
  at::PhiloxCudaState state;
  {
    std::lock_guard<std::mutex> lock(gen->mutex_);
    state = gen->philox_cuda_state(4);
  }
  if (state.captured_) {
    d.rng.seed_ptr = state.seed_.ptr;
    d.rng.offset_ptr = state.offset_.ptr;
    d.rng.offset_intragraph = state.offset_intragraph_;
  } else {
    d.rng.seed = state.seed_.val;
    d.rng.offset = state.offset_.val;
  }
  return d;
}

Drop make_drop(double p, const c10::optional<Tensor>& rng_state, const Tensor& like) {
  check_p(p);
  // p = 0 drops nothing and draws nothing: no state exists, and rng_state stays undefined
  // (None in Python).  ops.sparse_dropout(values, 0) comes here; the attention ops refuse p = 0.
  const bool replay = rng_state.has_value() && rng_state->defined();
  Drop d = replay || p != 0.0 ? draw_state(rng_state, like) : Drop();
  d.p = p;
  return d;
}

// out = x * keep * scale on a values array ([nnz], or [R, width] with a unit last stride), in
// x's type; row r is replica r.
Tensor dropout_values(const Tensor& x_in, const Drop& d) {
  TORCH_CHECK(x_in.is_cuda(), "sparse_dropout: values must be a GPU (HIP) tensor");
  TORCH_CHECK(x_in.dim() == 1 || x_in.dim() == 2, "sparse_dropout: values must be [nnz] or [R, width]");
  const int dtype = type_code(x_in.scalar_type());
  TORCH_CHECK(dtype >= 0, "sparse_dropout: expected float32, float16 or bfloat16 values, got ",
              x_in.scalar_type());
  const Tensor x = x_in.dim() == 1 ? x_in.contiguous().view({1, -1})
                                   : (x_in.stride(1) == 1 ? x_in : x_in.contiguous());
  Tensor out = at::empty(x.sizes(), x.options());
  const int rows = to_int(x.size(0), "rows"), width = to_int(x.size(1), "width");
  check_status(sputnik_hip_sparse_dropout_typed(rows, width, 0, dtype, x.data_ptr(),
                                                std::max<int64_t>(x.stride(0), width), out.data_ptr(),
                                                width, d.p, d.rng, d.rng_state_out,
                                                current_stream(x)),
               "sparse_dropout");
  return x_in.dim() == 1 ? out.view(x_in.sizes()) : out;
}

// -> {out, rng_state}
std::vector<Tensor> sparse_dropout(const Tensor& values, double p, const c10::optional<Tensor>& rng_state) {
  const c10::DeviceGuard guard(values.device());
  const Drop d = make_drop(p, rng_state, values);
  return {dropout_values(values, d), d.rng_state};
}

// What the fused attention ops return: {out}, {out, lse}, or with dropout
// {out, lse or undefined, rng_state}.
std::vector<Tensor> attention_result(const Tensor& out, const Tensor& lse, bool want_lse, const Drop* drop) {
  if (drop != nullptr) return {out, want_lse ? lse : Tensor(), drop->rng_state};
  if (want_lse) return {out, lse};
  return {out};
}

// Runs one of a layout's four C forward functions.  `args(forward, tail...)` holds the
// layout's argument list up to lse_stride; the tail is [p, rng, rng_state_out,] workspace,
// workspace_bytes, stream.  The workspace is the plan if one is given (checked), else fresh.
template <typename Args, typename F, typename FP, typename FD, typename FPD>
int run_forward(const Args& args, F unplanned, FP planned, FD unplanned_dropout, FPD planned_dropout,
                const c10::optional<Tensor>& plan, size_t ws_bytes, const Tensor& like, const Drop* drop) {
  const Workspace ws = plan_or_workspace(plan, ws_bytes, like);   // (never empty where the kernels serve)
  const sputnik_hip_stream_t stream = current_stream(like);
  auto with_workspace = [&](auto fresh, auto from_plan, auto... dropout) {
    return ws.planned ? args(from_plan, dropout..., static_cast<const void*>(ws.ptr), ws_bytes, stream)
                      : args(fresh, dropout..., ws.ptr, ws_bytes, stream);
  };
  return drop != nullptr
             ? with_workspace(unplanned_dropout, planned_dropout, drop->p, drop->rng, drop->rng_state_out)
             : with_workspace(unplanned, planned);
}

// Fused softmax(scale * sddmm(q, k)) @ v over a fixed mask
// (modules/sparse_attention.py:66-82).  q [R,m,d] / [m,d]; k, v [R,n,d] / [n,d].
// Shapes the fused kernel does not serve are composed from the three operators.
std::vector<Tensor> sparse_attention_impl(const Tensor& q_in, const Tensor& k_in,
                                          const Tensor& v_in, const Tensor& row_indices,
                                          const Tensor& row_offsets,
                                          const Tensor& column_indices, double scale,
                                          bool want_lse,
                                          const c10::optional<Tensor>& plan = c10::nullopt,
                                          const Drop* drop = nullptr) {
  const Tensor q = as_float(q_in, "query");
  const Tensor k = as_float(k_in, "key");
  const Tensor v = as_float(v_in, "value");
  TORCH_CHECK(q.dim() == 2 || q.dim() == 3, "expected 2-dim or 3-dim query, got ", q.dim());
  TORCH_CHECK(k.dim() == q.dim() && v.dim() == q.dim(), "query, key, value must match in dims");
  TORCH_CHECK(k.sizes() == v.sizes(), "key and value must have one shape");
  TORCH_CHECK(q.size(-1) == k.size(-1), "query and key must have one head dimension");
  TORCH_CHECK(q.device() == k.device() && q.device() == v.device(),
              "query, key, value must be on one device");
  const c10::DeviceGuard guard(q.device());
  const int m = to_int(q.size(-2), "m"), n = to_int(k.size(-2), "n");
  const int d = to_int(q.size(-1), "d");
  const int replicas = q.dim() == 3 ? to_int(q.size(0), "replicas") : 1;
  TORCH_CHECK(q.dim() == 2 || k.size(0) == replicas, "first dim of query and key must match");
  const Topology topo = check_topology(m, row_indices, row_offsets, column_indices, q);

  if (!sputnik_hip_sparse_attention_supported(m, n, d, topo.nonzeros)) {
    TORCH_CHECK(!want_lse || drop != nullptr, "sparse_attention_with_lse: head dimension ", d,
                " is not served by the fused kernel (64 is)");
    Tensor weights = sparse_softmax_scaled(
        sddmm(m, n, topo.row_indices, topo.row_offsets, topo.column_indices, q, k),
        topo.row_indices, topo.row_offsets, topo.column_indices, scale);
    if (drop != nullptr) weights = dropout_values(weights, *drop);
    Tensor out = spmm(m, n, weights, topo.row_indices, topo.row_offsets, topo.column_indices, v);
    return attention_result(out, Tensor(), false, drop);   // (no lse on this route)
  }
  Tensor out = at::empty_like(q);
  Tensor lse;
  if (want_lse)
    lse = q.dim() == 3 ? at::empty({replicas, m}, q.options()) : at::empty({m}, q.options());
  const size_t ws_bytes = sputnik_hip_sparse_attention_workspace_bytes(m, n, d, topo.nonzeros);
  auto args = [&](auto forward, auto... tail) {
    return forward(m, n, d, topo.nonzeros, replicas, topo.row_indices.data_ptr<int>(),
                   topo.row_offsets.data_ptr<int>(), topo.column_indices.data_ptr<int>(),
                   q.data_ptr<float>(), static_cast<int64_t>(m) * d, k.data_ptr<float>(),
                   static_cast<int64_t>(n) * d, v.data_ptr<float>(), static_cast<int64_t>(n) * d,
                   static_cast<float>(scale), out.data_ptr<float>(), static_cast<int64_t>(m) * d,
                   want_lse ? lse.data_ptr<float>() : nullptr, m, tail...);
  };
  check_status(run_forward(args, sputnik_hip_sparse_attention_forward,
                           sputnik_hip_sparse_attention_forward_planned,
                           sputnik_hip_sparse_attention_forward_dropout,
                           sputnik_hip_sparse_attention_forward_planned_dropout, plan, ws_bytes, q, drop),
               drop != nullptr ? "sparse_attention_dropout"
                               : plan.has_value() ? "sparse_attention_planned" : "sparse_attention");
  return attention_result(out, lse, want_lse, drop);
}

// {out, lse, rng_state}: the fused attention with dropout p > 0 on the attention weights
// (lse undefined where the composed route serves the call: head dimension other than 64).
std::vector<Tensor> sparse_attention_dropout(const Tensor& q, const Tensor& k, const Tensor& v,
                                             const Tensor& row_indices, const Tensor& row_offsets,
                                             const Tensor& column_indices, double scale, double p,
                                             const c10::optional<Tensor>& plan) {
  TORCH_CHECK(p > 0.0 && p < 1.0, "sparse_attention_dropout: p must lie in (0, 1), got ", p);
  const c10::DeviceGuard guard(q.device());
  const Drop drop = make_drop(p, c10::nullopt, q);
  return sparse_attention_impl(q, k, v, row_indices, row_offsets, column_indices, scale, true, plan,
                               &drop);
}

Tensor sparse_attention(const Tensor& q, const Tensor& k, const Tensor& v,
                        const Tensor& row_indices, const Tensor& row_offsets,
                        const Tensor& column_indices, double scale) {
  return sparse_attention_impl(q, k, v, row_indices, row_offsets, column_indices, scale, false)[0];
}

// {out, lse}: lse[r, i] = log sum_j exp(scale * <q_i, k_j>) over the stored j
// (-inf for rows without entries), what a backward needs to rebuild the weights.
std::vector<Tensor> sparse_attention_with_lse(const Tensor& q, const Tensor& k, const Tensor& v,
                                              const Tensor& row_indices,
                                              const Tensor& row_offsets,
                                              const Tensor& column_indices, double scale) {
  return sparse_attention_impl(q, k, v, row_indices, row_offsets, column_indices, scale, true);
}

// Empty plan (numel 0 is never returned; 16 bytes) when the fused kernel does not
// serve the shape: sparse_attention_planned then composes the three operators.
Tensor sparse_attention_plan(int64_t m, int64_t n, int64_t d, const Tensor& row_indices,
                             const Tensor& row_offsets, const Tensor& column_indices) {
  return make_plan("sparse_attention_plan", to_int(m, "m"), to_int(n, "n"), to_int(d, "d"),
                   row_indices, row_offsets, column_indices, sputnik_hip_sparse_attention_workspace_bytes,
                   sputnik_hip_sparse_attention_plan, sputnik_hip_sparse_attention_supported);
}

Tensor sparse_attention_planned(const Tensor& q, const Tensor& k, const Tensor& v,
                                const Tensor& row_indices, const Tensor& row_offsets,
                                const Tensor& column_indices, double scale, const Tensor& plan) {
  return sparse_attention_impl(q, k, v, row_indices, row_offsets, column_indices, scale, false,
                               plan)[0];
}

// {out, lse} through a plan of sparse_attention_plan: the forward of the fused backward.
std::vector<Tensor> sparse_attention_with_lse_planned(const Tensor& q, const Tensor& k,
                                                      const Tensor& v, const Tensor& row_indices,
                                                      const Tensor& row_offsets,
                                                      const Tensor& column_indices, double scale,
                                                      const Tensor& plan) {
  return sparse_attention_impl(q, k, v, row_indices, row_offsets, column_indices, scale, true,
                               plan);
}

// {out, lse} or, with p > 0, {out, lse, rng_state}: the fused attention forward in the row-group
// form (sputnik_hip_sparse_attention_rows_forward: head dimension 128), with dropout p on the
// weights when p > 0.  float32 q [R,m,d] / [m,d]; k, v [R,n,d] / [n,d]; no plan.  A shape the
// kernel does not serve is an error.
std::vector<Tensor> sparse_attention_rows(const Tensor& q_in, const Tensor& k_in, const Tensor& v_in,
                                          const Tensor& row_indices, const Tensor& row_offsets,
                                          const Tensor& column_indices, double scale, double p) {
  for (const Tensor* t : {&q_in, &k_in, &v_in})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat,
                "sparse_attention_rows: query, key, value must be float32 GPU (HIP) tensors");
  check_p(p);
  const Tensor q = q_in.contiguous(), k = k_in.contiguous(), v = v_in.contiguous();
  TORCH_CHECK(q.dim() == 2 || q.dim() == 3, "expected 2-dim or 3-dim query, got ", q.dim());
  TORCH_CHECK(k.dim() == q.dim() && v.dim() == q.dim(), "query, key, value must match in dims");
  TORCH_CHECK(k.sizes() == v.sizes(), "key and value must have one shape");
  TORCH_CHECK(q.size(-1) == k.size(-1), "query and key must have one head dimension");
  TORCH_CHECK(q.device() == k.device() && q.device() == v.device(),
              "query, key, value must be on one device");
  const c10::DeviceGuard guard(q.device());
  const int m = to_int(q.size(-2), "m"), n = to_int(k.size(-2), "n");
  const int d = to_int(q.size(-1), "d");
  const int replicas = q.dim() == 3 ? to_int(q.size(0), "replicas") : 1;
  TORCH_CHECK(q.dim() == 2 || k.size(0) == replicas, "first dim of query and key must match");
  const Topology topo = check_topology(m, row_indices, row_offsets, column_indices, q);
  TORCH_CHECK(sputnik_hip_sparse_attention_rows_supported(m, n, d, topo.nonzeros),
              "sparse_attention_rows: shape not served (head dimension 128, a mask with entries, "
              "m and n below 2^23)");
  const Drop drop = make_drop(p, c10::nullopt, q);
  Tensor out = at::empty_like(q);
  Tensor lse = q.dim() == 3 ? at::empty({replicas, m}, q.options()) : at::empty({m}, q.options());
  const int64_t qs = static_cast<int64_t>(m) * d, ks = static_cast<int64_t>(n) * d;
  check_status(sputnik_hip_sparse_attention_rows_forward(
                   m, n, d, topo.nonzeros, replicas, topo.row_indices.data_ptr<int>(),
                   topo.row_offsets.data_ptr<int>(), topo.column_indices.data_ptr<int>(),
                   q.data_ptr<float>(), qs, k.data_ptr<float>(), ks, v.data_ptr<float>(), ks,
                   static_cast<float>(scale), out.data_ptr<float>(), qs, lse.data_ptr<float>(), m,
                   drop.p, drop.rng, drop.rng_state_out, current_stream(q)),
               "sparse_attention_rows");
  if (p > 0.0) return {out, lse, drop.rng_state};
  return {out, lse};
}

// {grad_q, grad_k, grad_v} of the fused attention (sputnik_hip_sparse_attention_backward),
// empty tensors for those not wanted.  q [R,m,d] / [m,d]; k, v [R,n,d] / [n,d]; out and
// grad_out as q; lse [R,m] / [m] from the forward.  The transposed mask (t_*, permutation) is
// needed for grad_k / grad_v only.  p > 0 replays the forward's mask from rng_state.
std::vector<Tensor> sparse_attention_backward(
    const Tensor& q_in, const Tensor& k_in, const Tensor& v_in, const Tensor& out_in,
    const Tensor& grad_out_in, const Tensor& lse_in, const Tensor& row_indices,
    const Tensor& row_offsets, const Tensor& column_indices,
    const c10::optional<Tensor>& t_row_indices, const c10::optional<Tensor>& t_row_offsets,
    const c10::optional<Tensor>& t_column_indices, const c10::optional<Tensor>& permutation,
    double scale, double p, const c10::optional<Tensor>& rng_state, bool want_q, bool want_k,
    bool want_v) {
  const Tensor q = as_float(q_in, "query");
  const Tensor k = as_float(k_in, "key");
  const Tensor v = as_float(v_in, "value");
  const Tensor out = as_float(out_in, "out");
  const Tensor grad_out = as_float(grad_out_in, "grad_out");
  const Tensor lse = as_float(lse_in, "lse");
  TORCH_CHECK(q.dim() == 2 || q.dim() == 3, "expected 2-dim or 3-dim query, got ", q.dim());
  TORCH_CHECK(k.dim() == q.dim() && v.dim() == q.dim(), "query, key, value must match in dims");
  TORCH_CHECK(k.sizes() == v.sizes(), "key and value must have one shape");
  TORCH_CHECK(out.sizes() == q.sizes() && grad_out.sizes() == q.sizes(),
              "out and grad_out must have the shape of query");
  TORCH_CHECK(q.size(-1) == k.size(-1), "query and key must have one head dimension");
  TORCH_CHECK(q.device() == k.device() && q.device() == v.device() &&
                  q.device() == out.device() && q.device() == grad_out.device() &&
                  q.device() == lse.device(),
              "query, key, value, out, grad_out, lse must be on one device");
  const c10::DeviceGuard guard(q.device());
  const int m = to_int(q.size(-2), "m"), n = to_int(k.size(-2), "n");
  const int d = to_int(q.size(-1), "d");
  const int replicas = q.dim() == 3 ? to_int(q.size(0), "replicas") : 1;
  TORCH_CHECK(q.dim() == 2 || k.size(0) == replicas, "first dim of query and key must match");
  TORCH_CHECK(lse.numel() == static_cast<int64_t>(replicas) * m, "lse must hold ", replicas,
              " x ", m, " values");
  const Topology topo = check_topology(m, row_indices, row_offsets, column_indices, q);
  TORCH_CHECK(sputnik_hip_sparse_attention_backward_supported(m, n, d, topo.nonzeros),
              "sparse_attention_backward: shape not served (head dimension 64 or 128, m * d and n * d "
              "below 2^30)");
  Topology t{};
  Tensor perm;
  if (want_k || want_v) {
    TORCH_CHECK(t_row_indices.has_value() && t_row_offsets.has_value() &&
                    t_column_indices.has_value(),
                "sparse_attention_backward: grad_k / grad_v need the transposed mask");
    t = check_topology(n, *t_row_indices, *t_row_offsets, *t_column_indices, q);
    TORCH_CHECK(t.nonzeros == topo.nonzeros, "the transposed mask must hold the mask's entries");
    if (p > 0.0) {
      TORCH_CHECK(permutation.has_value(), "sparse_attention_backward: dropout needs the permutation");
      perm = as_index(*permutation, "permutation", q);
      TORCH_CHECK(perm.size(0) == topo.nonzeros, "permutation must hold one index per entry");
    }
  }
  TORCH_CHECK(p == 0.0 || (rng_state.has_value() && rng_state->defined()),
              "sparse_attention_backward: dropout needs the forward's rng_state");
  const Drop drop = make_drop(p, rng_state, q);
  Tensor grad_q = want_q ? at::empty_like(q) : at::empty({0}, q.options());
  Tensor grad_k = want_k ? at::empty_like(k) : at::empty({0}, q.options());
  Tensor grad_v = want_v ? at::empty_like(v) : at::empty({0}, q.options());
  const size_t ws_bytes = sputnik_hip_sparse_attention_backward_workspace_bytes(
      m, n, d, topo.nonzeros, replicas);
  Tensor workspace = at::empty({static_cast<int64_t>(std::max<size_t>(ws_bytes, 16))},
                               q.options().dtype(at::kByte));
  const bool cols = want_k || want_v;
  const int64_t qs = static_cast<int64_t>(m) * d, ks = static_cast<int64_t>(n) * d;
  check_status(sputnik_hip_sparse_attention_backward(
                   m, n, d, topo.nonzeros, replicas, topo.row_indices.data_ptr<int>(),
                   topo.row_offsets.data_ptr<int>(), topo.column_indices.data_ptr<int>(),
                   cols ? t.row_indices.data_ptr<int>() : nullptr,
                   cols ? t.row_offsets.data_ptr<int>() : nullptr,
                   cols ? t.column_indices.data_ptr<int>() : nullptr,
                   perm.defined() ? perm.data_ptr<int>() : nullptr, q.data_ptr<float>(), qs,
                   k.data_ptr<float>(), ks, v.data_ptr<float>(), ks, static_cast<float>(scale),
                   out.data_ptr<float>(), qs, grad_out.data_ptr<float>(), qs,
                   lse.data_ptr<float>(), m, want_q ? grad_q.data_ptr<float>() : nullptr, qs,
                   want_k ? grad_k.data_ptr<float>() : nullptr, ks,
                   want_v ? grad_v.data_ptr<float>() : nullptr, ks, drop.p, drop.rng,
                   workspace.data_ptr(), ws_bytes, current_stream(q)),
               "sparse_attention_backward");
  return {grad_q, grad_k, grad_v};
}

// ---- the fused attention on half storage with strided head views (sputnik_hip.h:
// sparse_attention_heads_*) ----
struct HeadOperand {
  Tensor t;                      // keeps the storage alive
  int64_t batch, heads, rows, d;
  int64_t batch_stride, head_stride, row_stride;
};

// [B, H, rows, d], [R, rows, d] (H = 1) or [rows, d] (B = H = 1) with unit stride along d.
HeadOperand head_operand(const Tensor& x_in, const char* name) {
  TORCH_CHECK(x_in.is_cuda(), name, " must be a GPU (HIP) tensor, got ", x_in.device());
  TORCH_CHECK(x_in.dim() >= 2 && x_in.dim() <= 4, name, " must have 2, 3 or 4 dimensions, got ", x_in.dim());
  const Tensor x = x_in.stride(-1) == 1 ? x_in : x_in.contiguous();
  HeadOperand o;
  o.t = x;
  o.rows = x.size(-2);
  o.d = x.size(-1);
  o.row_stride = x.stride(-2);
  if (x.dim() == 4) {
    o.batch = x.size(0), o.heads = x.size(1);
    o.batch_stride = x.stride(0), o.head_stride = x.stride(1);
  } else if (x.dim() == 3) {
    o.batch = x.size(0), o.heads = 1;
    o.batch_stride = x.stride(0), o.head_stride = 0;
  } else {
    o.batch = 1, o.heads = 1;
    o.batch_stride = 0, o.head_stride = 0;
  }
  return o;
}

// What both heads ops ask of their operands (`op` names the op in the messages); -> the
// operands' type code.
int check_head_operands(const HeadOperand& q, const HeadOperand& k, const HeadOperand& v, int64_t out_type,
                        const char* op) {
  const auto st = q.t.scalar_type();
  const int dtype = type_code(st);
  TORCH_CHECK(dtype == SPUTNIK_HIP_F16 || dtype == SPUTNIK_HIP_BF16, op,
              ": expected float16 / bfloat16 operands, got ", st);
  TORCH_CHECK(k.t.scalar_type() == st && v.t.scalar_type() == st, op,
              ": query, key, value must have one type");
  TORCH_CHECK(q.t.dim() == k.t.dim() && q.t.dim() == v.t.dim(), "query, key, value must match in dims");
  TORCH_CHECK(k.t.sizes() == v.t.sizes(), "key and value must have one shape");
  TORCH_CHECK(q.d == k.d, "query and key must have one head dimension");
  TORCH_CHECK(q.batch == k.batch && q.heads == k.heads, "query and key must have one batch and head count");
  TORCH_CHECK(q.t.device() == k.t.device() && q.t.device() == v.t.device(),
              "query, key, value must be on one device");
  TORCH_CHECK(out_type == SPUTNIK_HIP_F32 || out_type == dtype, op,
              ": out_type is float32 or the operands' type");
  return dtype;
}

// q [.., m, 64], k and v [.., n, 64] of one half type (any strides with a unit last one);
// out in the layout of the [B, m, H, d] buffer it views ([B, m, E] for 4-D operands), stored
// as out_type (0 float32, else the operands' type); lse [.., m] float32 on request.
// A call the kernel does not serve is composed from the typed operators (no lse then).
std::vector<Tensor> sparse_attention_heads_run(const Tensor& q_in, const Tensor& k_in, const Tensor& v_in,
                                           const Tensor& row_indices, const Tensor& row_offsets,
                                           const Tensor& column_indices, double scale, int64_t out_type,
                                           bool want_lse, const c10::optional<Tensor>& plan,
                                           const Drop* drop = nullptr) {
  const HeadOperand q = head_operand(q_in, "query"), k = head_operand(k_in, "key"),
                    v = head_operand(v_in, "value");
  const int dtype = check_head_operands(q, k, v, out_type, "sparse_attention_heads");
  const auto st = q.t.scalar_type();
  const c10::DeviceGuard guard(q.t.device());
  const int m = to_int(q.rows, "m"), n = to_int(k.rows, "n"), d = to_int(q.d, "d");
  const int batch = to_int(q.batch, "batch"), heads = to_int(q.heads, "heads");
  const Topology topo = check_topology(m, row_indices, row_offsets, column_indices, q.t);
  const auto out_st = out_type == SPUTNIK_HIP_F32 ? at::kFloat : st;

  Tensor buffer, out;   // out: the [.., m, d] view of `buffer` the kernel writes
  if (q.t.dim() == 4) {
    buffer = at::empty({q.batch, q.rows, q.heads, q.d}, q.t.options().dtype(out_st));
    out = buffer.permute({0, 2, 1, 3});
  } else {
    out = buffer = at::empty(q.t.sizes(), q.t.options().dtype(out_st));
  }
  const HeadOperand o = head_operand(out, "out");
  std::vector<int64_t> lse_shape(q.t.sizes().begin(), q.t.sizes().end() - 1);
  Tensor lse = want_lse ? at::empty(lse_shape, q.t.options().dtype(at::kFloat)) : Tensor();

  const bool served = sputnik_hip_sparse_attention_heads_supported(
      m, n, d, topo.nonzeros, batch, heads, dtype, static_cast<int>(out_type), q.t.data_ptr(),
      q.batch_stride, q.head_stride, q.row_stride, k.t.data_ptr(), k.batch_stride, k.head_stride,
      k.row_stride, v.t.data_ptr(), v.batch_stride, v.head_stride, v.row_stride, o.t.data_ptr(),
      o.batch_stride, o.head_stride, o.row_stride);
  if (!served) {
    TORCH_CHECK(!want_lse || drop != nullptr, "sparse_attention_heads: lse needs a call the fused "
                "kernel serves (head dimension 64, 16-byte aligned views)");
    // the typed operators on per-head copies in the storage type: float32 scores and
    // weights, float32 product, narrowed into the output's layout
    const int64_t replicas = q.batch * q.heads;
    auto per_head = [&](const HeadOperand& x) {
      const Tensor flat = x.t.reshape({replicas, x.rows, x.d});
      return replicas == 1 ? flat[0] : flat;
    };
    const Tensor q3 = per_head(q), k3 = per_head(k), v3 = per_head(v);
    Tensor weights = sparse_softmax_scaled(
        sddmm(m, n, topo.row_indices, topo.row_offsets, topo.column_indices, q3, k3),
        topo.row_indices, topo.row_offsets, topo.column_indices, scale);
    if (drop != nullptr) weights = dropout_values(weights.dim() == 1 ? weights.view({1, -1}) : weights, *drop);
    const Tensor product = spmm(m, n, replicas == 1 ? weights.view({-1}) : weights, topo.row_indices,
                                topo.row_offsets, topo.column_indices, v3);
    out.copy_(product.reshape(out.sizes()));
    return attention_result(out, Tensor(), false, drop);
  }
  const size_t ws_bytes = sputnik_hip_sparse_attention_heads_workspace_bytes(m, n, d, topo.nonzeros);
  auto args = [&](auto forward, auto... tail) {
    return forward(m, n, d, topo.nonzeros, batch, heads, topo.row_indices.data_ptr<int>(),
                   topo.row_offsets.data_ptr<int>(), topo.column_indices.data_ptr<int>(), dtype,
                   q.t.data_ptr(), q.batch_stride, q.head_stride, q.row_stride, k.t.data_ptr(),
                   k.batch_stride, k.head_stride, k.row_stride, v.t.data_ptr(), v.batch_stride,
                   v.head_stride, v.row_stride, static_cast<float>(scale), o.t.data_ptr(),
                   static_cast<int>(out_type), o.batch_stride, o.head_stride, o.row_stride,
                   want_lse ? lse.data_ptr<float>() : nullptr, static_cast<int64_t>(m), tail...);
  };
  check_status(run_forward(args, sputnik_hip_sparse_attention_heads_forward,
                           sputnik_hip_sparse_attention_heads_forward_planned,
                           sputnik_hip_sparse_attention_heads_forward_dropout,
                           sputnik_hip_sparse_attention_heads_forward_planned_dropout, plan, ws_bytes, q.t,
                           drop),
               drop != nullptr ? "sparse_attention_heads_dropout" : "sparse_attention_heads");
  return attention_result(out, lse, want_lse, drop);
}

// y [batch, seq, out] = x W^T per batch element in ROW orientation (sputnik_hip.h:
// sparse_linear_half_rows_forward), x [batch, seq, in] half with a unit last stride; stored
// into `out` when given (any [batch, seq, out] view with a unit last stride, e.g. a column
// slice of a wider buffer) as out_type (0 float32, else x's type).  An EMPTY tensor says the
// route does not serve the call.
Tensor half_linear_rows(int64_t out64, const Tensor& image, int64_t values_type, const Tensor& x_in,
                        const c10::optional<Tensor>& out_in, int64_t out_type) {
  TORCH_CHECK(x_in.is_cuda() && x_in.dim() == 3, "half_linear_rows: x must be a GPU tensor [batch, seq, in]");
  const Tensor x = x_in.stride(2) == 1 ? x_in : x_in.contiguous();
  const int tile = tile_code_of(x);
  const c10::DeviceGuard guard(x.device());
  const int out_f = to_int(out64, "out"), batch = to_int(x.size(0), "batch"), seq = to_int(x.size(1), "seq"),
            in_f = to_int(x.size(2), "in");
  TORCH_CHECK(out_type == SPUTNIK_HIP_F32 || out_type == tile, "half_linear_rows: out_type is float32 or x's type");
  TORCH_CHECK(static_cast<size_t>(image.numel()) >=
                  sputnik_hip_sparse_linear_half_image_bytes(out_f, in_f, static_cast<int>(values_type), tile),
              "half_linear_rows: the image was made for another shape");
  const auto out_st = out_type == SPUTNIK_HIP_F32 ? at::kFloat : x.scalar_type();
  Tensor y;
  if (out_in.has_value()) {
    y = *out_in;
    TORCH_CHECK(y.dim() == 3 && y.size(0) == batch && y.size(1) == seq && y.size(2) == out_f && y.stride(2) == 1,
                "half_linear_rows: out must be a [batch, seq, out] view with a unit last stride");
    TORCH_CHECK(y.scalar_type() == out_st && y.device() == x.device(), "half_linear_rows: out has another type or device");
  } else {
    y = at::empty({batch, seq, out_f}, x.options().dtype(out_st));
  }
  const int st = sputnik_hip_sparse_linear_half_rows_forward(
      out_f, in_f, seq, batch, image.data_ptr(), static_cast<int>(values_type), x.data_ptr(), x.stride(0),
      x.stride(1), tile, y.data_ptr(), static_cast<int>(out_type), y.stride(0), y.stride(1), current_stream(x));
  if (st == SPUTNIK_HIP_UNSUPPORTED) return at::empty({0}, x.options().dtype(out_st));
  check_status(st, "half_linear_rows");
  return y;
}

// ---------------------------------------------------------------------------
// many-mask family (tests/transformer/functions.py, tests/transformer/utils.py:17-38):
// b topologies, concatenated; replica r uses mask r / (R / b).
// ---------------------------------------------------------------------------
struct ManyMask {
  int masks, m, replicas, width;  // width = max nonzeros
  std::vector<int> nonzeros;
  Tensor row_indices, row_offsets, column_indices;  // flat int32
  bool uniform;                                     // every mask has `width` nonzeros
};

Tensor as_flat_index(const Tensor& t, const char* name, const Tensor& like) {
  TORCH_CHECK(t.scalar_type() == at::kInt || t.scalar_type() == at::kLong, name,
              " must be an int32 (or int64) tensor, got ", t.scalar_type());
  TORCH_CHECK(t.device() == like.device(), name, " must be on ", like.device(), ", got ",
              t.device());
  return t.to(at::kInt).contiguous().view({-1});
}

// `nonzeros` is the tensor tests/transformer/utils.py:36 builds with
// torch.tensor(nnzs): it lives on the host.  A device tensor is accepted but
// costs a synchronising copy.
ManyMask check_many_mask(int64_t b, int64_t m, const Tensor& nonzeros,
                         const c10::optional<Tensor>& row_indices, const Tensor& row_offsets,
                         const Tensor& column_indices, const Tensor& like, int64_t replicas) {
  ManyMask mm;
  mm.masks = to_int(b, "b");
  mm.m = to_int(m, "m");
  mm.replicas = to_int(replicas, "replicas");
  TORCH_CHECK(mm.masks > 0, "b must be positive");
  TORCH_CHECK(mm.replicas % mm.masks == 0, "the number of replicas (", replicas,
              ") must be a multiple of the number of masks (", b, ")");
  TORCH_CHECK(nonzeros.numel() == mm.masks, "nonzeros should have b = ", b, " entries, got ",
              nonzeros.numel());
  TORCH_CHECK(at::isIntegralType(nonzeros.scalar_type(), false), "nonzeros must be integral");
  const Tensor host = nonzeros.to(at::kCPU, at::kLong).contiguous();
  int64_t total = 0;
  mm.width = 0;
  mm.uniform = true;
  for (int i = 0; i < mm.masks; ++i) {
    const int64_t v = host.data_ptr<int64_t>()[i];
    mm.nonzeros.push_back(to_int(v, "nonzeros[i]"));
    total += v;
    mm.width = std::max(mm.width, mm.nonzeros.back());
  }
  for (int v : mm.nonzeros) mm.uniform = mm.uniform && v == mm.width;
  mm.row_offsets = as_flat_index(row_offsets, "row_offsets", like);
  mm.column_indices = as_flat_index(column_indices, "column_indices", like);
  TORCH_CHECK(mm.row_offsets.numel() == static_cast<int64_t>(mm.masks) * (mm.m + 1),
              "row_offsets should have b * (m + 1) = ", static_cast<int64_t>(mm.masks) * (mm.m + 1),
              " entries, got ", mm.row_offsets.numel());
  TORCH_CHECK(mm.column_indices.numel() == total, "column_indices should have sum(nonzeros) = ",
              total, " entries, got ", mm.column_indices.numel());
  if (row_indices.has_value()) {
    mm.row_indices = as_flat_index(*row_indices, "row_indices", like);
    TORCH_CHECK(mm.row_indices.numel() == static_cast<int64_t>(mm.masks) * mm.m,
                "row_indices should have b * m = ", static_cast<int64_t>(mm.masks) * mm.m,
                " entries, got ", mm.row_indices.numel());
  }
  return mm;
}

Tensor many_mask_values(const Tensor& t, const ManyMask& mm, const char* name) {
  TORCH_CHECK(t.dim() == 2, name, " should be [replicas, max(nonzeros)], got ", t.sizes());
  TORCH_CHECK(t.size(0) == mm.replicas, name, ": expected ", mm.replicas, " replicas, got ",
              t.size(0));
  TORCH_CHECK(t.size(1) >= mm.width, name, ": rows must hold max(nonzeros) = ", mm.width,
              " entries, got ", t.size(1));
  return t;
}

Tensor spmm_many_mask(int64_t b, int64_t m64, int64_t k64, const Tensor& nonzeros,
                      const Tensor& values_in, const Tensor& row_indices,
                      const Tensor& row_offsets, const Tensor& column_indices,
                      const Tensor& dense_in) {
  const Tensor values = as_float(values_in, "values");
  const Tensor dense = as_float(dense_in, "dense");
  TORCH_CHECK(dense.dim() == 3, "dense should be [replicas, k, n], got ", dense.sizes());
  TORCH_CHECK(dense.device() == values.device(), "values and dense must be on one device");
  const c10::DeviceGuard guard(values.device());
  const ManyMask mm = check_many_mask(b, m64, nonzeros, row_indices, row_offsets, column_indices,
                                      values, dense.size(0));
  many_mask_values(values, mm, "values");
  const int k = to_int(k64, "k"), n = to_int(dense.size(2), "n");
  TORCH_CHECK(dense.size(1) == k, "inner matrix dimensions must match: dense has ",
              dense.size(1), " rows, k = ", k);
  Tensor out = at::empty({mm.replicas, mm.m, n}, values.options());
  const size_t ws_bytes = sputnik_hip_spmm_workspace_bytes(mm.m, k, n, mm.width);
  Tensor workspace;
  if (ws_bytes > 0)
    workspace = at::empty({static_cast<int64_t>(ws_bytes)}, values.options().dtype(at::kByte));
  check_status(sputnik_hip_spmm_many_mask(
                   mm.masks, mm.m, k, n, mm.nonzeros.data(), mm.replicas,
                   mm.row_indices.data_ptr<int>(), values.data_ptr<float>(), values.size(1),
                   mm.row_offsets.data_ptr<int>(), mm.column_indices.data_ptr<int>(),
                   dense.data_ptr<float>(), static_cast<int64_t>(k) * n, out.data_ptr<float>(),
                   static_cast<int64_t>(mm.m) * n, ws_bytes ? workspace.data_ptr() : nullptr,
                   ws_bytes, current_stream(values)),
               "spmm_many_mask");
  return out;
}

Tensor sddmm_many_mask(int64_t b, int64_t m64, int64_t n64, const Tensor& nonzeros,
                       const Tensor& row_indices, const Tensor& row_offsets,
                       const Tensor& column_indices, const Tensor& lhs_in, const Tensor& rhs_in) {
  const Tensor lhs = as_float(lhs_in, "lhs_matrix");
  const Tensor rhs = as_float(rhs_in, "rhs_matrix");
  TORCH_CHECK(lhs.dim() == 3 && rhs.dim() == 3, "expected 3-dim lhs_matrix and rhs_matrix");
  TORCH_CHECK(lhs.device() == rhs.device(), "lhs_matrix and rhs_matrix must be on one device");
  TORCH_CHECK(lhs.size(0) == rhs.size(0), "first dim of lhs_matrix and rhs_matrix must match");
  TORCH_CHECK(lhs.size(2) == rhs.size(2), "last dim of input matrices must match");
  const c10::DeviceGuard guard(lhs.device());
  const ManyMask mm = check_many_mask(b, m64, nonzeros, row_indices, row_offsets, column_indices,
                                      lhs, lhs.size(0));
  const int n = to_int(n64, "n"), k = to_int(lhs.size(2), "k");
  TORCH_CHECK(lhs.size(1) == mm.m, "lhs_matrix should have m = ", mm.m, " rows");
  TORCH_CHECK(rhs.size(1) == n, "rhs_matrix should have n = ", n, " rows");
  // Entries past a replica's own count stay zero.
  Tensor out = mm.uniform ? at::empty({mm.replicas, mm.width}, lhs.options())
                          : at::zeros({mm.replicas, mm.width}, lhs.options());
  // (one plan per mask: all masks run in one launch, csrc/many_mask.hip)
  const size_t ws_bytes = sputnik_hip_sddmm_many_mask_workspace_bytes(
      mm.masks, mm.m, k, n, mm.width);
  Tensor workspace;
  if (ws_bytes > 0)
    workspace = at::empty({static_cast<int64_t>(ws_bytes)}, lhs.options().dtype(at::kByte));
  check_status(sputnik_hip_sddmm_many_mask(
                   mm.masks, mm.m, k, n, mm.nonzeros.data(), mm.replicas,
                   mm.row_indices.data_ptr<int>(), mm.row_offsets.data_ptr<int>(),
                   mm.column_indices.data_ptr<int>(), lhs.data_ptr<float>(),
                   static_cast<int64_t>(mm.m) * k, rhs.data_ptr<float>(),
                   static_cast<int64_t>(n) * k, out.data_ptr<float>(), mm.width,
                   ws_bytes ? workspace.data_ptr() : nullptr, ws_bytes, current_stream(lhs)),
               "sddmm_many_mask");
  return out;
}

Tensor sparse_softmax_many_mask_scaled(int64_t b, int64_t m64, const Tensor& nonzeros,
                                       const Tensor& values_in, const Tensor& row_indices,
                                       const Tensor& row_offsets, const Tensor& column_indices,
                                       double scale) {
  const Tensor values = as_float(values_in, "values");
  const c10::DeviceGuard guard(values.device());
  TORCH_CHECK(values.dim() == 2, "values should be [replicas, max(nonzeros)]");
  const ManyMask mm = check_many_mask(b, m64, nonzeros, row_indices, row_offsets, column_indices,
                                      values, values.size(0));
  many_mask_values(values, mm, "values");
  Tensor out = mm.uniform && values.size(1) == mm.width ? at::empty_like(values)
                                                        : at::zeros_like(values);
  check_status(sputnik_hip_sparse_softmax_many_mask(
                   mm.masks, mm.m, mm.nonzeros.data(), mm.replicas, values.data_ptr<float>(),
                   values.size(1), mm.row_indices.data_ptr<int>(),
                   mm.row_offsets.data_ptr<int>(), mm.column_indices.data_ptr<int>(),
                   static_cast<float>(scale), out.data_ptr<float>(), out.size(1),
                   current_stream(values)),
               "sparse_softmax_many_mask");
  return out;
}

Tensor sparse_softmax_many_mask(int64_t b, int64_t m, const Tensor& nonzeros,
                                const Tensor& values, const Tensor& row_indices,
                                const Tensor& row_offsets, const Tensor& column_indices) {
  return sparse_softmax_many_mask_scaled(b, m, nonzeros, values, row_indices, row_offsets,
                                         column_indices, 1.0);
}

Tensor sparse_softmax_backward_many_mask(int64_t b, int64_t m64, const Tensor& nonzeros,
                                         const Tensor& softmax_out_in, const Tensor& grad_out_in,
                                         const Tensor& row_offsets, double scale) {
  const Tensor y = as_float(softmax_out_in, "softmax_out");
  const Tensor g = as_float(grad_out_in, "grad_out");
  TORCH_CHECK(y.dim() == 2 && y.sizes() == g.sizes(),
              "softmax_out and grad_out should be [replicas, max(nonzeros)] and match");
  const c10::DeviceGuard guard(y.device());
  const int masks = to_int(b, "b"), m = to_int(m64, "m");
  TORCH_CHECK(masks > 0 && y.size(0) % masks == 0, "replicas must be a multiple of b");
  TORCH_CHECK(nonzeros.numel() == masks, "nonzeros should have b entries");
  const Tensor host = nonzeros.to(at::kCPU, at::kLong).contiguous();
  std::vector<int> counts;
  bool full = true;
  for (int i = 0; i < masks; ++i) {
    counts.push_back(to_int(host.data_ptr<int64_t>()[i], "nonzeros[i]"));
    TORCH_CHECK(counts.back() <= y.size(1), "nonzeros[i] exceeds the row length of softmax_out");
    full = full && counts.back() == y.size(1);
  }
  const Tensor offsets = as_flat_index(row_offsets, "row_offsets", y);
  TORCH_CHECK(offsets.numel() == static_cast<int64_t>(masks) * (m + 1),
              "row_offsets should have b * (m + 1) entries");
  Tensor out = full ? at::empty_like(y) : at::zeros_like(y);
  check_status(sputnik_hip_sparse_softmax_backward_many_mask(
                   masks, m, counts.data(), to_int(y.size(0), "replicas"), y.data_ptr<float>(),
                   y.size(1), g.data_ptr<float>(), g.size(1), offsets.data_ptr<int>(),
                   static_cast<float>(scale), out.data_ptr<float>(), out.size(1),
                   current_stream(y)),
               "sparse_softmax_backward_many_mask");
  return out;
}

std::vector<Tensor> csr_transpose_many_mask(int64_t b, int64_t m64, int64_t n64,
                                            const Tensor& nonzeros, const Tensor& values_in,
                                            const Tensor& row_offsets,
                                            const Tensor& column_indices) {
  const Tensor values = as_float(values_in, "values");
  const c10::DeviceGuard guard(values.device());
  TORCH_CHECK(values.dim() == 2, "values should be [replicas, max(nonzeros)]");
  const ManyMask mm = check_many_mask(b, m64, nonzeros, c10::nullopt, row_offsets,
                                      column_indices, values, values.size(0));
  many_mask_values(values, mm, "values");
  const int n = to_int(n64, "n");
  const auto index_options = values.options().dtype(at::kInt);
  Tensor out_values = mm.uniform && values.size(1) == mm.width ? at::empty_like(values)
                                                               : at::zeros_like(values);
  // [b, n + 1]: tests/transformer/utils.py:51-62 (diffsort_many_mask) indexes it per mask
  Tensor out_row_offsets = at::empty({mm.masks, n + 1}, index_options);
  Tensor out_column_indices = at::empty({mm.column_indices.numel()}, index_options);
  const size_t ws_bytes = sputnik_hip_csr_transpose_many_mask_workspace_bytes(mm.masks, mm.m, n, mm.width);
  Tensor workspace =
      at::empty({static_cast<int64_t>(ws_bytes)}, values.options().dtype(at::kByte));
  check_status(sputnik_hip_csr_transpose_many_mask(
                   mm.masks, mm.m, n, mm.nonzeros.data(), mm.replicas, values.data_ptr<float>(),
                   values.size(1), mm.row_offsets.data_ptr<int>(),
                   mm.column_indices.data_ptr<int>(), out_values.data_ptr<float>(),
                   out_values.size(1), out_row_offsets.data_ptr<int>(),
                   out_column_indices.data_ptr<int>(), nullptr, workspace.data_ptr(), ws_bytes,
                   current_stream(values)),
               "csr_transpose_many_mask");
  return {out_values, out_row_offsets, out_column_indices};
}

// ---- CSR topologies built on the device (sputnik_hip.h: dense_to_csr_*, csr_row_order) ----

// row_offsets [m + 1] or [b, m + 1] -> row_indices [m] / [b, m]: the rows of every mask by
// ascending length, ties by row (topology.diffsort).  One launch on the current stream, no
// synchronisation, torch allocations only: capturable.
Tensor row_order(const Tensor& row_offsets_in) {
  TORCH_CHECK(row_offsets_in.is_cuda(), "row_offsets must be a GPU (HIP) tensor, got ",
              row_offsets_in.device());
  TORCH_CHECK(row_offsets_in.scalar_type() == at::kInt, "row_offsets must be int32, got ",
              row_offsets_in.scalar_type());
  TORCH_CHECK((row_offsets_in.dim() == 1 || row_offsets_in.dim() == 2) && row_offsets_in.size(-1) >= 1,
              "row_offsets should be [m + 1] or [b, m + 1], got ", row_offsets_in.sizes());
  const c10::DeviceGuard guard(row_offsets_in.device());
  const Tensor row_offsets = row_offsets_in.contiguous();
  const int masks = row_offsets.dim() == 2 ? to_int(row_offsets.size(0), "b") : 1;
  const int m = to_int(row_offsets.size(-1) - 1, "m");
  int served = 0;
  check_status(sputnik_hip_csr_row_order_route(masks, m, 0, &served, nullptr, nullptr, nullptr), "row_order");
  check_served("row_order", served, "sputnik_hip_csr_row_order_route", "torch.argsort");
  Tensor row_indices = row_offsets.dim() == 2 ? at::empty({masks, m}, row_offsets.options())
                                              : at::empty({m}, row_offsets.options());
  check_status(sputnik_hip_csr_row_order(masks, m, 0, row_offsets.data_ptr<int>(),
                                         row_indices.data_ptr<int>(), current_stream(row_offsets)),
               "row_order");
  return row_indices;
}

// dense [m, n], [b, m, n] or [b, 1, m, n] -> [row_indices, row_offsets, column_indices,
// nonzeros (int64, host)] (+ values, 2-D only): topology.dense_to_sparse / dense_to_sparse_3d.
// Count and row order are launched, the b counts are read back -- the ONE synchronisation: the
// operators take `nonzeros` on the host, and column_indices is allocated at its exact size --
// and the fill is launched.  Views with a dense last dimension are read in place.
std::vector<Tensor> dense_to_csr(const Tensor& dense_in, bool with_values) {
  TORCH_CHECK(dense_in.is_cuda(), "dense must be a GPU (HIP) tensor, got ", dense_in.device());
  TORCH_CHECK(dense_in.dim() >= 2 && dense_in.dim() <= 4,
              "expected a [m, n], [b, m, n] or [b, 1, m, n] tensor, got ", dense_in.sizes());
  TORCH_CHECK(dense_in.dim() != 4 || dense_in.size(1) == 1,
              "expected a [b, 1, m, n] tensor, got ", dense_in.sizes());
  TORCH_CHECK(!with_values || dense_in.dim() == 2, "values are returned for 2-D inputs only");
  const auto type = dense_in.scalar_type();
  TORCH_CHECK(!c10::isComplexType(type) && !c10::isQIntType(type), "unsupported element type ", type);
  const c10::DeviceGuard guard(dense_in.device());
  const auto [dense, row_stride] = rows_in_place(dense_in.dim() == 4 ? dense_in.select(1, 0) : dense_in);
  const bool batched = dense.dim() == 3;
  const int masks = batched ? to_int(dense.size(0), "b") : 1;
  const int m = to_int(dense.size(-2), "m"), n = to_int(dense.size(-1), "n");
  const int64_t batch_stride = batched && masks > 1 ? dense.stride(0) : 0;
  const int element_bytes = static_cast<int>(dense.element_size());
  const int floating = c10::isFloatingType(type) ? 1 : 0;
  const auto index_options = dense.options().dtype(at::kInt);
  Tensor row_offsets = batched ? at::empty({masks, m + 1}, index_options) : at::empty({m + 1}, index_options);
  Tensor counts = at::empty({masks}, index_options);
  Tensor bases = at::empty({masks}, dense.options().dtype(at::kLong));
  const auto stream = current_stream(dense);
  check_status(sputnik_hip_dense_to_csr_count(masks, m, n, dense.data_ptr(), element_bytes, floating,
                                              batch_stride, row_stride, row_offsets.data_ptr<int>(),
                                              counts.data_ptr<int>(), bases.data_ptr<int64_t>(), stream),
               "dense_to_csr (count)");
  Tensor row_indices = row_order(row_offsets);
  Tensor nonzeros = counts.to(at::kCPU).to(at::kLong);   // the synchronisation
  const int64_t total = nonzeros.sum().item<int64_t>();
  Tensor column_indices = at::empty({total}, index_options);
  Tensor values;
  if (with_values) values = at::empty({total}, dense.options());
  if (total > 0)
    check_status(sputnik_hip_dense_to_csr_fill(masks, m, n, dense.data_ptr(), element_bytes, floating,
                                               batch_stride, row_stride, row_offsets.data_ptr<int>(),
                                               bases.data_ptr<int64_t>(), column_indices.data_ptr<int>(),
                                               with_values ? values.data_ptr() : nullptr, stream),
                 "dense_to_csr (fill)");
  std::vector<Tensor> out{row_indices, row_offsets, column_indices, nonzeros};
  if (with_values) out.push_back(values);
  return out;
}

// scores [m, n] (float32 / float16 / bfloat16) -> [row_indices, row_offsets, column_indices,
// values]: the CSR topology of the `per_row` largest |scores| of every row, or of the `total`
// largest of the matrix (the other one -1), with the elements of `values_from` (same shape, any
// 2- or 4-byte dtype; the scores themselves by default) at the kept positions.  Every size is
// known up front: no synchronisation.  The workspace is this call's own allocation, on the
// stream's allocator, so no other call can be writing its histograms.
std::vector<Tensor> topk_to_csr(const Tensor& scores_in, int64_t per_row, int64_t total,
                                const c10::optional<Tensor>& values_from_in) {
  const char* op = "topk_to_csr";
  const auto [scores, score_stride] = check_scores(op, scores_in);
  const auto [total_mode, count] = parse_selection(op, per_row, total);
  const c10::DeviceGuard guard(scores.device());
  const int m = to_int(scores.size(0), "m"), n = to_int(scores.size(1), "n");
  const int element_bytes = static_cast<int>(scores.element_size());
  int served = 0;
  check_status(sputnik_hip_topk_to_csr_launch_shape(m, n, element_bytes, total_mode, &served, nullptr, nullptr,
                                                    nullptr, nullptr, nullptr),
               op);
  check_served(op, served, "sputnik_hip_topk_to_csr_launch_shape", "topology.magnitude_prune");
  check_count(op, total_mode ? "total" : "per_row", count, total_mode ? static_cast<int64_t>(m) * n : n);
  const Tensor& from = values_from_in.has_value() ? *values_from_in : scores;
  TORCH_CHECK(from.is_cuda() && from.device() == scores.device() && from.sizes() == scores.sizes(),
              "torch_sputnik::topk_to_csr: values_from must be a tensor of the scores' shape on their device, got ",
              from.sizes(), " on ", from.device());
  TORCH_CHECK(from.element_size() == 2 || from.element_size() == 4,
              "torch_sputnik::topk_to_csr: values_from must have 2- or 4-byte elements, got ", from.scalar_type());
  const auto [values_from, from_stride] = rows_in_place(from);
  const int64_t nonzeros = total_mode ? count : count * m;
  const auto index_options = scores.options().dtype(at::kInt);
  Tensor row_indices = at::empty({m}, index_options);
  Tensor row_offsets = at::empty({m + 1}, index_options);
  Tensor column_indices = at::empty({nonzeros}, index_options);
  Tensor values = at::empty({nonzeros}, values_from.options());
  const size_t ws_bytes = sputnik_hip_topk_to_csr_workspace_bytes(m, n, total_mode);
  Tensor workspace = workspace_like(scores, ws_bytes);
  check_status(sputnik_hip_topk_to_csr(
                   m, n, scores.data_ptr(), element_bytes, score_stride, total_mode, count, values_from.data_ptr(),
                   static_cast<int>(values_from.element_size()), from_stride, workspace.data_ptr(), ws_bytes,
                   row_indices.data_ptr<int>(), row_offsets.data_ptr<int>(), column_indices.data_ptr<int>(),
                   values.data_ptr(), current_stream(scores)),
               op);
  return {row_indices, row_offsets, column_indices, values};
}

// A uniformly random m x n CSR topology with its initial values, drawn on `device`
// (sputnik_hip.h: sputnik_hip_random_csr) -> [row_indices, row_offsets, column_indices, values,
// rng_state]: `per_row` positions of every row or `total` of the matrix (the other one -1),
// values of `dtype` uniform on [-2^23 scale, 2^23 scale).  The state comes from the device's
// default generator as attention dropout's does (draw_state), or replays `rng_state`; the
// returned rng_state holds what the kernels resolved.  Every size is known up front: no
// synchronisation, and a captured call draws a new pattern on every replay.
std::vector<Tensor> random_csr(int64_t m_in, int64_t n_in, int64_t per_row, int64_t total, at::ScalarType dtype,
                               double scale, c10::Device device, const c10::optional<Tensor>& rng_state,
                               int64_t key_mask) {
  const char* op = "random_csr";
  TORCH_CHECK(device.is_cuda(), "torch_sputnik::random_csr: device must be a GPU (HIP) device, got ", device);
  TORCH_CHECK(type_code(dtype) >= 0, "torch_sputnik::random_csr: dtype must be float32, float16 or bfloat16, got ",
              dtype);
  const auto [total_mode, count] = parse_selection(op, per_row, total);
  check_count(op, "key_mask", key_mask, 0x7fffffff);
  const c10::DeviceGuard guard(device);
  if (!device.has_index()) device = c10::Device(device.type(), at::cuda::current_device());
  const int m = to_int(m_in, "m"), n = to_int(n_in, "n");
  int served = 0;
  check_status(sputnik_hip_random_csr_launch_shape(m, n, total_mode, &served, nullptr, nullptr, nullptr, nullptr,
                                                   nullptr, nullptr),
               op);
  check_served(op, served, "sputnik_hip_random_csr_launch_shape", "topology.random_csr");
  check_count(op, total_mode ? "total" : "per_row", count, total_mode ? static_cast<int64_t>(m) * n : n);
  const int64_t nonzeros = total_mode ? count : count * m;
  const auto index_options = at::TensorOptions().device(device).dtype(at::kInt);
  Tensor row_indices = at::empty({m}, index_options);
  Tensor row_offsets = at::empty({m + 1}, index_options);
  Tensor column_indices = at::empty({nonzeros}, index_options);
  Tensor values = at::empty({nonzeros}, index_options.dtype(dtype));
  const Drop state = draw_state(rng_state, row_offsets);
  const size_t ws_bytes = sputnik_hip_random_csr_workspace_bytes(m, n, total_mode);
  Tensor workspace = workspace_like(row_offsets, ws_bytes);
  check_status(sputnik_hip_random_csr(m, n, total_mode, count, type_code(dtype), static_cast<float>(scale),
                                      static_cast<unsigned>(key_mask), state.rng, state.rng_state_out,
                                      workspace.data_ptr(), ws_bytes, row_indices.data_ptr<int>(),
                                      row_offsets.data_ptr<int>(), column_indices.data_ptr<int>(),
                                      values.data_ptr(), current_stream(row_offsets)),
               op);
  return {row_indices, row_offsets, column_indices, values, state.rng_state};
}

// The CSR topology of an attention pattern over m rows and n columns, built on `device` from
// its rule (sputnik_hip.h, "Attention patterns"; ops.attention_pattern_csr checks and clamps
// the fields) -> [row_indices, row_offsets, column_indices] (+ rng_state with random blocks).
// Count and scan are launched, the one count is read back -- the ONE synchronisation -- and
// the fill and the row order are launched.  `global_flags`: uint8 [n] on the device, or none.
// Only a rule with random blocks has a Philox state: a replay of `rng_state`, or 4 drawn from
// the device's default generator (draw_state).
std::vector<Tensor> attention_pattern_csr(int64_t m_in, int64_t n_in, int64_t offset, int64_t window_left,
                                          int64_t window_right, int64_t dilation, int64_t block,
                                          int64_t summary_stride, int64_t summary_first, int64_t random_block,
                                          int64_t random_threshold, bool causal, bool global_rows,
                                          const c10::optional<Tensor>& global_flags_in, c10::Device device,
                                          const c10::optional<Tensor>& rng_state) {
  const char* op = "attention_pattern_csr";
  TORCH_CHECK(device.is_cuda(), "torch_sputnik::attention_pattern_csr: device must be a GPU (HIP) device, got ",
              device);
  const c10::DeviceGuard guard(device);
  if (!device.has_index()) device = c10::Device(device.type(), at::cuda::current_device());
  const int m = to_int(m_in, "m"), n = to_int(n_in, "n");
  int served = 0;
  check_status(sputnik_hip_attention_pattern_launch_shape(m, n, offset, &served, nullptr, nullptr, nullptr, nullptr,
                                                          nullptr),
               op);
  check_served(op, served, "sputnik_hip_attention_pattern_launch_shape", "topology.AttentionPattern.build");
  sputnik_hip_attention_pattern_args rule{};
  rule.offset = offset;
  rule.window_left = window_left;
  rule.window_right = window_right;
  rule.dilation = dilation;
  rule.block = to_int(block, "block");
  rule.summary_stride = to_int(summary_stride, "summary_stride");
  rule.summary_first = to_int(summary_first, "summary_first");
  rule.random_block = to_int(random_block, "random_block");
  check_count(op, "random_threshold", random_threshold, int64_t{1} << 31);
  rule.random_threshold = static_cast<unsigned>(random_threshold);
  rule.causal = causal ? 1 : 0;
  rule.global_rows = global_rows ? 1 : 0;
  Tensor global_flags;
  if (global_flags_in.has_value() && global_flags_in->defined()) {
    TORCH_CHECK(global_flags_in->device() == device && global_flags_in->scalar_type() == at::kByte &&
                    global_flags_in->dim() == 1 && global_flags_in->numel() == n,
                "torch_sputnik::attention_pattern_csr: global_flags must be a uint8 [n] tensor on ", device, ", got ",
                global_flags_in->scalar_type(), " ", global_flags_in->sizes(), " on ", global_flags_in->device());
    global_flags = global_flags_in->contiguous();
    if (reinterpret_cast<uintptr_t>(global_flags.data_ptr()) % 4 != 0) global_flags = global_flags.clone();
    rule.global_flags = static_cast<const unsigned char*>(global_flags.data_ptr());
  }
  const auto index_options = at::TensorOptions().device(device).dtype(at::kInt);
  Tensor row_indices = at::empty({m}, index_options);
  Tensor row_offsets = at::empty({m + 1}, index_options);
  Tensor count = at::empty({1}, index_options);
  const bool random = random_block > 0;
  const Drop state = random ? draw_state(rng_state, row_offsets) : Drop();
  const auto stream = current_stream(row_offsets);
  check_status(sputnik_hip_attention_pattern_count(m, n, &rule, state.rng, state.rng_state_out,
                                                   row_offsets.data_ptr<int>(), count.data_ptr<int>(), stream),
               "attention_pattern_csr (count)");
  const int nonzeros = count.to(at::kCPU).item<int>();   // the synchronisation
  Tensor column_indices = at::empty({nonzeros}, index_options);
  check_status(sputnik_hip_attention_pattern_fill(m, n, &rule, state.rng, nonzeros, row_offsets.data_ptr<int>(),
                                                  row_indices.data_ptr<int>(), column_indices.data_ptr<int>(), stream),
               "attention_pattern_csr (fill)");
  std::vector<Tensor> out{row_indices, row_offsets, column_indices};
  if (random) out.push_back(state.rng_state);
  return out;
}

// One per-row drop-and-grow step of the CSR pattern (row_offsets [m + 1], column_indices [nnz])
// with `values` [nnz] under dense `scores` [m, n] -> [column_indices, values, source (int64)] of
// the new pattern in the same slots (sputnik_hip.h: sputnik_hip_csr_regrow).  nnz is known up
// front: one launch, no synchronisation, torch allocations only.  Scores with a dense last
// dimension are read in place.
std::vector<Tensor> csr_regrow(const Tensor& values_in, const Tensor& row_offsets_in,
                               const Tensor& column_indices_in, const Tensor& drop_counts_in,
                               const Tensor& scores_in) {
  const char* op = "csr_regrow";
  const CsrValues csr = check_csr_values(op, values_in, row_offsets_in, column_indices_in);
  const auto [scores, score_stride] = check_scores(op, scores_in, &csr);
  check_index(op, "drop_counts", drop_counts_in, csr.values);
  TORCH_CHECK(drop_counts_in.numel() == csr.m, "torch_sputnik::csr_regrow: drop_counts should be [m] for [m, n] scores ",
              scores.sizes(), ", got ", drop_counts_in.sizes());
  const c10::DeviceGuard guard(csr.values.device());
  const Tensor drop_counts = drop_counts_in.contiguous();
  const int m = csr.m, n = to_int(scores.size(1), "n"), nonzeros = csr.nonzeros;
  const int score_bytes = static_cast<int>(scores.element_size());
  int served = 0;
  check_status(sputnik_hip_csr_regrow_launch_shape(m, n, score_bytes, csr.value_bytes, &served, nullptr, nullptr,
                                                   nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
               op);
  check_served(op, served, "sputnik_hip_csr_regrow_launch_shape", "topology.regrow_per_row");
  Tensor out_columns = at::empty_like(csr.column_indices);
  Tensor out_values = at::empty_like(csr.values);
  Tensor source = at::empty({static_cast<int64_t>(nonzeros)}, csr.column_indices.options().dtype(at::kLong));
  const size_t ws_bytes = sputnik_hip_csr_regrow_workspace_bytes(m, n, nonzeros);
  Tensor workspace = workspace_like(scores, ws_bytes);
  check_status(sputnik_hip_csr_regrow(
                   m, n, nonzeros, csr.row_offsets.data_ptr<int>(), csr.column_indices.data_ptr<int>(),
                   csr.values.data_ptr(), csr.value_bytes, drop_counts.data_ptr<int>(), scores.data_ptr(), score_bytes,
                   score_stride, key_limit(scores.scalar_type()), ws_bytes ? workspace.data_ptr() : nullptr, ws_bytes,
                   out_columns.data_ptr<int>(), out_values.data_ptr(), source.data_ptr<int64_t>(),
                   current_stream(csr.values)),
               op);
  return {out_columns, out_values, source};
}

// One matrix-wide drop-and-grow step of the CSR pattern (row_offsets [m + 1], column_indices
// [nnz]) with `values` [nnz] under dense `scores` [m, n]: `drop` entries go, as many come ->
// [row_indices, row_offsets, column_indices, values, source (int64)] of the new pattern
// (sputnik_hip.h: sputnik_hip_csr_regrow_total).  nnz does not change, so every size is known up
// front: no synchronisation, torch allocations only; the workspace is this call's own allocation
// on the stream's allocator.  Scores with a dense last dimension are read in place.
std::vector<Tensor> csr_regrow_total(const Tensor& values_in, const Tensor& row_offsets_in,
                                     const Tensor& column_indices_in, int64_t drop, const Tensor& scores_in) {
  const char* op = "csr_regrow_total";
  const CsrValues csr = check_csr_values(op, values_in, row_offsets_in, column_indices_in);
  const auto [scores, score_stride] = check_scores(op, scores_in, &csr);
  check_count(op, "drop", drop, csr.nonzeros);
  const c10::DeviceGuard guard(csr.values.device());
  const int m = csr.m, n = to_int(scores.size(1), "n"), nonzeros = csr.nonzeros;
  const int score_bytes = static_cast<int>(scores.element_size());
  int served = 0;
  check_status(sputnik_hip_csr_regrow_total_launch_shape(
                   m, n, nonzeros, score_bytes, csr.value_bytes, &served, nullptr, nullptr, nullptr, nullptr, nullptr,
                   nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
               op);
  check_served(op, served, "sputnik_hip_csr_regrow_total_launch_shape", "topology.regrow_total");
  const auto index_options = csr.row_offsets.options();
  Tensor out_row_indices = at::empty({m}, index_options);
  Tensor out_row_offsets = at::empty({m + 1}, index_options);
  Tensor out_columns = at::empty({nonzeros}, index_options);
  Tensor out_values = at::empty_like(csr.values);
  Tensor source = at::empty({nonzeros}, index_options.dtype(at::kLong));
  const size_t ws_bytes = sputnik_hip_csr_regrow_total_workspace_bytes(m, n, nonzeros);
  Tensor workspace = workspace_like(csr.values, ws_bytes);
  check_status(sputnik_hip_csr_regrow_total(
                   m, n, nonzeros, csr.row_offsets.data_ptr<int>(), csr.column_indices.data_ptr<int>(),
                   csr.values.data_ptr(), csr.value_bytes, drop, scores.data_ptr(), score_bytes, score_stride,
                   key_limit(scores.scalar_type()), workspace.data_ptr(), ws_bytes, out_row_indices.data_ptr<int>(),
                   out_row_offsets.data_ptr<int>(), out_columns.data_ptr<int>(), out_values.data_ptr(),
                   source.data_ptr<int64_t>(), current_stream(csr.values)),
               op);
  return {out_row_indices, out_row_offsets, out_columns, out_values, source};
}

// The arguments the two steps under generated scores share (sputnik_hip.h:
// sputnik_hip_csr_regrow_random): the width of the matrix, the mask and the scale of a grown
// value (negative: grown entries are +0.0).
struct KeyStep {
  int n;
  unsigned key_mask;
  int grow_values;
  float grow_scale;
};
KeyStep check_key_step(const char* op, int64_t n, int64_t key_mask, double grow_scale) {
  check_count(op, "key_mask", key_mask, 0x3fffffff);
  TORCH_CHECK(!(grow_scale >= 0.0) || grow_scale < std::numeric_limits<float>::infinity(), "torch_sputnik::", op,
              ": grow_scale must be finite, got ", grow_scale);
  const bool grow = grow_scale >= 0.0;
  return {to_int(n, "n"), static_cast<unsigned>(key_mask), grow ? 1 : 0, grow ? static_cast<float>(grow_scale) : 0.f};
}

// One per-row drop-and-grow step of the CSR pattern of an m x n matrix under random scores that
// are never stored (sputnik_hip.h: sputnik_hip_csr_regrow_random) -> [column_indices, values,
// source (int64), rng_state].  The state comes from the device's default generator (draw_state)
// or replays `rng_state`; grow_scale < 0: grown entries are +0.0, else the value stream under
// that scale.  One launch, no synchronisation, torch allocations only.
std::vector<Tensor> csr_regrow_random(const Tensor& values_in, const Tensor& row_offsets_in,
                                      const Tensor& column_indices_in, const Tensor& drop_counts_in, int64_t n_in,
                                      double grow_scale, const c10::optional<Tensor>& rng_state, int64_t key_mask) {
  const char* op = "csr_regrow_random";
  const CsrValues csr = check_csr_values(op, values_in, row_offsets_in, column_indices_in);
  const KeyStep step = check_key_step(op, n_in, key_mask, grow_scale);
  check_index(op, "drop_counts", drop_counts_in, csr.values);
  TORCH_CHECK(drop_counts_in.numel() == csr.m, "torch_sputnik::csr_regrow_random: drop_counts should be [", csr.m,
              "], got ", drop_counts_in.sizes());
  const c10::DeviceGuard guard(csr.values.device());
  const Tensor drop_counts = drop_counts_in.contiguous();
  const int m = csr.m, n = step.n, nonzeros = csr.nonzeros;
  int served = 0;
  check_status(sputnik_hip_csr_regrow_random_launch_shape(m, n, nonzeros, csr.value_bytes, 0, &served, nullptr,
                                                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                          nullptr, nullptr, nullptr),
               op);
  check_served(op, served, "sputnik_hip_csr_regrow_random_launch_shape", "topology.regrow_per_row_random");
  Tensor out_columns = at::empty_like(csr.column_indices);
  Tensor out_values = at::empty_like(csr.values);
  Tensor source = at::empty({static_cast<int64_t>(nonzeros)}, csr.column_indices.options().dtype(at::kLong));
  const Drop state = draw_state(rng_state, csr.row_offsets);
  check_status(sputnik_hip_csr_regrow_random(
                   m, n, nonzeros, csr.row_offsets.data_ptr<int>(), csr.column_indices.data_ptr<int>(),
                   csr.values.data_ptr(), type_code(csr.values.scalar_type()), drop_counts.data_ptr<int>(), state.rng,
                   state.rng_state_out, step.key_mask, step.grow_values, step.grow_scale, nullptr, 0,
                   out_columns.data_ptr<int>(), out_values.data_ptr(), source.data_ptr<int64_t>(),
                   current_stream(csr.values)),
               op);
  return {out_columns, out_values, source, state.rng_state};
}

// One matrix-wide drop-and-grow step under random scores that are never stored (sputnik_hip.h:
// sputnik_hip_csr_regrow_total_random) -> [row_indices, row_offsets, column_indices, values,
// source (int64), rng_state].  No synchronisation, torch allocations only; the workspace is this
// call's own allocation on the stream's allocator.
std::vector<Tensor> csr_regrow_total_random(const Tensor& values_in, const Tensor& row_offsets_in,
                                            const Tensor& column_indices_in, int64_t drop, int64_t n_in,
                                            double grow_scale, const c10::optional<Tensor>& rng_state,
                                            int64_t key_mask) {
  const char* op = "csr_regrow_total_random";
  const CsrValues csr = check_csr_values(op, values_in, row_offsets_in, column_indices_in);
  const KeyStep step = check_key_step(op, n_in, key_mask, grow_scale);
  check_count(op, "drop", drop, csr.nonzeros);
  const c10::DeviceGuard guard(csr.values.device());
  const int m = csr.m, n = step.n, nonzeros = csr.nonzeros;
  int served = 0;
  check_status(sputnik_hip_csr_regrow_random_launch_shape(m, n, nonzeros, csr.value_bytes, 1, &served, nullptr,
                                                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                          nullptr, nullptr, nullptr),
               op);
  check_served(op, served, "sputnik_hip_csr_regrow_random_launch_shape", "topology.regrow_total_random");
  const auto index_options = csr.row_offsets.options();
  Tensor out_row_indices = at::empty({m}, index_options);
  Tensor out_row_offsets = at::empty({m + 1}, index_options);
  Tensor out_columns = at::empty({nonzeros}, index_options);
  Tensor out_values = at::empty_like(csr.values);
  Tensor source = at::empty({nonzeros}, index_options.dtype(at::kLong));
  const Drop state = draw_state(rng_state, csr.row_offsets);
  const size_t ws_bytes = sputnik_hip_csr_regrow_random_workspace_bytes(m, n, nonzeros, 1);
  Tensor workspace = workspace_like(csr.values, ws_bytes);
  check_status(sputnik_hip_csr_regrow_total_random(
                   m, n, nonzeros, csr.row_offsets.data_ptr<int>(), csr.column_indices.data_ptr<int>(),
                   csr.values.data_ptr(), type_code(csr.values.scalar_type()), drop, state.rng, state.rng_state_out,
                   step.key_mask, step.grow_values, step.grow_scale, workspace.data_ptr(), ws_bytes,
                   out_row_indices.data_ptr<int>(), out_row_offsets.data_ptr<int>(), out_columns.data_ptr<int>(),
                   out_values.data_ptr(), source.data_ptr<int64_t>(), current_stream(csr.values)),
               op);
  return {out_row_indices, out_row_offsets, out_columns, out_values, source, state.rng_state};
}

// The CSR pattern (row_offsets [m + 1], column_indices [nnz]) with `values` [nnz] -> [row_indices,
// row_offsets, column_indices, values, source (int64)] of its `total` entries of largest |value|,
// or of the `per_row` largest of every row (the other one -1): sputnik_hip.h:
// sputnik_hip_csr_topk.  Total mode knows its size up front: no synchronisation, torch
// allocations only.  Per-row mode reads the new size out_row_offsets[m] back once -- the ONE
// synchronisation, as in dense_to_csr -- between the offsets half and the fill half of the call.
// The op does not know the matrix width: any per_row >= 0 is taken (a row keeps
// min(len_r, per_row)).
std::vector<Tensor> csr_topk(const Tensor& values_in, const Tensor& row_offsets_in,
                             const Tensor& column_indices_in, int64_t per_row, int64_t total) {
  const char* op = "csr_topk";
  const CsrValues csr = check_csr_values(op, values_in, row_offsets_in, column_indices_in);
  const Selection mode = parse_selection(op, per_row, total);
  const c10::DeviceGuard guard(csr.values.device());
  const int m = csr.m, nonzeros = csr.nonzeros, total_mode = mode.total_mode;
  const int n = std::numeric_limits<int>::max();   // (not known here: bounds per_row alone)
  const int64_t count = total_mode ? mode.count : std::min<int64_t>(mode.count, n);
  int served = 0;
  check_status(sputnik_hip_csr_topk_launch_shape(m, n, nonzeros, csr.value_bytes, total_mode, &served, nullptr,
                                                 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
               op);
  check_served(op, served, "sputnik_hip_csr_topk_launch_shape", "topology.prune_csr");
  if (total_mode) check_count(op, "total", count, nonzeros);
  const auto index_options = csr.row_offsets.options();
  Tensor out_row_indices = at::empty({m}, index_options);
  Tensor out_row_offsets = at::empty({m + 1}, index_options);
  const size_t ws_bytes = sputnik_hip_csr_topk_workspace_bytes(m, n, nonzeros, total_mode);
  Tensor workspace = workspace_like(csr.values, ws_bytes);
  const auto stream = current_stream(csr.values);
  const int* offsets_in = csr.row_offsets.data_ptr<int>();
  int64_t kept = count;
  if (!total_mode) {
    check_status(sputnik_hip_csr_topk(m, n, nonzeros, offsets_in, nullptr, nullptr, csr.value_bytes, 0, count, nullptr,
                                      0, out_row_indices.data_ptr<int>(), out_row_offsets.data_ptr<int>(), nullptr,
                                      nullptr, nullptr, 0, stream),
                 "csr_topk (offsets)");
    kept = out_row_offsets[m].item<int>();   // the synchronisation
    TORCH_CHECK(kept >= 0 && kept <= nonzeros, "torch_sputnik::csr_topk: row_offsets do not ascend inside 0 .. ",
                nonzeros);
  }
  Tensor out_columns = at::empty({kept}, index_options);
  Tensor out_values = at::empty({kept}, csr.values.options());
  Tensor source = at::empty({kept}, index_options.dtype(at::kLong));
  if (total_mode || kept > 0)
    check_status(sputnik_hip_csr_topk(
                     m, n, nonzeros, offsets_in, csr.column_indices.data_ptr<int>(), csr.values.data_ptr(),
                     csr.value_bytes, total_mode, count, ws_bytes ? workspace.data_ptr() : nullptr, ws_bytes,
                     total_mode ? out_row_indices.data_ptr<int>() : nullptr, out_row_offsets.data_ptr<int>(),
                     out_columns.data_ptr<int>(), out_values.data_ptr(), source.data_ptr<int64_t>(), kept, stream),
                 op);
  return {out_row_indices, out_row_offsets, out_columns, out_values, source};
}

// Several CSR patterns (lists of equal length: values[l] [nnz_l], row_offsets[l] [m_l + 1],
// column_indices[l] [nnz_l]) -> for every layer, one after the other, [row_indices, row_offsets,
// column_indices, values, source (int64)] of what it keeps when the `total` entries of largest
// |value| over ALL layers stay: sputnik_hip.h: sputnik_hip_csr_topk_global_*.  The layers' new
// sizes are read back once -- the ONE synchronisation, whatever the number of layers --
// between the select half and the fill half.
std::vector<Tensor> csr_topk_global(at::TensorList values_in, at::TensorList row_offsets_in,
                                    at::TensorList column_indices_in, int64_t total) {
  const char* op = "csr_topk_global";
  const size_t count_layers = values_in.size();
  TORCH_CHECK(row_offsets_in.size() == count_layers && column_indices_in.size() == count_layers,
              "torch_sputnik::csr_topk_global: ", count_layers, " values, ", row_offsets_in.size(),
              " row_offsets and ", column_indices_in.size(), " column_indices");
  if (count_layers == 0) {
    check_count(op, "total", total, 0);
    return {};
  }
  const int layers = to_int(static_cast<int64_t>(count_layers), "layers");
  std::vector<CsrValues> csr;
  std::vector<int> rows(layers), nonzeros(layers);
  int64_t entries = 0;
  for (int l = 0; l < layers; ++l) {
    csr.push_back(check_csr_values(op, values_in[l], row_offsets_in[l], column_indices_in[l]));
    TORCH_CHECK(csr[l].values.device() == csr[0].values.device() &&
                    csr[l].values.scalar_type() == csr[0].values.scalar_type(),
                "torch_sputnik::csr_topk_global: values must be on one device and of one dtype, got ",
                csr[0].values.scalar_type(), " on ", csr[0].values.device(), " and ", csr[l].values.scalar_type(),
                " on ", csr[l].values.device(), " in layer ", l);
    rows[l] = csr[l].m;
    nonzeros[l] = csr[l].nonzeros;
    entries += nonzeros[l];
  }
  const Tensor& like = csr[0].values;
  const c10::DeviceGuard guard(like.device());
  const int value_bytes = csr[0].value_bytes;
  int served = 0;
  check_status(sputnik_hip_csr_topk_global_launch_shape(layers, rows.data(), nonzeros.data(), value_bytes, &served,
                                                        nullptr, nullptr, nullptr, nullptr),
               op);
  check_served(op, served, "sputnik_hip_csr_topk_global_launch_shape", "topology.prune_csr_global");
  check_count(op, "total", total, entries);
  const auto index_options = csr[0].row_offsets.options();
  std::vector<Tensor> out_row_indices, out_row_offsets;
  std::vector<const int*> offsets_in(layers), columns_in(layers);
  std::vector<const void*> values_ptr(layers);
  std::vector<int*> order_out(layers), offsets_out(layers);
  for (int l = 0; l < layers; ++l) {
    out_row_offsets.push_back(at::empty({rows[l] + 1}, index_options));
    out_row_indices.push_back(at::empty({rows[l]}, index_options));
    offsets_in[l] = csr[l].row_offsets.data_ptr<int>();
    columns_in[l] = csr[l].column_indices.data_ptr<int>();
    values_ptr[l] = csr[l].values.data_ptr();
    offsets_out[l] = out_row_offsets[l].data_ptr<int>();
    order_out[l] = out_row_indices[l].data_ptr<int>();
  }
  const size_t ws_bytes = sputnik_hip_csr_topk_global_workspace_bytes(layers, rows.data());
  Tensor workspace = workspace_like(like, ws_bytes);
  Tensor sizes = at::empty({layers}, index_options);
  const auto stream = current_stream(like);
  check_status(sputnik_hip_csr_topk_global_select(layers, rows.data(), nonzeros.data(), offsets_in.data(),
                                                  values_ptr.data(), value_bytes, total, workspace.data_ptr(),
                                                  ws_bytes, offsets_out.data(), sizes.data_ptr<int>(), stream),
               "csr_topk_global (select)");
  const Tensor host_sizes = sizes.cpu();   // the synchronisation
  const int* kept = host_sizes.data_ptr<int>();
  std::vector<int64_t> capacity(layers);
  std::vector<int*> columns_out(layers);
  std::vector<void*> values_out(layers);
  std::vector<int64_t*> source_out(layers);
  std::vector<Tensor> result;
  result.reserve(5 * count_layers);
  int64_t kept_all = 0;
  for (int l = 0; l < layers; ++l) {
    TORCH_CHECK(kept[l] >= 0 && kept[l] <= nonzeros[l], "torch_sputnik::csr_topk_global: row_offsets of layer ", l,
                " do not ascend inside 0 .. ", nonzeros[l]);
    capacity[l] = kept[l];
    kept_all += kept[l];
    Tensor out_columns = at::empty({capacity[l]}, index_options);
    Tensor out_values = at::empty({capacity[l]}, csr[l].values.options());
    Tensor source = at::empty({capacity[l]}, index_options.dtype(at::kLong));
    columns_out[l] = out_columns.data_ptr<int>();
    values_out[l] = out_values.data_ptr();
    source_out[l] = source.data_ptr<int64_t>();
    result.insert(result.end(), {out_row_indices[l], out_row_offsets[l], out_columns, out_values, source});
  }
  TORCH_CHECK(kept_all == total, "torch_sputnik::csr_topk_global: the layers keep ", kept_all, " entries, not ",
              total, ": row_offsets do not describe the values");
  check_status(sputnik_hip_csr_topk_global_fill(layers, rows.data(), nonzeros.data(), offsets_in.data(),
                                                columns_in.data(), values_ptr.data(), value_bytes,
                                                workspace.data_ptr(), ws_bytes, capacity.data(), order_out.data(),
                                                offsets_out.data(), columns_out.data(), values_out.data(),
                                                source_out.data(), stream),
               "csr_topk_global (fill)");
  return result;
}

// ---- the fused attention with one mask per batch element (sputnik_hip.h:
// sparse_attention_many_mask_*, sparse_attention_heads_many_mask_*) ----

// softmax(scale * sddmm) @ v from the separate many-mask operators (float32, [R, S, D]):
// what the fused kernels do not serve.
Tensor attention_many_mask_composed(int64_t b, const Tensor& nonzeros, const Tensor& q,
                                    const Tensor& k, const Tensor& v, const Tensor& row_indices,
                                    const Tensor& row_offsets, const Tensor& column_indices,
                                    double scale, const Drop* drop = nullptr) {
  const int64_t m = q.size(-2), n = k.size(-2);
  const Tensor scores = sddmm_many_mask(b, m, n, nonzeros, row_indices, row_offsets,
                                        column_indices, q, k);
  Tensor weights = sparse_softmax_many_mask_scaled(b, m, nonzeros, scores, row_indices,
                                                   row_offsets, column_indices, scale);
  if (drop != nullptr) weights = dropout_values(weights, *drop);
  return spmm_many_mask(b, m, n, nonzeros, weights, row_indices, row_offsets, column_indices, v);
}

// q [R, m, d], k and v [R, n, d] (float32; half storage is widened: the heads op keeps it);
// replica r uses mask r / (R / b).  -> {out} or {out, lse [R, m]}.
std::vector<Tensor> sparse_attention_many_mask_run(int64_t b, const Tensor& nonzeros, const Tensor& q_in,
                                               const Tensor& k_in, const Tensor& v_in,
                                               const Tensor& row_indices, const Tensor& row_offsets,
                                               const Tensor& column_indices, double scale,
                                               bool want_lse, const c10::optional<Tensor>& plan,
                                               const Drop* drop = nullptr) {
  const Tensor q = as_float(q_in, "query");
  const Tensor k = as_float(k_in, "key");
  const Tensor v = as_float(v_in, "value");
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3,
              "sparse_attention_many_mask: expected [replicas, rows, d] query, key, value");
  TORCH_CHECK(k.sizes() == v.sizes(), "key and value must have one shape");
  TORCH_CHECK(q.size(0) == k.size(0) && q.size(2) == k.size(2),
              "query and key must have one replica count and head dimension");
  TORCH_CHECK(q.device() == k.device() && q.device() == v.device(),
              "query, key, value must be on one device");
  const c10::DeviceGuard guard(q.device());
  const ManyMask mm = check_many_mask(b, q.size(1), nonzeros, row_indices, row_offsets,
                                      column_indices, q, q.size(0));
  const int n = to_int(k.size(1), "n"), d = to_int(q.size(2), "d");
  const size_t ws_bytes =
      sputnik_hip_sparse_attention_many_mask_workspace_bytes(mm.masks, mm.m, n, d, mm.width);
  Tensor out = at::empty_like(q);
  Tensor lse = want_lse ? at::empty({mm.replicas, mm.m}, q.options()) : Tensor();
  int status = SPUTNIK_HIP_UNSUPPORTED;
  if (ws_bytes > 0) {
    auto args = [&](auto forward, auto... tail) {
      return forward(mm.masks, mm.m, n, d, mm.nonzeros.data(), mm.replicas,
                     mm.row_indices.data_ptr<int>(), mm.row_offsets.data_ptr<int>(),
                     mm.column_indices.data_ptr<int>(), q.data_ptr<float>(),
                     static_cast<int64_t>(mm.m) * d, k.data_ptr<float>(),
                     static_cast<int64_t>(n) * d, v.data_ptr<float>(), static_cast<int64_t>(n) * d,
                     static_cast<float>(scale), out.data_ptr<float>(),
                     static_cast<int64_t>(mm.m) * d, want_lse ? lse.data_ptr<float>() : nullptr,
                     static_cast<int64_t>(mm.m), tail...);
    };
    status = run_forward(args, sputnik_hip_sparse_attention_many_mask_forward,
                         sputnik_hip_sparse_attention_many_mask_forward_planned,
                         sputnik_hip_sparse_attention_many_mask_forward_dropout,
                         sputnik_hip_sparse_attention_many_mask_forward_planned_dropout, plan, ws_bytes, q,
                         drop);
  }
  if (status == SPUTNIK_HIP_UNSUPPORTED) {
    TORCH_CHECK(!want_lse || drop != nullptr, "sparse_attention_many_mask: lse needs a call the "
                "fused kernel serves (head dimension 64, 16-byte aligned operands)");
    const Tensor composed = attention_many_mask_composed(b, nonzeros, q, k, v, mm.row_indices,
                                                         mm.row_offsets, mm.column_indices, scale, drop);
    return attention_result(composed, Tensor(), false, drop);
  }
  check_status(status, "sparse_attention_many_mask");
  return attention_result(out, lse, want_lse, drop);
}

// Topology-only pre-pass of both many-mask attention forms (16 unused bytes when the kernels
// do not serve the shape: the planned call then composes the operators).
Tensor sparse_attention_many_mask_plan(int64_t b, int64_t m64, int64_t n64, int64_t d64,
                                       const Tensor& nonzeros, const Tensor& row_indices,
                                       const Tensor& row_offsets, const Tensor& column_indices) {
  TORCH_CHECK(row_offsets.is_cuda(), "row_offsets must be a GPU (HIP) tensor");
  const c10::DeviceGuard guard(row_offsets.device());
  const ManyMask mm = check_many_mask(b, m64, nonzeros, row_indices, row_offsets, column_indices,
                                      row_offsets, b);
  const int n = to_int(n64, "n"), d = to_int(d64, "d");
  const size_t bytes =
      sputnik_hip_sparse_attention_many_mask_workspace_bytes(mm.masks, mm.m, n, d, mm.width);
  Tensor plan = make_plan_tensor(bytes, row_offsets);
  if (bytes > 0)
    check_status(sputnik_hip_sparse_attention_many_mask_plan(
                     mm.masks, mm.m, n, d, mm.nonzeros.data(), mm.row_indices.data_ptr<int>(),
                     mm.row_offsets.data_ptr<int>(), mm.column_indices.data_ptr<int>(),
                     plan.data_ptr(), bytes, current_stream(row_offsets)),
                 "sparse_attention_many_mask_plan");
  return plan;
}

// q [B, H, m, d], k and v [B, H, n, d] views of one half type (any strides with a unit last
// one; batch element b uses mask b, so B = b); out stored as out_type (0 float32, else the
// operands' type) in a [B, m, H, d] buffer, returned as its [B, H, m, d] view; lse [B, H, m].
// A call the kernel does not serve is composed from the float32 many-mask operators.
std::vector<Tensor> sparse_attention_heads_many_mask_run(int64_t b, const Tensor& nonzeros,
                                                     const Tensor& q_in, const Tensor& k_in,
                                                     const Tensor& v_in, const Tensor& row_indices,
                                                     const Tensor& row_offsets,
                                                     const Tensor& column_indices, double scale,
                                                     int64_t out_type, bool want_lse,
                                                     const c10::optional<Tensor>& plan,
                                                     const Drop* drop = nullptr) {
  TORCH_CHECK(q_in.dim() == 4 && k_in.dim() == 4 && v_in.dim() == 4,
              "sparse_attention_heads_many_mask: expected [batch, heads, rows, d] views");
  const HeadOperand q = head_operand(q_in, "query"), k = head_operand(k_in, "key"),
                    v = head_operand(v_in, "value");
  const int dtype = check_head_operands(q, k, v, out_type, "sparse_attention_heads_many_mask");
  const auto st = q.t.scalar_type();
  const c10::DeviceGuard guard(q.t.device());
  TORCH_CHECK(q.batch == b, "sparse_attention_heads_many_mask: batch (", q.batch,
              ") must equal the number of masks (", b, ")");
  const ManyMask mm = check_many_mask(b, q.rows, nonzeros, row_indices, row_offsets,
                                      column_indices, q.t, q.batch * q.heads);
  const int n = to_int(k.rows, "n"), d = to_int(q.d, "d");
  const int heads = to_int(q.heads, "heads");
  const auto out_st = out_type == SPUTNIK_HIP_F32 ? at::kFloat : st;
  Tensor buffer = at::empty({q.batch, q.rows, q.heads, q.d}, q.t.options().dtype(out_st));
  Tensor out = buffer.permute({0, 2, 1, 3});
  const HeadOperand o = head_operand(out, "out");
  Tensor lse = want_lse ? at::empty({q.batch, q.heads, q.rows}, q.t.options().dtype(at::kFloat))
                        : Tensor();
  const size_t ws_bytes =
      sputnik_hip_sparse_attention_many_mask_workspace_bytes(mm.masks, mm.m, n, d, mm.width);
  int status = SPUTNIK_HIP_UNSUPPORTED;
  if (ws_bytes > 0) {
    auto args = [&](auto forward, auto... tail) {
      return forward(mm.masks, mm.m, n, d, mm.nonzeros.data(), mm.masks, heads,
                     mm.row_indices.data_ptr<int>(), mm.row_offsets.data_ptr<int>(),
                     mm.column_indices.data_ptr<int>(), dtype, q.t.data_ptr(), q.batch_stride,
                     q.head_stride, q.row_stride, k.t.data_ptr(), k.batch_stride, k.head_stride,
                     k.row_stride, v.t.data_ptr(), v.batch_stride, v.head_stride, v.row_stride,
                     static_cast<float>(scale), o.t.data_ptr(), static_cast<int>(out_type),
                     o.batch_stride, o.head_stride, o.row_stride,
                     want_lse ? lse.data_ptr<float>() : nullptr, static_cast<int64_t>(mm.m), tail...);
    };
    status = run_forward(args, sputnik_hip_sparse_attention_heads_many_mask_forward,
                         sputnik_hip_sparse_attention_heads_many_mask_forward_planned,
                         sputnik_hip_sparse_attention_heads_many_mask_forward_dropout,
                         sputnik_hip_sparse_attention_heads_many_mask_forward_planned_dropout, plan, ws_bytes,
                         q.t, drop);
  }
  if (status == SPUTNIK_HIP_UNSUPPORTED) {
    TORCH_CHECK(!want_lse || drop != nullptr, "sparse_attention_heads_many_mask: lse needs a call "
                "the fused kernel serves (head dimension 64, 16-byte aligned views)");
    // float32 per-head copies [B*H, rows, d] through the many-mask operators
    auto per_head = [&](const HeadOperand& x) {
      return x.t.to(at::kFloat).reshape({x.batch * x.heads, x.rows, x.d});
    };
    const Tensor product = attention_many_mask_composed(b, nonzeros, per_head(q), per_head(k),
                                                        per_head(v), mm.row_indices,
                                                        mm.row_offsets, mm.column_indices, scale, drop);
    out.copy_(product.reshape(out.sizes()));
    return attention_result(out, Tensor(), false, drop);
  }
  check_status(status, "sparse_attention_heads_many_mask");
  return attention_result(out, lse, want_lse, drop);
}

// The dropout forms of the three ops above: {out, lse, rng_state} (lse undefined on the
// composed route).
std::vector<Tensor> sparse_attention_heads_dropout(const Tensor& q, const Tensor& k, const Tensor& v,
                                                   const Tensor& row_indices, const Tensor& row_offsets,
                                                   const Tensor& column_indices, double scale,
                                                   int64_t out_type, double p,
                                                   const c10::optional<Tensor>& plan) {
  TORCH_CHECK(p > 0.0 && p < 1.0, "sparse_attention_heads_dropout: p must lie in (0, 1), got ", p);
  const c10::DeviceGuard guard(q.device());
  const Drop drop = make_drop(p, c10::nullopt, q);
  return sparse_attention_heads_run(q, k, v, row_indices, row_offsets, column_indices, scale, out_type,
                                    true, plan, &drop);
}

std::vector<Tensor> sparse_attention_many_mask_dropout(int64_t b, const Tensor& nonzeros, const Tensor& q,
                                                       const Tensor& k, const Tensor& v,
                                                       const Tensor& row_indices, const Tensor& row_offsets,
                                                       const Tensor& column_indices, double scale, double p,
                                                       const c10::optional<Tensor>& plan) {
  TORCH_CHECK(p > 0.0 && p < 1.0, "sparse_attention_many_mask_dropout: p must lie in (0, 1), got ", p);
  const c10::DeviceGuard guard(q.device());
  const Drop drop = make_drop(p, c10::nullopt, q);
  return sparse_attention_many_mask_run(b, nonzeros, q, k, v, row_indices, row_offsets, column_indices,
                                        scale, true, plan, &drop);
}

std::vector<Tensor> sparse_attention_heads_many_mask_dropout(
    int64_t b, const Tensor& nonzeros, const Tensor& q, const Tensor& k, const Tensor& v,
    const Tensor& row_indices, const Tensor& row_offsets, const Tensor& column_indices, double scale,
    int64_t out_type, double p, const c10::optional<Tensor>& plan) {
  TORCH_CHECK(p > 0.0 && p < 1.0, "sparse_attention_heads_many_mask_dropout: p must lie in (0, 1), got ", p);
  const c10::DeviceGuard guard(q.device());
  const Drop drop = make_drop(p, c10::nullopt, q);
  return sparse_attention_heads_many_mask_run(b, nonzeros, q, k, v, row_indices, row_offsets,
                                              column_indices, scale, out_type, true, plan, &drop);
}

// the registered forms without dropout
std::vector<Tensor> sparse_attention_heads(const Tensor& q, const Tensor& k, const Tensor& v,
                                           const Tensor& row_indices, const Tensor& row_offsets,
                                           const Tensor& column_indices, double scale, int64_t out_type,
                                           bool want_lse, const c10::optional<Tensor>& plan) {
  return sparse_attention_heads_run(q, k, v, row_indices, row_offsets, column_indices, scale, out_type,
                                    want_lse, plan);
}

std::vector<Tensor> sparse_attention_many_mask(int64_t b, const Tensor& nonzeros, const Tensor& q,
                                               const Tensor& k, const Tensor& v,
                                               const Tensor& row_indices, const Tensor& row_offsets,
                                               const Tensor& column_indices, double scale,
                                               bool want_lse, const c10::optional<Tensor>& plan) {
  return sparse_attention_many_mask_run(b, nonzeros, q, k, v, row_indices, row_offsets, column_indices,
                                        scale, want_lse, plan);
}

std::vector<Tensor> sparse_attention_heads_many_mask(int64_t b, const Tensor& nonzeros, const Tensor& q,
                                                     const Tensor& k, const Tensor& v,
                                                     const Tensor& row_indices, const Tensor& row_offsets,
                                                     const Tensor& column_indices, double scale,
                                                     int64_t out_type, bool want_lse,
                                                     const c10::optional<Tensor>& plan) {
  return sparse_attention_heads_many_mask_run(b, nonzeros, q, k, v, row_indices, row_offsets,
                                              column_indices, scale, out_type, want_lse, plan);
}

// Layout pass of the reference's modules (modules/sparse_linear.py:89,
// modules/sparse_attention.py:108-126): x[..., R, C] -> contiguous [..., C, R],
// i.e. `x.transpose(-1, -2).contiguous()` as ONE tiled kernel, optionally
// changing the storage type on the way (out_type: -1 keep, 0 float32, 1 float16,
// 2 bfloat16; half <-> float and equal types).
Tensor transpose_last2_as(const Tensor& x_in, int64_t out_type) {
  TORCH_CHECK(x_in.is_cuda(), "transpose_last2: expected a GPU (HIP) tensor, got ", x_in.device());
  TORCH_CHECK(x_in.dim() >= 2, "transpose_last2: expected at least 2 dimensions, got ", x_in.dim());
  const int in_code = type_code(x_in.scalar_type());
  const int out_code = out_type < 0 ? in_code : static_cast<int>(out_type);
  const at::ScalarType out_dtype = out_code == SPUTNIK_HIP_F32 ? at::kFloat
                                   : out_code == SPUTNIK_HIP_F16 ? at::kHalf : at::kBFloat16;
  const bool native = in_code >= 0 && out_code >= 0 && out_code <= 2 &&
                      (in_code == out_code || in_code == SPUTNIK_HIP_F32 || out_code == SPUTNIK_HIP_F32);
  if (!native) {   // (other element types: ATen's strided copy)
    Tensor t = x_in.transpose(-1, -2).contiguous();
    return out_type < 0 ? t : t.to(out_dtype);
  }
  const Tensor x = x_in.contiguous();
  const c10::DeviceGuard guard(x.device());
  std::vector<int64_t> sizes = x.sizes().vec();
  const int rows = to_int(sizes[sizes.size() - 2], "rows"), cols = to_int(sizes.back(), "cols");
  std::swap(sizes[sizes.size() - 2], sizes[sizes.size() - 1]);
  Tensor out = at::empty(sizes, x.options().dtype(out_dtype));
  const int64_t per = static_cast<int64_t>(rows) * cols;
  const int batches = per == 0 ? 0 : to_int(x.numel() / per, "batches");
  check_status(sputnik_hip_transpose_cast_batched(batches, rows, cols, x.data_ptr(), in_code, per,
                                                  out.data_ptr(), out_code, per,
                                                  current_stream(x)),
               "transpose_last2");
  return out;
}

Tensor transpose_last2(const Tensor& x) { return transpose_last2_as(x, -1); }

// values[..., permutation] for value arrays [nnz] / [R, nnz] that share one int32
// permutation (the transposed order of a static pattern): `index_select(-1, perm)`
// as one kernel that reads the permutation once for all rows.
Tensor permute_last(const Tensor& values_in, const Tensor& permutation) {
  const Tensor values = as_float(values_in, "values");
  TORCH_CHECK(values.dim() == 1 || values.dim() == 2, "values should have 1 or 2 dimensions, got ",
              values.dim());
  check_permutation(permutation, values.size(-1), values);
  const c10::DeviceGuard guard(values.device());
  const int n = to_int(values.size(-1), "n");
  const int rows = values.dim() == 2 ? to_int(values.size(0), "rows") : 1;
  Tensor out = at::empty_like(values);
  check_status(sputnik_hip_permute_last_batched(n, rows, values.data_ptr<float>(), n,
                                                permutation.data_ptr<int>(),
                                                out.data_ptr<float>(), n, current_stream(values)),
               "permute_last");
  return out;
}

// permute_last through LDS for many rows; the lists come from
// torch_sputnik_amd.functional (one stable sort per cached permutation)
Tensor permute_last_banded(const Tensor& values_in, const Tensor& dest_list,
                           const Tensor& source_in_band) {
  const Tensor values = as_float(values_in, "values");
  TORCH_CHECK(values.dim() == 1 || values.dim() == 2, "values should have 1 or 2 dimensions, got ",
              values.dim());
  for (const Tensor* t : {&dest_list, &source_in_band})
    TORCH_CHECK(t->scalar_type() == at::kInt && t->dim() == 1 && t->is_contiguous() &&
                    t->device() == values.device() && t->size(0) == values.size(-1),
                "dest_list / source_in_band must be contiguous int32 vectors of ",
                values.size(-1), " entries on ", values.device());
  const c10::DeviceGuard guard(values.device());
  const int n = to_int(values.size(-1), "n");
  const int rows = values.dim() == 2 ? to_int(values.size(0), "rows") : 1;
  Tensor out = at::empty_like(values);
  check_status(sputnik_hip_permute_banded_batched(
                   n, rows, values.data_ptr<float>(), n, dest_list.data_ptr<int>(),
                   source_in_band.data_ptr<int>(), out.data_ptr<float>(), n,
                   current_stream(values)),
               "permute_last_banded");
  return out;
}

int64_t permute_band_size() { return sputnik_hip_permute_band_size(); }

}  // namespace

TORCH_LIBRARY(torch_sputnik, m) {
  m.def(
      "spmm(int m, int k, Tensor values, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices, Tensor dense_matrix) -> Tensor");
  m.def(
      "left_spmm(int m, int k, Tensor values, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices, Tensor dense_matrix) -> Tensor");
  m.def(
      "left_spmm_half_tiles(int m, int k, Tensor values, Tensor row_offsets, Tensor column_indices, "
      "Tensor dense_matrix, int tile_type) -> Tensor");
  m.def("half_linear_image(int out_features, int in_features, Tensor values, Tensor row_offsets, "
        "Tensor column_indices, int tile_type) -> Tensor");
  m.def("half_planes(Tensor t, int tile_type) -> Tensor");
  m.def("half_linear_forward(int out_features, Tensor image, int values_type, Tensor x) -> Tensor");
  m.def("half_linear_plan(int out_features, int in_features, Tensor row_offsets, Tensor column_indices) "
        "-> Tensor");
  m.def("half_linear_weight_gradient(int out_features, Tensor row_offsets, Tensor column_indices, "
        "Tensor grad, bool grad_is_planes, Tensor x, Tensor? plan) -> Tensor");
  m.def("half_linear_weight_gradient_dense(int out_features, Tensor row_offsets, Tensor column_indices, "
        "Tensor grad, bool grad_is_planes, Tensor x, Tensor? plan) -> (Tensor, Tensor)");
  m.def("dense_weight_gradient(Tensor grad, bool grad_is_planes, Tensor x, bool x_is_planes, int x_layout, "
        "int tile_type, int out_features, int in_features, int seq, int batch) -> Tensor");
  m.def("half_linear_input_gradient(int out_features, int in_features, Tensor grad, bool grad_is_planes, "
        "Tensor image, int values_type, Tensor like, int batch, int seq) -> Tensor");
  m.def(
      "sddmm(int m, int n, Tensor row_indices, Tensor row_offsets, Tensor column_indices, "
      "Tensor lhs_matrix, Tensor rhs_matrix) -> Tensor");
  m.def(
      "sddmm_narrow(int m, int n, Tensor row_indices, Tensor row_offsets, Tensor column_indices, "
      "Tensor lhs_matrix, Tensor rhs_matrix) -> Tensor");
  m.def(
      "sparse_softmax(Tensor values, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices) -> Tensor");
  m.def(
      "csr_transpose(int m, int n, Tensor values, Tensor row_offsets, Tensor column_indices) "
      "-> Tensor[]");
  m.def(
      "csr_transpose_with_permutation(int m, int n, Tensor values, Tensor row_offsets, "
      "Tensor column_indices, bool checked=True) -> Tensor[]");
  // extensions
  m.def(
      "spmm_bias(int m, int k, Tensor values, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices, Tensor bias, Tensor dense_matrix) -> Tensor");
  m.def(
      "spmm_bias_relu(int m, int k, Tensor values, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices, Tensor bias, Tensor dense_matrix) -> Tensor");
  m.def(
      "sparse_softmax_scaled(Tensor values, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices, float scale) -> Tensor");
  m.def(
      "sparse_softmax_backward(Tensor softmax_out, Tensor grad_out, Tensor row_offsets, "
      "float scale) -> Tensor");
  m.def(
      "sparse_attention(Tensor query, Tensor key, Tensor value, Tensor row_indices, "
      "Tensor row_offsets, Tensor column_indices, float scale) -> Tensor");
  m.def(
      "sparse_attention_with_lse(Tensor query, Tensor key, Tensor value, Tensor row_indices, "
      "Tensor row_offsets, Tensor column_indices, float scale) -> Tensor[]");
  m.def(
      "sparse_attention_with_lse_planned(Tensor query, Tensor key, Tensor value, "
      "Tensor row_indices, Tensor row_offsets, Tensor column_indices, float scale, Tensor plan) "
      "-> Tensor[]");
  m.def(
      "sparse_attention_rows(Tensor query, Tensor key, Tensor value, Tensor row_indices, "
      "Tensor row_offsets, Tensor column_indices, float scale, float p) -> Tensor[]");
  m.def(
      "sparse_attention_backward(Tensor query, Tensor key, Tensor value, Tensor out, "
      "Tensor grad_out, Tensor lse, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices, Tensor? t_row_indices, Tensor? t_row_offsets, "
      "Tensor? t_column_indices, Tensor? permutation, float scale, float p, Tensor? rng_state, "
      "bool want_q, bool want_k, bool want_v) -> Tensor[]");
  m.def(
      "spmm_plan(int m, int k, int n, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices) -> Tensor");
  m.def(
      "spmm_planned(int m, int k, Tensor values, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices, Tensor dense_matrix, Tensor plan) -> Tensor");
  m.def(
      "left_spmm_planned(int m, int k, Tensor values, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices, Tensor dense_matrix, Tensor plan) -> Tensor");
  m.def(
      "sddmm_plan(int m, int n, int k, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices) -> Tensor");
  m.def(
      "sddmm_planned(int m, int n, Tensor row_indices, Tensor row_offsets, Tensor column_indices, "
      "Tensor lhs_matrix, Tensor rhs_matrix, Tensor plan) -> Tensor");
  m.def(
      "sddmm_sum_plan(int m, int n, int k, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices) -> Tensor");
  m.def(
      "sddmm_sum(int m, int n, Tensor row_indices, Tensor row_offsets, Tensor column_indices, "
      "Tensor lhs_matrix, Tensor rhs_matrix) -> Tensor");
  m.def(
      "sddmm_sum_planned(int m, int n, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices, Tensor lhs_matrix, Tensor rhs_matrix, Tensor plan) -> Tensor");
  m.def(
      "sddmm_sum_group_planned(int m, int n, Tensor[] row_indices, Tensor[] row_offsets, "
      "Tensor[] column_indices, Tensor[] lhs_matrices, Tensor rhs_matrix, Tensor[] plans) -> Tensor[]");
  m.def(
      "sparse_attention_plan(int m, int n, int d, Tensor row_indices, Tensor row_offsets, "
      "Tensor column_indices) -> Tensor");
  m.def(
      "sparse_attention_planned(Tensor query, Tensor key, Tensor value, Tensor row_indices, "
      "Tensor row_offsets, Tensor column_indices, float scale, Tensor plan) -> Tensor");
  m.def(
      "sparse_attention_heads(Tensor query, Tensor key, Tensor value, Tensor row_indices, "
      "Tensor row_offsets, Tensor column_indices, float scale, int out_type, bool want_lse, "
      "Tensor? plan) -> Tensor[]");
  m.def(
      "half_linear_rows(int out_features, Tensor image, int values_type, Tensor x, Tensor? out, "
      "int out_type) -> Tensor");
  m.def(
      "spmm_many_mask(int b, int m, int k, Tensor nonzeros, Tensor values, Tensor row_indices, "
      "Tensor row_offsets, Tensor column_indices, Tensor dense_matrix) -> Tensor");
  m.def(
      "sddmm_many_mask(int b, int m, int n, Tensor nonzeros, Tensor row_indices, "
      "Tensor row_offsets, Tensor column_indices, Tensor lhs_matrix, Tensor rhs_matrix) -> Tensor");
  m.def(
      "sparse_softmax_many_mask(int b, int m, Tensor nonzeros, Tensor values, "
      "Tensor row_indices, Tensor row_offsets, Tensor column_indices) -> Tensor");
  m.def(
      "sparse_softmax_many_mask_scaled(int b, int m, Tensor nonzeros, Tensor values, "
      "Tensor row_indices, Tensor row_offsets, Tensor column_indices, float scale) -> Tensor");
  m.def(
      "sparse_softmax_backward_many_mask(int b, int m, Tensor nonzeros, Tensor softmax_out, "
      "Tensor grad_out, Tensor row_offsets, float scale) -> Tensor");
  m.def(
      "csr_transpose_many_mask(int b, int m, int n, Tensor nonzeros, Tensor values, "
      "Tensor row_offsets, Tensor column_indices) -> Tensor[]");
  m.def("dense_to_csr(Tensor dense, bool with_values) -> Tensor[]");
  m.def("row_order(Tensor row_offsets) -> Tensor");
  m.def("topk_to_csr(Tensor scores, int per_row, int total, Tensor? values_from) -> Tensor[]");
  // (no tensor among the arguments of a fresh draw: registered for every backend, GPU devices only)
  m.def("random_csr(int m, int n, int per_row, int total, ScalarType dtype, float scale, Device device, "
        "Tensor? rng_state, int key_mask) -> Tensor[]", &random_csr);
  m.def("attention_pattern_csr(int m, int n, int offset, int window_left, int window_right, int dilation, "
        "int block, int summary_stride, int summary_first, int random_block, int random_threshold, bool causal, "
        "bool global_rows, Tensor? global_flags, Device device, Tensor? rng_state) -> Tensor[]",
        &attention_pattern_csr);
  m.def("csr_regrow(Tensor values, Tensor row_offsets, Tensor column_indices, Tensor drop_counts, "
        "Tensor scores) -> Tensor[]");
  m.def("csr_regrow_total(Tensor values, Tensor row_offsets, Tensor column_indices, int drop, "
        "Tensor scores) -> Tensor[]");
  m.def("csr_regrow_random(Tensor values, Tensor row_offsets, Tensor column_indices, Tensor drop_counts, int n, "
        "float grow_scale, Tensor? rng_state, int key_mask) -> Tensor[]");
  m.def("csr_regrow_total_random(Tensor values, Tensor row_offsets, Tensor column_indices, int drop, int n, "
        "float grow_scale, Tensor? rng_state, int key_mask) -> Tensor[]");
  m.def("csr_topk(Tensor values, Tensor row_offsets, Tensor column_indices, int per_row, int total) -> Tensor[]");
  m.def("csr_topk_global(Tensor[] values, Tensor[] row_offsets, Tensor[] column_indices, int total) -> Tensor[]");
  m.def(
      "sparse_attention_many_mask(int b, Tensor nonzeros, Tensor query, Tensor key, Tensor value, "
      "Tensor row_indices, Tensor row_offsets, Tensor column_indices, float scale, bool want_lse, "
      "Tensor? plan) -> Tensor[]");
  m.def(
      "sparse_attention_many_mask_plan(int b, int m, int n, int d, Tensor nonzeros, "
      "Tensor row_indices, Tensor row_offsets, Tensor column_indices) -> Tensor");
  m.def(
      "sparse_attention_heads_many_mask(int b, Tensor nonzeros, Tensor query, Tensor key, "
      "Tensor value, Tensor row_indices, Tensor row_offsets, Tensor column_indices, float scale, "
      "int out_type, bool want_lse, Tensor? plan) -> Tensor[]");
  // attention dropout
  m.def("sparse_dropout(Tensor values, float p, Tensor? rng_state) -> Tensor[]");
  m.def(
      "sparse_attention_dropout(Tensor query, Tensor key, Tensor value, Tensor row_indices, "
      "Tensor row_offsets, Tensor column_indices, float scale, float p, Tensor? plan) -> Tensor[]");
  m.def(
      "sparse_attention_heads_dropout(Tensor query, Tensor key, Tensor value, Tensor row_indices, "
      "Tensor row_offsets, Tensor column_indices, float scale, int out_type, float p, "
      "Tensor? plan) -> Tensor[]");
  m.def(
      "sparse_attention_many_mask_dropout(int b, Tensor nonzeros, Tensor query, Tensor key, "
      "Tensor value, Tensor row_indices, Tensor row_offsets, Tensor column_indices, float scale, "
      "float p, Tensor? plan) -> Tensor[]");
  m.def(
      "sparse_attention_heads_many_mask_dropout(int b, Tensor nonzeros, Tensor query, Tensor key, "
      "Tensor value, Tensor row_indices, Tensor row_offsets, Tensor column_indices, float scale, "
      "int out_type, float p, Tensor? plan) -> Tensor[]");
  m.def("permute_last(Tensor values, Tensor permutation) -> Tensor");
  m.def("permute_last_banded(Tensor values, Tensor dest_list, Tensor source_in_band) -> Tensor");
  m.def("permute_band_size() -> int", &permute_band_size);
  m.def(
      "spmm_permuted(int m, int k, Tensor values, Tensor permutation, Tensor row_indices, "
      "Tensor row_offsets, Tensor column_indices, Tensor dense_matrix, Tensor? plan) -> Tensor");
  m.def(
      "spmm_transposed_out(int m, int k, Tensor values, Tensor? permutation, Tensor row_indices, "
      "Tensor row_offsets, Tensor column_indices, Tensor dense_matrix, int block_rows, bool left, "
      "Tensor? plan) -> Tensor");
  m.def(
      "left_spmm_group(int m, int k, Tensor[] values, Tensor[] row_indices, Tensor[] row_offsets, "
      "Tensor[] column_indices, Tensor dense_matrix, int block_rows) -> Tensor[]");
  m.def(
      "left_spmm_group_sum(int m, int k, Tensor[] values, Tensor[] permutations, "
      "Tensor[] row_indices, Tensor[] row_offsets, Tensor[] column_indices, "
      "Tensor[] dense_matrices) -> Tensor");
  m.def(
      "left_spmm_permuted(int m, int k, Tensor values, Tensor permutation, Tensor row_indices, "
      "Tensor row_offsets, Tensor column_indices, Tensor dense_matrix, Tensor? plan) -> Tensor");
  m.def("transpose_last2(Tensor x) -> Tensor");
  m.def("transpose_last2_as(Tensor x, int out_type) -> Tensor");
}

// "CUDA" is the dispatch key of HIP tensors in a ROCm build of PyTorch.
TORCH_LIBRARY_IMPL(torch_sputnik, CUDA, m) {
  m.impl("spmm", &spmm_plain<false>);
  m.impl("left_spmm", &spmm_plain<true>);
  m.impl("sddmm", &sddmm);
  m.impl("sddmm_narrow", &sddmm_narrow);
  m.impl("sparse_softmax", &sparse_softmax);
  m.impl("csr_transpose", &csr_transpose);
  m.impl("csr_transpose_with_permutation", &csr_transpose_with_permutation);
  m.impl("spmm_bias", &spmm_bias<false>);
  m.impl("spmm_bias_relu", &spmm_bias<true>);
  m.impl("sparse_softmax_scaled", &sparse_softmax_scaled);
  m.impl("sparse_softmax_backward", &sparse_softmax_backward);
  m.impl("sparse_attention", &sparse_attention);
  m.impl("sparse_attention_with_lse", &sparse_attention_with_lse);
  m.impl("sparse_attention_with_lse_planned", &sparse_attention_with_lse_planned);
  m.impl("sparse_attention_rows", &sparse_attention_rows);
  m.impl("sparse_attention_backward", &sparse_attention_backward);
  m.impl("spmm_plan", &spmm_plan);
  m.impl("spmm_planned", &spmm_planned<false>);
  m.impl("left_spmm_planned", &spmm_planned<true>);
  m.impl("sddmm_plan", &sddmm_plan);
  m.impl("sddmm_planned", &sddmm_planned);
  m.impl("left_spmm_half_tiles", &left_spmm_half_tiles);
  m.impl("half_linear_image", &half_linear_image);
  m.impl("half_planes", &half_planes);
  m.impl("half_linear_forward", &half_linear_forward);
  m.impl("half_linear_plan", &half_linear_plan);
  m.impl("half_linear_weight_gradient", &half_linear_weight_gradient);
  m.impl("half_linear_weight_gradient_dense", &half_linear_weight_gradient_dense);
  m.impl("dense_weight_gradient", &dense_weight_gradient);
  m.impl("half_linear_input_gradient", &half_linear_input_gradient);
  m.impl("sddmm_sum", &sddmm_sum);
  m.impl("sddmm_sum_plan", &sddmm_sum_plan);
  m.impl("sddmm_sum_planned", &sddmm_sum_planned);
  m.impl("sddmm_sum_group_planned", &sddmm_sum_group_planned);
  m.impl("sparse_attention_plan", &sparse_attention_plan);
  m.impl("sparse_attention_planned", &sparse_attention_planned);
  m.impl("sparse_attention_heads", &sparse_attention_heads);
  m.impl("half_linear_rows", &half_linear_rows);
  m.impl("spmm_many_mask", &spmm_many_mask);
  m.impl("sddmm_many_mask", &sddmm_many_mask);
  m.impl("sparse_softmax_many_mask", &sparse_softmax_many_mask);
  m.impl("sparse_softmax_many_mask_scaled", &sparse_softmax_many_mask_scaled);
  m.impl("sparse_softmax_backward_many_mask", &sparse_softmax_backward_many_mask);
  m.impl("csr_transpose_many_mask", &csr_transpose_many_mask);
  m.impl("dense_to_csr", &dense_to_csr);
  m.impl("row_order", &row_order);
  m.impl("topk_to_csr", &topk_to_csr);
  m.impl("csr_regrow", &csr_regrow);
  m.impl("csr_regrow_total", &csr_regrow_total);
  m.impl("csr_regrow_random", &csr_regrow_random);
  m.impl("csr_regrow_total_random", &csr_regrow_total_random);
  m.impl("csr_topk", &csr_topk);
  m.impl("csr_topk_global", &csr_topk_global);
  m.impl("sparse_attention_many_mask", &sparse_attention_many_mask);
  m.impl("sparse_attention_many_mask_plan", &sparse_attention_many_mask_plan);
  m.impl("sparse_attention_heads_many_mask", &sparse_attention_heads_many_mask);
  m.impl("sparse_dropout", &sparse_dropout);
  m.impl("sparse_attention_dropout", &sparse_attention_dropout);
  m.impl("sparse_attention_heads_dropout", &sparse_attention_heads_dropout);
  m.impl("sparse_attention_many_mask_dropout", &sparse_attention_many_mask_dropout);
  m.impl("sparse_attention_heads_many_mask_dropout", &sparse_attention_heads_many_mask_dropout);
  m.impl("permute_last", &permute_last);
  m.impl("permute_last_banded", &permute_last_banded);
  m.impl("spmm_permuted", &spmm_permuted<false>);
  m.impl("spmm_transposed_out", &spmm_transposed_out);
  m.impl("left_spmm_group", &left_spmm_group);
  m.impl("left_spmm_group_sum", &left_spmm_group_sum);
  m.impl("left_spmm_permuted", &spmm_permuted<true>);
  m.impl("transpose_last2", &transpose_last2);
  m.impl("transpose_last2_as", &transpose_last2_as);
}
