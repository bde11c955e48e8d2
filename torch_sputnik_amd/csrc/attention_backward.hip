// Fused sparse attention backward for gfx950:
//
//   p  = exp(scale * <q_i, k_j> - lse_i)          pd = p * keep(r, e) / (1 - p_drop)
//   dp = <dO_i, v_j> * keep(r, e) / (1 - p_drop)  D_i = <dO_i, O_i>
//   ds = p * (dp - D_i) * scale
//   dQ_i += ds * k_j      dK_j += ds * q_i      dV_j += pd * dO_i
//
// for every stored entry e = (i, j) of the mask, without the [replicas, nnz] score, weight
// and gradient arrays the composed backward (functional._attention_backward) materialises.
// Two launches, each output row written by exactly one 16-lane row group (no atomics, the
// same sums in the same order on every run):
//   rows:    one row group per query row i of the mask (in row_indices order: rows of like
//            length side by side).  It forms D_i from the dO and O rows, stores it into the caller's workspace for
//            the second launch and, when dQ is wanted, walks the row's entries: K and V rows
//            gathered from L2 (float4 per lane, 256 contiguous bytes per load), the two dot
//            products reduced over the 16 lanes by DPP, dQ_i accumulated in registers.
//   columns: one row group per key row j of the TRANSPOSED mask (its row_indices order):
//            slot t holds query row i and the original entry e = permutation[t], which keys
//            the dropout decision (consecutive slots are not consecutive entries).  Q and dO rows are gathered, lse_i and D_i read as scalars
//            broadcast to the 16 lanes; dK_j and dV_j are accumulated in registers.
// A row group walks its list in windows of 16 entries: with dropout, lane u decides entry u
// of the window (one Philox call per lane and window, keep_window) and a ballot shares the
// bits.  Entries are taken kUnroll at a time so that their gathers are in flight together.
// Rows without entries give zero gradient rows (their lse of -inf is never read).
// The kernels are templates on the head dimension D (64 or 128): a lane owns D / 16 columns,
// one float4 at D = 64 and two at D = 128 (columns 4i.. and 64 + 4i..: attention_rowgroup.h).
// Offsets inside a replica are 32-bit: m * D * 4 and n * D * 4 below 2^32 (supported()).
#include <math.h>

#include <utility>

#include "attention_rowgroup.h"

namespace sputnik_hip {
namespace {

using namespace rowgroup;

// Entries whose gathers are issued together, at either D.  Per entry a lane holds 2 * D / 16
// floats of gathered rows; at D = 128 the columns kernel, with two accumulators and two rows
// of its own besides, still stays out of scratch with four (104 VGPRs with dropout).
constexpr int kUnroll = 4;

// Pointers and strides of one launch (replica 0 of the launch at the bases).
struct BackwardArgs {
  int m, n;
  const int* row_indices;     // of the mask (rows launch) or of its transpose (columns launch)
  const int* row_offsets;
  const int* column_indices;
  const int* permutation;     // columns launch: original entry of each transposed slot
  const float* q; int64_t q_stride;
  const float* k; int64_t k_stride;
  const float* v; int64_t v_stride;
  const float* out; int64_t out_stride;
  const float* dout; int64_t dout_stride;
  const float* lse; int64_t lse_stride;
  float* dterm;               // [replicas, m] workspace: D_i
  float* dq; int64_t dq_stride;
  float* dk; int64_t dk_stride;
  float* dv; int64_t dv_stride;
  float scale;
};

// Rows launch: D_i for every query row, and dQ_i when a.dq is set.
template <int D, typename... Drop>
__global__ __launch_bounds__(kThreads) void attention_backward_rows_kernel(BackwardArgs a,
                                                                           Drop... drop_arg) {
  constexpr bool DROP = sizeof...(Drop) > 0;
  const DropArgs drop = drop_of(drop_arg...);
  const int slot = blockIdx.x * kRowsPerBlock + threadIdx.x / kGroup;
  if (slot >= a.m) return;   // (the whole row group: the DPP reductions stay inside it)
  const int i = threadIdx.x % kGroup;
  const int replica = blockIdx.y;
  const int row = a.row_indices[slot];
  const unsigned own = static_cast<unsigned>(row) * D + 4 * i;
  const Frag<D> go = load_frag<D>(a.dout + replica * a.dout_stride, own);
  const Frag<D> o = load_frag<D>(a.out + replica * a.out_stride, own);
  const float dterm = group_sum<kGroup>(dot(go, o));
  if (i == 0) a.dterm[static_cast<int64_t>(replica) * a.m + row] = dterm;
  if (a.dq == nullptr) return;

  const float* __restrict__ k = a.k + replica * a.k_stride;
  const float* __restrict__ v = a.v + replica * a.v_stride;
  const Frag<D> qs = scaled(load_frag<D>(a.q + replica * a.q_stride, own), a.scale);
  const int p0 = a.row_offsets[row], p1 = a.row_offsets[row + 1];
  const float lse = p1 > p0 ? a.lse[replica * a.lse_stride + row] : 0.f;
  PhiloxKey key{};
  if constexpr (DROP) key = philox_key(drop, false);
  const int drop_r = replica + drop.replica0;
  Frag<D> acc = zero_frag<D>();

  auto entry = [&](bool kept, const Frag<D>& kf, const Frag<D>& vf) {
    const float s = group_sum<kGroup>(dot(qs, kf));
    float dp = group_sum<kGroup>(dot(go, vf));
    if constexpr (DROP) dp = kept ? dp * drop.scale : 0.f;
    const float ds = __expf(s - lse) * (dp - dterm) * a.scale;
    fma(acc, ds, kf);
  };

  for (int w = p0; w < p1; w += kGroup) {   // windows of 16 entries
    const int end = min(w + kGroup, p1);
    unsigned bits = 0xffffu;
    if constexpr (DROP) bits = keep_window(key, drop, drop_r, w, end, [](int e) { return e; });
    int p = w;
    for (; p + kUnroll <= end; p += kUnroll) {
      Frag<D> kf[kUnroll], vf[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const unsigned col = static_cast<unsigned>(a.column_indices[p + u]) * D + 4 * i;
        kf[u] = load_frag<D>(k, col);
        vf[u] = load_frag<D>(v, col);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) entry((bits >> (p + u - w)) & 1u, kf[u], vf[u]);
    }
    for (; p < end; ++p) {
      const unsigned col = static_cast<unsigned>(a.column_indices[p]) * D + 4 * i;
      entry((bits >> (p - w)) & 1u, load_frag<D>(k, col), load_frag<D>(v, col));
    }
  }
  store_frag<D>(a.dq + replica * a.dq_stride, own, acc);
}

// Columns launch over the transposed mask: dK_j and / or dV_j (a.dk, a.dv may be NULL).
template <int D, typename... Drop>
__global__ __launch_bounds__(kThreads) void attention_backward_columns_kernel(BackwardArgs a,
                                                                              Drop... drop_arg) {
  constexpr bool DROP = sizeof...(Drop) > 0;
  const DropArgs drop = drop_of(drop_arg...);
  const int slot = blockIdx.x * kRowsPerBlock + threadIdx.x / kGroup;
  if (slot >= a.n) return;
  const int i = threadIdx.x % kGroup;
  const int replica = blockIdx.y;
  const int row = a.row_indices[slot];   // key row j
  const unsigned own = static_cast<unsigned>(row) * D + 4 * i;
  const Frag<D> ks = scaled(load_frag<D>(a.k + replica * a.k_stride, own), a.scale);
  const Frag<D> vf = load_frag<D>(a.v + replica * a.v_stride, own);
  const float* __restrict__ q = a.q + replica * a.q_stride;
  const float* __restrict__ dout = a.dout + replica * a.dout_stride;
  const float* __restrict__ lse = a.lse + replica * a.lse_stride;
  const float* __restrict__ dterm = a.dterm + static_cast<int64_t>(replica) * a.m;
  PhiloxKey key{};
  if constexpr (DROP) key = philox_key(drop, false);
  const int drop_r = replica + drop.replica0;
  Frag<D> acc_k = zero_frag<D>();
  Frag<D> acc_v = zero_frag<D>();

  auto entry = [&](bool kept, int qrow, const Frag<D>& qf, const Frag<D>& go) {
    const float s = group_sum<kGroup>(dot(qf, ks));
    float dp = group_sum<kGroup>(dot(go, vf));
    const float pr = __expf(s - lse[qrow]);
    float pd = pr;
    if constexpr (DROP) {
      dp = kept ? dp * drop.scale : 0.f;
      pd = kept ? pr * drop.scale : 0.f;
    }
    fma(acc_k, pr * (dp - dterm[qrow]) * a.scale, qf);
    fma(acc_v, pd, go);
  };

  const int t0 = a.row_offsets[row], t1 = a.row_offsets[row + 1];
  for (int w = t0; w < t1; w += kGroup) {   // windows of 16 slots
    const int end = min(w + kGroup, t1);
    unsigned bits = 0xffffu;
    if constexpr (DROP)
      bits = keep_window(key, drop, drop_r, w, end, [&](int t) { return a.permutation[t]; });
    int t = w;
    for (; t + kUnroll <= end; t += kUnroll) {
      int qrow[kUnroll];
      Frag<D> qf[kUnroll], go[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        qrow[u] = a.column_indices[t + u];
        const unsigned off = static_cast<unsigned>(qrow[u]) * D + 4 * i;
        qf[u] = load_frag<D>(q, off);
        go[u] = load_frag<D>(dout, off);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) entry((bits >> (t + u - w)) & 1u, qrow[u], qf[u], go[u]);
    }
    for (; t < end; ++t) {
      const int qrow = a.column_indices[t];
      const unsigned off = static_cast<unsigned>(qrow) * D + 4 * i;
      entry((bits >> (t - w)) & 1u, qrow, load_frag<D>(q, off), load_frag<D>(dout, off));
    }
  }
  if (a.dk != nullptr) store_frag<D>(a.dk + replica * a.dk_stride, own, acc_k);
  if (a.dv != nullptr) store_frag<D>(a.dv + replica * a.dv_stride, own, acc_v);
}

bool supported(int m, int n, int d, int nonzeros) {
  return (d == 64 || d == 128) && m > 0 && n > 0 && nonzeros >= 0 && rows_fit_32_bits(m, d) &&
         rows_fit_32_bits(n, d);
}

// Launch `kernel` once per 65535 replicas, the bases moved to the launch's first replica.
template <typename Kernel>
int launch_replicas(Kernel kernel, int rows, int replicas, BackwardArgs a, const DropArgs* drop,
                    hipStream_t stream) {
  for (int r0 = 0; r0 < replicas; r0 += kMaxGridYZ) {
    const int ry = min(replicas - r0, kMaxGridYZ);
    BackwardArgs b = a;
    b.q += r0 * a.q_stride;
    b.k += r0 * a.k_stride;
    b.v += r0 * a.v_stride;
    b.out += r0 * a.out_stride;
    b.dout += r0 * a.dout_stride;
    b.lse += r0 * a.lse_stride;
    b.dterm += static_cast<int64_t>(r0) * a.m;
    if (b.dq != nullptr) b.dq += r0 * a.dq_stride;
    if (b.dk != nullptr) b.dk += r0 * a.dk_stride;
    if (b.dv != nullptr) b.dv += r0 * a.dv_stride;
    kernel(dim3(ceil_div(rows, kRowsPerBlock), ry), b, drop, r0, stream);
    const int st = launch_status();
    if (st != 0) return st;
  }
  return 0;
}

template <int D>
void launch_rows_kernel(dim3 grid, const BackwardArgs& b, const DropArgs* dr, int r0, hipStream_t s) {
  if (dr != nullptr) {
    DropArgs dd = *dr;
    dd.replica0 = r0;
    hipLaunchKernelGGL((attention_backward_rows_kernel<D, DropArgs>), grid, dim3(kThreads), 0, s,
                       b, dd);
  } else {
    hipLaunchKernelGGL((attention_backward_rows_kernel<D>), grid, dim3(kThreads), 0, s, b);
  }
}

template <int D>
void launch_columns_kernel(dim3 grid, const BackwardArgs& b, const DropArgs* dr, int r0,
                           hipStream_t s) {
  if (dr != nullptr) {
    DropArgs dd = *dr;
    dd.replica0 = r0;
    hipLaunchKernelGGL((attention_backward_columns_kernel<D, DropArgs>), grid, dim3(kThreads), 0,
                       s, b, dd);
  } else {
    hipLaunchKernelGGL((attention_backward_columns_kernel<D>), grid, dim3(kThreads), 0, s, b);
  }
}

}  // namespace
}  // namespace sputnik_hip

using namespace sputnik_hip;

extern "C" {

int sputnik_hip_sparse_attention_backward_supported(int m, int n, int d, int nonzeros) {
  return supported(m, n, d, nonzeros) ? 1 : 0;
}

size_t sputnik_hip_sparse_attention_backward_workspace_bytes(int m, int n, int d, int nonzeros,
                                                             int replicas) {
  if (!supported(m, n, d, nonzeros) || replicas <= 0) return 0;
  return (sizeof(float) * static_cast<size_t>(replicas) * m + 15) / 16 * 16;
}

int sputnik_hip_sparse_attention_backward(
    int m, int n, int d, int nonzeros, int replicas, const int* row_indices,
    const int* row_offsets, const int* column_indices, const int* t_row_indices,
    const int* t_row_offsets, const int* t_column_indices, const int* permutation,
    const float* q, int64_t q_stride, const float* k, int64_t k_stride, const float* v,
    int64_t v_stride, float scale, const float* out, int64_t out_stride, const float* grad_out,
    int64_t grad_out_stride, const float* lse, int64_t lse_stride, float* grad_q,
    int64_t grad_q_stride, float* grad_k, int64_t grad_k_stride, float* grad_v,
    int64_t grad_v_stride, double p, sputnik_hip_philox_state rng, void* workspace,
    size_t workspace_bytes, sputnik_hip_stream_t stream) {
  if (m < 0 || n < 0 || d < 0 || nonzeros < 0 || replicas < 0) return SPUTNIK_HIP_INVALID_ARGUMENT;
  DropArgs drop_store;
  if (!drop_args(p, rng, nullptr, &drop_store)) return SPUTNIK_HIP_INVALID_ARGUMENT;
  const DropArgs* drop = p > 0.0 ? &drop_store : nullptr;
  if (replicas == 0 || (grad_q == nullptr && grad_k == nullptr && grad_v == nullptr)) return 0;
  if (!supported(m, n, d, nonzeros)) return SPUTNIK_HIP_UNSUPPORTED;
  if (!operand_ok(q, q_stride) || !operand_ok(k, k_stride) || !operand_ok(v, v_stride) ||
      !operand_ok(out, out_stride) || !operand_ok(grad_out, grad_out_stride) ||
      !operand_ok(grad_q, grad_q_stride) || !operand_ok(grad_k, grad_k_stride) ||
      !operand_ok(grad_v, grad_v_stride) || lse_stride < 0)
    return SPUTNIK_HIP_UNSUPPORTED;
  if (nonzeros == 0) {   // every row is empty: zero gradients
    const std::pair<float*, int64_t> outs[3] = {{grad_q, grad_q_stride}, {grad_k, grad_k_stride},
                                                {grad_v, grad_v_stride}};
    for (int g = 0; g < 3; ++g) {
      if (outs[g].first == nullptr) continue;
      const int rows = g == 0 ? m : n;
      for (int r = 0; r < replicas; ++r) {
        const hipError_t e = hipMemsetAsync(outs[g].first + r * outs[g].second, 0,
                                            sizeof(float) * rows * d, stream);
        if (e != hipSuccess) return static_cast<int>(e);
      }
    }
    return 0;
  }
  if (q == nullptr || k == nullptr || v == nullptr || out == nullptr || grad_out == nullptr ||
      lse == nullptr || row_indices == nullptr || row_offsets == nullptr ||
      column_indices == nullptr)
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  const bool columns = grad_k != nullptr || grad_v != nullptr;
  if (columns && (t_row_indices == nullptr || t_row_offsets == nullptr ||
                  t_column_indices == nullptr || (drop != nullptr && permutation == nullptr)))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  if (workspace == nullptr || !aligned_to(workspace, 16) ||
      workspace_bytes <
          sputnik_hip_sparse_attention_backward_workspace_bytes(m, n, d, nonzeros, replicas))
    return SPUTNIK_HIP_INVALID_ARGUMENT;

  BackwardArgs a{};
  a.m = m;
  a.n = n;
  a.q = q; a.q_stride = q_stride;
  a.k = k; a.k_stride = k_stride;
  a.v = v; a.v_stride = v_stride;
  a.out = out; a.out_stride = out_stride;
  a.dout = grad_out; a.dout_stride = grad_out_stride;
  a.lse = lse; a.lse_stride = lse_stride;
  a.dterm = static_cast<float*>(workspace);
  a.scale = scale;

  auto launch_rows = [d](dim3 grid, const BackwardArgs& b, const DropArgs* dr, int r0,
                         hipStream_t s) {
    if (d == 64) launch_rows_kernel<64>(grid, b, dr, r0, s);
    else launch_rows_kernel<128>(grid, b, dr, r0, s);
  };
  auto launch_columns = [d](dim3 grid, const BackwardArgs& b, const DropArgs* dr, int r0,
                            hipStream_t s) {
    if (d == 64) launch_columns_kernel<64>(grid, b, dr, r0, s);
    else launch_columns_kernel<128>(grid, b, dr, r0, s);
  };

  // 1. D (always: the columns launch reads it) and dQ
  BackwardArgs rows = a;
  rows.row_indices = row_indices;
  rows.row_offsets = row_offsets;
  rows.column_indices = column_indices;
  rows.dq = grad_q; rows.dq_stride = grad_q_stride;
  int st = launch_replicas(launch_rows, m, replicas, rows, drop, stream);
  if (st != 0 || !columns) return st;
  // 2. dK, dV over the transposed mask
  BackwardArgs cols = a;
  cols.row_indices = t_row_indices;
  cols.row_offsets = t_row_offsets;
  cols.column_indices = t_column_indices;
  cols.permutation = permutation;
  cols.dk = grad_k; cols.dk_stride = grad_k_stride;
  cols.dv = grad_v; cols.dv_stride = grad_v_stride;
  return launch_replicas(launch_columns, n, replicas, cols, drop, stream);
}

}  // extern "C"
