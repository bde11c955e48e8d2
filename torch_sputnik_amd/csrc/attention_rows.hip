// Fused sparse attention forward in the row-group form, for gfx950:
//
//   out[i, :] = sum_j softmax_j(scale * <q_i, k_j>) * v_j      lse[i] = log sum_j exp(scale * <q_i, k_j>)
//
// j over the stored columns of mask row i -- what attention.hip computes at head dimension 64,
// here at head dimension 128, where two LDS stages of K and V rows (256 KiB) do not fit a CU.
// One 16-lane row group per query row (in row_indices order: rows of like length side by
// side), 16 rows per workgroup, replicas on grid y.  The group keeps its q row (times the
// scale), the running maximum, the running sum and the unnormalised output row in registers
// (online softmax, float32) and walks the row's entries in windows of 16: K and V rows are
// gathered from L2 (two float4 per lane and row, each load instruction 256 contiguous bytes),
// kUnroll entries in flight together, the scores reduced over the group by DPP.  The
// accumulators are rescaled once per unrolled step.  No LDS, no atomics; the order of a row's
// columns does not matter, and a row without entries reads none.
//
// Attention dropout (philox.h): entry e is the CSR position, lane u decides
// entry u of a window (keep_window); the row sum and lse take every entry, a dropped entry's
// weight into V is 0, and the keep scale is applied with 1 / l at the end.
#include <math.h>

#include "attention_rowgroup.h"

namespace sputnik_hip {
namespace {

using namespace rowgroup;

constexpr int kUnroll = 4;   // entries whose gathers are issued together

// Pointers and strides of one launch (replica 0 of the launch at the bases).
struct ForwardArgs {
  int m;
  const int* row_indices;
  const int* row_offsets;
  const int* column_indices;
  const float* q; int64_t q_stride;
  const float* k; int64_t k_stride;
  const float* v; int64_t v_stride;
  float* out; int64_t out_stride;
  float* lse; int64_t lse_stride;   // may be NULL
  float scale;
};

template <int D, typename... Drop>
__global__ __launch_bounds__(kThreads) void attention_rows_forward_kernel(ForwardArgs a,
                                                                          Drop... drop_arg) {
  constexpr bool DROP = sizeof...(Drop) > 0;
  const DropArgs drop = drop_of(drop_arg...);
  PhiloxKey key{};
  if constexpr (DROP)
    key = philox_key(drop, blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0);
  const int slot = blockIdx.x * kRowsPerBlock + threadIdx.x / kGroup;
  if (slot >= a.m) return;   // (the whole row group: the DPP reductions stay inside it)
  const int i = threadIdx.x % kGroup;
  const int replica = blockIdx.y;
  const int drop_r = replica + drop.replica0;
  const int row = a.row_indices[slot];
  const unsigned own = static_cast<unsigned>(row) * D + 4 * i;
  const float* __restrict__ k = a.k + replica * a.k_stride;
  const float* __restrict__ v = a.v + replica * a.v_stride;
  const Frag<D> qs = scaled(load_frag<D>(a.q + replica * a.q_stride, own), a.scale);
  const int p0 = a.row_offsets[row], p1 = a.row_offsets[row + 1];
  float mx = -INFINITY, l = 0.f;
  Frag<D> acc = zero_frag<D>();

  // The row's maximum moves to m_new: the sum and the accumulators follow (mx = -inf gives 0).
  auto rescale = [&](float m_new) {
    const float alpha = __expf(mx - m_new);
    l *= alpha;
    acc = scaled(acc, alpha);
    mx = m_new;
  };
  auto add = [&](bool kept, float s, const Frag<D>& vf) {
    const float e = __expf(s - mx);
    l += e;
    float ek = e;
    if constexpr (DROP) ek = kept ? e : 0.f;
    fma(acc, ek, vf);
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
      float s[kUnroll];
      float m_new = mx;
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        s[u] = group_sum<kGroup>(dot(qs, kf[u]));
        m_new = fmaxf(m_new, s[u]);
      }
      rescale(m_new);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) add((bits >> (p + u - w)) & 1u, s[u], vf[u]);
    }
    for (; p < end; ++p) {
      const unsigned col = static_cast<unsigned>(a.column_indices[p]) * D + 4 * i;
      const Frag<D> kf = load_frag<D>(k, col);
      const Frag<D> vf = load_frag<D>(v, col);
      const float s = group_sum<kGroup>(dot(qs, kf));
      rescale(fmaxf(mx, s));
      add((bits >> (p - w)) & 1u, s, vf);
    }
  }

  float inv = l > 0.f ? 1.f / l : 0.f;   // rows without entries give zeros
  if constexpr (DROP) inv *= drop.scale;
  store_frag<D>(a.out + replica * a.out_stride, own, scaled(acc, inv));
  if (a.lse != nullptr && i == 0)
    a.lse[replica * a.lse_stride + row] = l > 0.f ? mx + __logf(l) : -INFINITY;
}

bool supported(int m, int n, int d, int nonzeros) {
  return d == 128 && m > 0 && n > 0 && nonzeros > 0 && rows_fit_32_bits(m, d) &&
         rows_fit_32_bits(n, d);
}

}  // namespace
}  // namespace sputnik_hip

using namespace sputnik_hip;

extern "C" {

int sputnik_hip_sparse_attention_rows_supported(int m, int n, int d, int nonzeros) {
  return supported(m, n, d, nonzeros) ? 1 : 0;
}

int sputnik_hip_sparse_attention_rows_forward(
    int m, int n, int d, int nonzeros, int replicas, const int* row_indices,
    const int* row_offsets, const int* column_indices, const float* q, int64_t q_stride,
    const float* k, int64_t k_stride, const float* v, int64_t v_stride, float scale, float* out,
    int64_t out_stride, float* lse, int64_t lse_stride, double p, sputnik_hip_philox_state rng,
    int64_t* rng_state_out, sputnik_hip_stream_t stream) {
  if (m < 0 || n < 0 || d < 0 || nonzeros < 0 || replicas < 0) return SPUTNIK_HIP_INVALID_ARGUMENT;
  DropArgs drop_store;
  if (!drop_args(p, rng, rng_state_out, &drop_store)) return SPUTNIK_HIP_INVALID_ARGUMENT;
  const DropArgs* drop = p > 0.0 ? &drop_store : nullptr;
  if (replicas == 0) return drop != nullptr ? publish_rng_state(*drop, stream) : 0;
  if (!supported(m, n, d, nonzeros)) return SPUTNIK_HIP_UNSUPPORTED;
  if (!operand_ok(q, q_stride) || !operand_ok(k, k_stride) || !operand_ok(v, v_stride) ||
      !operand_ok(out, out_stride) || lse_stride < 0)
    return SPUTNIK_HIP_UNSUPPORTED;
  if (q == nullptr || k == nullptr || v == nullptr || out == nullptr || row_indices == nullptr ||
      row_offsets == nullptr || column_indices == nullptr)
    return SPUTNIK_HIP_INVALID_ARGUMENT;

  // One launch per 65535 replicas, the bases moved to the launch's first replica; replica
  // numbers continue over the launches and the first publishes the rng state.
  for (int r0 = 0; r0 < replicas; r0 += kMaxGridYZ) {
    ForwardArgs a{};
    a.m = m;
    a.row_indices = row_indices;
    a.row_offsets = row_offsets;
    a.column_indices = column_indices;
    a.q = q + r0 * q_stride; a.q_stride = q_stride;
    a.k = k + r0 * k_stride; a.k_stride = k_stride;
    a.v = v + r0 * v_stride; a.v_stride = v_stride;
    a.out = out + r0 * out_stride; a.out_stride = out_stride;
    a.lse = lse != nullptr ? lse + r0 * lse_stride : nullptr; a.lse_stride = lse_stride;
    a.scale = scale;
    const dim3 grid(ceil_div(m, kRowsPerBlock), min(replicas - r0, kMaxGridYZ));
    if (drop != nullptr) {
      DropArgs dd = *drop;
      dd.replica0 = r0;
      if (r0 > 0) dd.rng_state_out = nullptr;
      hipLaunchKernelGGL((attention_rows_forward_kernel<128, DropArgs>), grid, dim3(kThreads), 0,
                         stream, a, dd);
    } else {
      hipLaunchKernelGGL((attention_rows_forward_kernel<128>), grid, dim3(kThreads), 0, stream, a);
    }
    const int st = launch_status();
    if (st != 0) return st;
  }
  return 0;
}

}  // extern "C"
