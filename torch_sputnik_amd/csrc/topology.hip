// CSR topologies from dense masks / matrices, built on the device for gfx950
// (include/sputnik_hip.h: sputnik_hip_dense_to_csr_*, sputnik_hip_csr_row_order).
//
// Replaces the torch loop of topology.dense_to_sparse_3d (per mask: != 0, to_sparse_csr, two
// casts, a stable argsort and a host read of the count) by a fixed number of launches for any
// number of masks:
//   count   one GROUP of lanes per row walks the row and counts the kept elements; the counts
//           land in row_offsets[mask][row + 1]
//   scan    one workgroup per mask: in-place inclusive scan of those counts = the offsets;
//           row_offsets[mask][0] = 0, nonzeros[mask] = the last one
//   bases   one workgroup: bases[mask] = entries of the masks in front (64 bit)
//   fill    the same walk as count; a kept element's slot is its row's offset + the kept
//           elements of the row in front of it (wave ballot + lane prefix count)
//   order   one workgroup per mask sorts the unique keys (length, row) in LDS
// An element is kept exactly when torch's `x != 0` says so, decided on the BITS: any bit set
// for integer / bool types, any bit but the sign for floating types (-0.0 goes, NaN, +-inf and
// denormals stay whatever the denormal mode of the float unit is).
//
// The walk: a lane loads 16 bytes = V elements (V = 16 / element bytes) and a group of
// 64 / rows_per_wave lanes covers group_lanes * V consecutive columns per step.  The 16-byte
// pieces are laid out from the row start's address ROUNDED DOWN to 16 bytes, so that every
// piece that lies inside the row is one aligned wide load whatever the row start is (odd n
// with a 1-byte type, a sliced view); the at most two pieces per row that stick out of it are
// read element by element, inside the row only.  Nothing outside [row start, row start + n)
// is ever read.
#include <limits.h>

#include "common.h"
#include "wave_utils.h"

namespace sputnik_hip {
namespace {

constexpr int kBuildBlock = 256;
constexpr int kBuildWaves = kBuildBlock / kWave;
constexpr int kLoadBytes = 16;
constexpr int kMaxRowsPerWave = 16;   // groups of 4 lanes
constexpr int kScanBlock = 1024;

// The host's launch decisions for count and fill: both entries launch what this returns,
// sputnik_hip_dense_to_csr_launch_shape reports it.
struct BuildShape {
  int status = 0;
  int rows_per_wave = 0, elements_per_lane = 0, rows_per_workgroup = 0;
  int blocks_per_mask = 0, grid = 0;
};
inline BuildShape build_shape(int masks, int m, int n, int element_bytes) {
  BuildShape s;
  if (masks < 0 || m < 0 || n < 0 ||
      (element_bytes != 1 && element_bytes != 2 && element_bytes != 4 && element_bytes != 8) ||
      static_cast<int64_t>(m) * n > INT_MAX) {   // (a mask's count must fit its int32 offsets)
    s.status = SPUTNIK_HIP_INVALID_ARGUMENT;
    return s;
  }
  s.elements_per_lane = kLoadBytes / element_bytes;
  // the most rows per wave whose group of lanes still covers a row in one step
  s.rows_per_wave = kMaxRowsPerWave;
  while (s.rows_per_wave > 1 && n > (kWave / s.rows_per_wave) * s.elements_per_lane) s.rows_per_wave /= 2;
  s.rows_per_workgroup = kBuildWaves * s.rows_per_wave;
  s.blocks_per_mask = static_cast<int>(ceil_div64(m, s.rows_per_workgroup));
  const int64_t grid = static_cast<int64_t>(s.blocks_per_mask) * masks;
  if (grid > INT_MAX) s.status = SPUTNIK_HIP_INVALID_ARGUMENT;
  s.grid = static_cast<int>(grid);
  return s;
}

template <typename U>
struct alignas(kLoadBytes) Piece {
  U e[kLoadBytes / sizeof(U)];
};

// FILL = false: row_offsets[mask][row + 1] = kept elements of the row.
// FILL = true:  the kept columns (and, VALUES, the kept elements) of the row go to
//               bases[mask] + row_offsets[mask][row] onwards, ascending.
template <typename U, bool FILL, bool VALUES>
__global__ __launch_bounds__(kBuildBlock) void topology_rows_kernel(
    int m, int n, int rows_per_wave, int blocks_per_mask, const U* __restrict__ dense,
    int64_t batch_stride, int64_t row_stride, U keep, int* __restrict__ row_offsets,
    const int64_t* __restrict__ bases, int* __restrict__ column_indices, U* __restrict__ values) {
  constexpr int V = kLoadBytes / sizeof(U);
  const int mask = blockIdx.x / blocks_per_mask;
  const int block = blockIdx.x % blocks_per_mask;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int group_lanes = kWave / rows_per_wave;
  const int group = lane / group_lanes, group_lane = lane % group_lanes;
  const int64_t row = (static_cast<int64_t>(block) * kBuildWaves + wave) * rows_per_wave + group;
  const bool live = row < m;
  const unsigned long long group_mask =
      (group_lanes == kWave ? ~0ull : (1ull << group_lanes) - 1ull) << (group * group_lanes);
  const unsigned long long below = group_mask & ((1ull << lane) - 1ull);   // my group's lanes in front of me

  const U* __restrict__ src = dense + (live ? mask * batch_stride + row * row_stride : int64_t{0});
  // elements between the 16-byte boundary at or in front of the row start and the row start
  const int lead = live ? static_cast<int>((reinterpret_cast<uintptr_t>(src) % kLoadBytes) / sizeof(U)) : 0;
  const bool any_lead = __ballot(lead != 0) != 0ull;
  const int64_t span = static_cast<int64_t>(group_lanes) * V;
  const int steps = static_cast<int>((static_cast<int64_t>(n) + (any_lead ? V - 1 : 0) + span - 1) / span);

  int64_t out = 0;
  if constexpr (FILL) {
    if (live) out = bases[mask] + row_offsets[mask * (int64_t{1} + m) + row];
  }
  int count = 0;
  for (int s = 0; s < steps; ++s) {
    const int64_t c0 = (static_cast<int64_t>(s) * group_lanes + group_lane) * V - lead;   // my piece's first column
    Piece<U> v;
    if (live && c0 >= 0 && c0 + V <= n) {
      v = *reinterpret_cast<const Piece<U>*>(src + c0);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) v.e[e] = live && c0 + e >= 0 && c0 + e < n ? src[c0 + e] : U{0};
    }
    unsigned flags = 0;
#pragma unroll
    for (int e = 0; e < V; ++e) flags |= ((v.e[e] & keep) != 0 ? 1u : 0u) << e;
    if constexpr (!FILL) {
      count += __popc(flags);
    } else {
      // the kept elements of the step in column order: lane after lane, element after element
      // inside a lane.  One ballot per element slot = per 64 elements of the step.
      int before = 0, total = 0;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const unsigned long long b = __ballot((flags >> e) & 1u);
        before += __popcll(b & below);
        total += __popcll(b & group_mask);
      }
      int64_t p = out + before;
#pragma unroll
      for (int e = 0; e < V; ++e)
        if ((flags >> e) & 1u) {
          column_indices[p] = static_cast<int>(c0 + e);
          if constexpr (VALUES) values[p] = v.e[e];
          ++p;
        }
      out += total;
    }
  }
  if constexpr (!FILL) {
    for (int o = group_lanes / 2; o > 0; o >>= 1) count += __shfl_xor(count, o, kWave);
    if (live && group_lane == 0) row_offsets[mask * (int64_t{1} + m) + row + 1] = count;
  }
}

// Exclusive scan of one value per thread over a workgroup of kScanBlock threads; *total = the sum.
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T value, T* __restrict__ wave_sums, T* total) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  T incl = value;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const T up = __shfl_up(incl, off, kWave);
    if (lane >= off) incl += up;
  }
  if (lane == kWave - 1) wave_sums[wave] = incl;
  __syncthreads();
  T before = 0, all = 0;
  for (int w = 0; w < kScanBlock / kWave; ++w) {
    if (w < wave) before += wave_sums[w];
    all += wave_sums[w];
  }
  *total = all;
  return before + incl - value;
}

// row_offsets[mask][1 .. m] hold the rows' counts: scanned in place into the offsets.
__global__ __launch_bounds__(kScanBlock) void topology_scan_kernel(int m, int* __restrict__ row_offsets,
                                                                   int* __restrict__ nonzeros) {
  __shared__ int wave_sums[kScanBlock / kWave];
  int* __restrict__ offsets = row_offsets + blockIdx.x * (int64_t{1} + m);
  const int t = threadIdx.x;
  const int64_t per = (static_cast<int64_t>(m) + kScanBlock - 1) / kScanBlock;
  const int64_t i0 = min(static_cast<int64_t>(m), t * per), i1 = min(static_cast<int64_t>(m), i0 + per);
  int mine = 0;
  for (int64_t i = i0; i < i1; ++i) mine += offsets[1 + i];
  int total;
  int running = block_exclusive_scan(mine, wave_sums, &total);
  for (int64_t i = i0; i < i1; ++i) {
    running += offsets[1 + i];
    offsets[1 + i] = running;
  }
  if (t == 0) {
    offsets[0] = 0;
    nonzeros[blockIdx.x] = total;
  }
}

// bases[mask] = sum of nonzeros[0 .. mask)
__global__ __launch_bounds__(kScanBlock) void topology_bases_kernel(int masks, const int* __restrict__ nonzeros,
                                                                    int64_t* __restrict__ bases) {
  __shared__ int64_t wave_sums[kScanBlock / kWave];
  const int t = threadIdx.x;
  const int per = (masks + kScanBlock - 1) / kScanBlock;
  const int i0 = min(masks, t * per), i1 = min(masks, i0 + per);
  int64_t mine = 0;
  for (int i = i0; i < i1; ++i) mine += nonzeros[i];
  int64_t total;
  int64_t running = block_exclusive_scan(mine, wave_sums, &total);
  for (int i = i0; i < i1; ++i) {
    bases[i] = running;
    running += nonzeros[i];
  }
}

// ---------------------------------------------------------------------------
// Row order: the rows of a mask by ascending length, ties by ascending row
// (torch.argsort(lengths, stable=True)).  The keys (length, row) are unique, so any sort of
// them is the stable order: a bitonic network over the next power of two in LDS, one
// workgroup per mask, one launch, nothing on the host depends on the data.  64-bit keys --
// the length (as torch orders int32: signed) above the row -- hold every int32 length, so no
// n is too wide; the padding keys are all ones and sort behind every row.
// ---------------------------------------------------------------------------
constexpr int kOrderSmallRows = 2048, kOrderSmallBlock = 256;     // 16 KiB of keys
constexpr int kOrderLargeRows = 16384, kOrderLargeBlock = 1024;   // 128 KiB of keys (of the CU's 160)

struct OrderRoute {
  int status = 0;
  int served = 0;
  int capacity = -1, threads = -1, sort_size = -1;
};
inline OrderRoute order_route(int masks, int m, int n) {
  OrderRoute r;
  if (masks < 0 || m < 0 || n < 0) {
    r.status = SPUTNIK_HIP_INVALID_ARGUMENT;
    return r;
  }
  if (m > kOrderLargeRows) return r;
  r.served = 1;
  r.capacity = m <= kOrderSmallRows ? kOrderSmallRows : kOrderLargeRows;
  r.threads = m <= kOrderSmallRows ? kOrderSmallBlock : kOrderLargeBlock;
  r.sort_size = 1;
  while (r.sort_size < m) r.sort_size *= 2;
  return r;
}

template <int CAPACITY, int THREADS>
__global__ __launch_bounds__(THREADS) void topology_row_order_kernel(
    int m, int sort_size, const int* __restrict__ row_offsets, int* __restrict__ row_indices) {
  __shared__ unsigned long long keys[CAPACITY];
  const int* __restrict__ offsets = row_offsets + static_cast<int64_t>(blockIdx.x) * (m + 1);
  int* __restrict__ out = row_indices + static_cast<int64_t>(blockIdx.x) * m;
  const int t = threadIdx.x;
  for (int i = t; i < sort_size; i += THREADS) {
    unsigned long long key = ~0ull;
    if (i < m) {
      const unsigned length = static_cast<unsigned>(offsets[i + 1]) - static_cast<unsigned>(offsets[i]);
      key = (static_cast<unsigned long long>(length ^ 0x80000000u) << 32) | static_cast<unsigned>(i);
    }
    keys[i] = key;
  }
  __syncthreads();
  for (int k = 2; k <= sort_size; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = t; p < sort_size / 2; p += THREADS) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const int l = i | j;
        const unsigned long long a = keys[i], b = keys[l];
        if ((a > b) == ((i & k) == 0)) {
          keys[i] = b;
          keys[l] = a;
        }
      }
      __syncthreads();
    }
  for (int i = t; i < m; i += THREADS) out[i] = static_cast<int>(static_cast<unsigned>(keys[i]));
}

template <typename U, bool FILL, bool VALUES>
int launch_rows(const BuildShape& s, int m, int n, const void* dense, int floating, int64_t batch_stride,
                int64_t row_stride, int* row_offsets, const int64_t* bases, int* column_indices,
                void* values, hipStream_t stream) {
  const U all = static_cast<U>(~U{0});
  const U keep = floating ? static_cast<U>(all >> 1) : all;   // (everything but the sign bit)
  hipLaunchKernelGGL((topology_rows_kernel<U, FILL, VALUES>), dim3(s.grid), dim3(kBuildBlock), 0, stream,
                     m, n, s.rows_per_wave, s.blocks_per_mask, static_cast<const U*>(dense), batch_stride,
                     row_stride, keep, row_offsets, bases, column_indices, static_cast<U*>(values));
  return launch_status();
}

template <bool FILL>
int launch_rows_typed(const BuildShape& s, int m, int n, const void* dense, int element_bytes, int floating,
                      int64_t batch_stride, int64_t row_stride, int* row_offsets, const int64_t* bases,
                      int* column_indices, void* values, hipStream_t stream) {
#define SPUTNIK_TOPOLOGY_ROWS(U)                                                                         \
  return FILL && values != nullptr                                                                       \
             ? launch_rows<U, FILL, FILL>(s, m, n, dense, floating, batch_stride, row_stride,            \
                                          row_offsets, bases, column_indices, values, stream)            \
             : launch_rows<U, FILL, false>(s, m, n, dense, floating, batch_stride, row_stride,           \
                                           row_offsets, bases, column_indices, values, stream)
  switch (element_bytes) {
    case 1: SPUTNIK_TOPOLOGY_ROWS(uint8_t);
    case 2: SPUTNIK_TOPOLOGY_ROWS(uint16_t);
    case 4: SPUTNIK_TOPOLOGY_ROWS(uint32_t);
    default: SPUTNIK_TOPOLOGY_ROWS(uint64_t);
  }
#undef SPUTNIK_TOPOLOGY_ROWS
}

inline bool dense_ok(const void* dense, int element_bytes, int64_t batch_stride, int64_t row_stride) {
  return dense != nullptr && aligned_to(dense, element_bytes) && batch_stride >= 0 && row_stride >= 0;
}

}  // namespace
}  // namespace sputnik_hip

using namespace sputnik_hip;

extern "C" {

int sputnik_hip_dense_to_csr_launch_shape(int masks, int m, int n, int element_bytes, int* rows_per_wave,
                                          int* elements_per_lane, int* rows_per_workgroup, int* grid) {
  const BuildShape s = build_shape(masks, m, n, element_bytes);
  if (s.status != 0) return s.status;
  if (rows_per_wave) *rows_per_wave = s.rows_per_wave;
  if (elements_per_lane) *elements_per_lane = s.elements_per_lane;
  if (rows_per_workgroup) *rows_per_workgroup = s.rows_per_workgroup;
  if (grid) *grid = s.grid;
  return 0;
}

int sputnik_hip_dense_to_csr_count(int masks, int m, int n, const void* dense, int element_bytes,
                                   int floating, int64_t batch_stride, int64_t row_stride,
                                   int* row_offsets, int* nonzeros, int64_t* bases,
                                   sputnik_hip_stream_t stream_) {
  const BuildShape s = build_shape(masks, m, n, element_bytes);
  if (s.status != 0) return s.status;
  if (masks == 0) return 0;
  if (row_offsets == nullptr || nonzeros == nullptr || bases == nullptr ||
      (s.grid > 0 && n > 0 && !dense_ok(dense, element_bytes, batch_stride, row_stride)))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (s.grid > 0) {
    const int st = launch_rows_typed<false>(s, m, n, dense, element_bytes, floating, batch_stride, row_stride,
                                            row_offsets, nullptr, nullptr, nullptr, stream);
    if (st != 0) return st;
  }
  hipLaunchKernelGGL(topology_scan_kernel, dim3(masks), dim3(kScanBlock), 0, stream, m, row_offsets, nonzeros);
  hipLaunchKernelGGL(topology_bases_kernel, dim3(1), dim3(kScanBlock), 0, stream, masks, nonzeros, bases);
  return launch_status();
}

int sputnik_hip_dense_to_csr_fill(int masks, int m, int n, const void* dense, int element_bytes,
                                  int floating, int64_t batch_stride, int64_t row_stride,
                                  const int* row_offsets, const int64_t* bases, int* column_indices,
                                  void* values, sputnik_hip_stream_t stream_) {
  const BuildShape s = build_shape(masks, m, n, element_bytes);
  if (s.status != 0) return s.status;
  if (s.grid == 0 || n == 0) return 0;
  if (row_offsets == nullptr || bases == nullptr || column_indices == nullptr ||
      !dense_ok(dense, element_bytes, batch_stride, row_stride) ||
      (values != nullptr && !aligned_to(values, element_bytes)))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  return launch_rows_typed<true>(s, m, n, dense, element_bytes, floating, batch_stride, row_stride,
                                 const_cast<int*>(row_offsets), bases, column_indices, values,
                                 static_cast<hipStream_t>(stream_));
}

int sputnik_hip_csr_row_order_route(int masks, int m, int n, int* served, int* capacity, int* threads,
                                    int* sort_size) {
  const OrderRoute r = order_route(masks, m, n);
  if (r.status != 0) return r.status;
  if (served) *served = r.served;
  if (capacity) *capacity = r.capacity;
  if (threads) *threads = r.threads;
  if (sort_size) *sort_size = r.sort_size;
  return 0;
}

int sputnik_hip_csr_row_order(int masks, int m, int n, const int* row_offsets, int* row_indices,
                              sputnik_hip_stream_t stream_) {
  const OrderRoute r = order_route(masks, m, n);
  if (r.status != 0) return r.status;
  if (!r.served) return SPUTNIK_HIP_INVALID_ARGUMENT;
  if (masks == 0 || m == 0) return 0;
  if (row_offsets == nullptr || row_indices == nullptr) return SPUTNIK_HIP_INVALID_ARGUMENT;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (r.capacity == kOrderSmallRows)
    hipLaunchKernelGGL((topology_row_order_kernel<kOrderSmallRows, kOrderSmallBlock>), dim3(masks),
                       dim3(kOrderSmallBlock), 0, stream, m, r.sort_size, row_offsets, row_indices);
  else
    hipLaunchKernelGGL((topology_row_order_kernel<kOrderLargeRows, kOrderLargeBlock>), dim3(masks),
                       dim3(kOrderLargeBlock), 0, stream, m, r.sort_size, row_offsets, row_indices);
  return launch_status();
}

}  // extern "C"
