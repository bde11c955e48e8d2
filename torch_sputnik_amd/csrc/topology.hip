// CSR topologies from dense masks / matrices, built on the device for gfx950
// (include/sputnik_hip.h: sputnik_hip_dense_to_csr_*, sputnik_hip_csr_row_order), and the
// selections that write one out: sputnik_hip_topk_to_csr, sputnik_hip_csr_regrow, sputnik_hip_csr_topk,
// sputnik_hip_csr_topk_global_*, sputnik_hip_csr_regrow_total, sputnik_hip_random_csr,
// sputnik_hip_csr_regrow_random, sputnik_hip_csr_regrow_total_random; and the attention patterns
// that are built from a rule with no dense mask at all (sputnik_hip_attention_pattern_*).
//
// The build replaces the torch loop of topology.dense_to_sparse_3d (per mask: != 0,
// to_sparse_csr, two casts, a stable argsort and a host read of the count) by a fixed number of
// launches for any number of masks:
//   count   one GROUP of lanes per row walks the row and counts the kept elements; the counts
//           land in row_offsets[mask][row + 1]
//   scan    one workgroup per mask: in-place inclusive scan of those counts = the offsets;
//           row_offsets[mask][0] = 0, nonzeros[mask] = the last one
//   bases   one workgroup: bases[mask] = entries of the masks in front (64 bit)
//   fill    the same walk as count; a kept element's slot is its row's offset + the kept
//           elements of the row in front of it
//   order   one workgroup per mask sorts the unique keys (length, row) in LDS
// An element is kept exactly when torch's `x != 0` says so, decided on the BITS: any bit set
// for integer / bool types, any bit but the sign for floating types (-0.0 goes, NaN, +-inf and
// denormals stay whatever the denormal mode of the float unit is).
//
// The build and every selection are made of the same parts, each written once:
//   RowGroup       the lanes of a wave that share a row: 64 / rows_per_wave of them, their mask
//                  in the wave's ballots, a lane's share of the row's 256 bins
//   load_piece     a lane loads 16 bytes = V elements (V = 16 / element bytes).  The pieces are
//                  laid out from the array start's address ROUNDED DOWN to 16 bytes, so that
//                  every piece that lies inside the array is one aligned wide load whatever the
//                  start is (odd n with a 1-byte type, a sliced view); the at most two pieces
//                  that stick out of it are read element by element, inside the array only.
//                  Nothing outside [start, start + n) is ever read.
//   RowWalk        a group covers group_lanes * V consecutive columns per step; made over a
//                  dense row (the constructor) or over the entries of a CSR row (entry_walk)
//   KeyWalk        the same walk over keys that are computed, not loaded (a random topology)
//   radix_select   the need-th largest key of a group's row, MSB first, 8-bit digits, a 256-bin
//                  histogram per row in LDS filled by the caller's step (count_digit per key)
//   group_prefix   the flagged elements of a step in front of a lane's piece and in the whole
//                  step: one wave ballot per element slot and a lane-prefix count
//   admit_ties     the first `quota` elements equal to the threshold join the flags, the tie
//                  count is carried across the steps of the row
//   thread_span, inclusive_scan_span   a 1024-thread workgroup's scan over any number of items
#include <limits.h>

#include <type_traits>

#include "common.h"
#include "philox.h"
#include "wave_utils.h"

namespace sputnik_hip {
namespace {

constexpr int kBuildBlock = 256;
constexpr int kBuildWaves = kBuildBlock / kWave;
constexpr int kLoadBytes = 16;
constexpr int kMaxRowsPerWave = 16;   // groups of 4 lanes
constexpr int kScanBlock = 1024;
constexpr int kDigitBits = 8;
constexpr int kDigitBins = 1 << kDigitBits;
constexpr int kMaxDigitPasses = 4;
constexpr unsigned kNoThreshold = 0xffffffffu;   // above every key: nothing is kept by it
static_assert(kDigitBins == kBuildBlock, "one thread per bin when a workgroup merges its histogram");

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

// ---------------------------------------------------------------------------
// The shared parts.
// ---------------------------------------------------------------------------
// The group of lanes of one row: workgroup `block` of a matrix serves the rows from
// block * kBuildWaves * rows_per_wave, one per group, wave after wave.
struct RowGroup {
  int lane, wave, group_lanes, group, group_lane;
  int slot;   // the group's place in the workgroup
  int64_t row;
  unsigned long long group_mask, below;   // my group's lanes in a ballot; those of them in front of me

  __device__ __forceinline__ explicit RowGroup(int rows_per_wave, int block = blockIdx.x) {
    lane = threadIdx.x % kWave;
    wave = threadIdx.x / kWave;
    group_lanes = kWave / rows_per_wave;
    group = lane / group_lanes;
    group_lane = lane % group_lanes;
    slot = wave * rows_per_wave + group;
    row = (static_cast<int64_t>(block) * kBuildWaves + wave) * rows_per_wave + group;
    group_mask = (group_lanes == kWave ? ~0ull : (1ull << group_lanes) - 1ull) << (group * group_lanes);
    below = group_mask & ((1ull << lane) - 1ull);
  }
  // A lane owns the `chunk` consecutive bins from `base` of its row's 256: 4 .. 256 of them.
  __device__ __forceinline__ int chunk() const { return kDigitBins / group_lanes; }
  __device__ __forceinline__ int base() const { return group_lane * chunk(); }
};

template <typename U>
struct alignas(kLoadBytes) Piece {
  U e[kLoadBytes / sizeof(U)];
};

// The 16-byte piece whose first element is src[c0], of an array of n elements: one wide load
// where it lies inside the array, else element by element, inside the array only.  *valid: a
// bit per element that lies inside the array (the others read as 0 and are not loaded).  A lane
// for which the array is not `there` loads nothing.
template <typename U>
__device__ __forceinline__ Piece<U> load_piece(const U* __restrict__ src, int64_t c0, int64_t n, unsigned* valid,
                                               bool there = true) {
  constexpr int V = kLoadBytes / sizeof(U);
  Piece<U> v;
  if (there && c0 >= 0 && c0 + V <= n) {
    v = *reinterpret_cast<const Piece<U>*>(src + c0);
    *valid = (1u << V) - 1u;
  } else {
    unsigned in = 0;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const bool inside = there && c0 + e >= 0 && c0 + e < n;
      v.e[e] = inside ? src[c0 + e] : U{0};
      in |= (inside ? 1u : 0u) << e;
    }
    *valid = in;
  }
  return v;
}

// One group of lanes on one row of n elements from src.  A group without a row (live = false)
// takes the steps and loads nothing.
template <typename U>
struct RowWalk {
  using Element = U;
  static constexpr int V = kLoadBytes / sizeof(U);
  const U* src;
  bool live;
  int n, lead, steps, group_lanes, group_lane;

  __device__ __forceinline__ RowWalk() {}   // (entry_walk)
  // Row g.row of a dense [m, n] matrix.  Every row of the wave takes the same steps: one more
  // piece per row where any of them starts off a 16-byte boundary.
  __device__ __forceinline__ RowWalk(const RowGroup& g, const U* dense, int64_t row_stride, int m, int n_) {
    group_lanes = g.group_lanes;
    group_lane = g.group_lane;
    live = g.row < m;
    n = n_;
    src = dense + (live ? g.row * row_stride : int64_t{0});
    // elements between the 16-byte boundary at or in front of the row start and the row start
    lead = live ? static_cast<int>((reinterpret_cast<uintptr_t>(src) % kLoadBytes) / sizeof(U)) : 0;
    const bool any_lead = __ballot(lead != 0) != 0ull;
    const int64_t span = static_cast<int64_t>(group_lanes) * V;
    steps = static_cast<int>((static_cast<int64_t>(n_) + (any_lead ? V - 1 : 0) + span - 1) / span);
  }
  // My piece of step s, its first column, and a bit per element that lies inside the row.
  __device__ __forceinline__ Piece<U> load(int s, int64_t* first_column, unsigned* valid) const {
    const int64_t c0 = (static_cast<int64_t>(s) * group_lanes + group_lane) * V - lead;
    *first_column = c0;
    return load_piece(src, c0, static_cast<int64_t>(n), valid, live);
  }
};

// The slots [begin, end) of a row's entries, inside [0, nonzeros) whatever the offsets say.
__device__ __forceinline__ void row_slots(const int* __restrict__ row_offsets, int64_t row, bool live, int nonzeros,
                                          int* begin, int* end) {
  *begin = 0;
  *end = 0;
  if (live) {
    *begin = min(max(row_offsets[row], 0), nonzeros);
    *end = min(max(row_offsets[row + 1], *begin), nonzeros);
  }
}

// The walk of a group over the entries [begin, end) of its CSR row, like a dense row:
// values + begin is the row start.  Every lane of the wave takes as many steps as the wave's
// longest row needs (the ballots of a fill are the wave's).
template <typename U>
__device__ __forceinline__ RowWalk<U> entry_walk(const RowGroup& g, const U* __restrict__ values, int begin, int end,
                                                 bool live) {
  constexpr int V = kLoadBytes / sizeof(U);
  RowWalk<U> w;
  w.n = end - begin;
  w.group_lanes = g.group_lanes;
  w.group_lane = g.group_lane;
  w.live = live;
  w.src = values + begin;
  w.lead = static_cast<int>((reinterpret_cast<uintptr_t>(w.src) % kLoadBytes) / sizeof(U));
  const int64_t span = static_cast<int64_t>(w.group_lanes) * V;
  int steps = static_cast<int>((static_cast<int64_t>(w.n) + w.lead + span - 1) / span);
  for (int o = kWave / 2; o > 0; o >>= 1) steps = max(steps, __shfl_xor(steps, o, kWave));
  w.steps = steps;
  return w;
}

// An element's KEY: its bit pattern without the sign bit, read as an unsigned integer.
template <typename U>
__device__ __forceinline__ unsigned key_of(U bits) {
  return static_cast<unsigned>(bits & static_cast<U>(static_cast<U>(~U{0}) >> 1));
}

// A bit per element of the piece whose key (at most key_limit) is above / equal to the threshold.
template <typename U>
__device__ __forceinline__ void compare_piece(const Piece<U>& v, unsigned threshold, unsigned key_limit,
                                              unsigned* greater, unsigned* equal) {
  unsigned above = 0, same = 0;
#pragma unroll
  for (int e = 0; e < static_cast<int>(kLoadBytes / sizeof(U)); ++e) {
    const unsigned key = min(key_of(v.e[e]), key_limit);
    above |= (key > threshold ? 1u : 0u) << e;
    same |= (key == threshold ? 1u : 0u) << e;
  }
  *greater = above;
  *equal = same;
}

// One key into the histogram of digit `shift / 8`, if it is counted and its higher digits
// equal `prefix`.
__device__ __forceinline__ void count_digit(unsigned key, bool counted, int shift, unsigned prefix,
                                            unsigned* __restrict__ bins) {
  // (64 bit: the first pass shifts everything out and compares with prefix 0)
  if (counted && static_cast<unsigned>(static_cast<uint64_t>(key) >> (shift + kDigitBits)) == prefix)
    atomicAdd(&bins[(key >> shift) & (kDigitBins - 1)], 1u);
}

// Histogram of digit `shift / 8` of the row's keys (at most key_limit) whose higher digits equal
// `prefix`; open(first column) = a bit per element of the piece that takes part.  Walk: a
// RowWalk over memory, or a KeyWalk over generated keys.
template <typename Walk, typename Open>
__device__ __forceinline__ void digit_histogram(const Walk& walk, int shift, unsigned prefix,
                                                unsigned* __restrict__ bins, unsigned key_limit, Open open) {
  for (int s = 0; s < walk.steps; ++s) {
    int64_t c0;
    unsigned valid;
    const Piece<typename Walk::Element> v = walk.load(s, &c0, &valid);
    const unsigned counted = valid & open(c0);
#pragma unroll
    for (int e = 0; e < Walk::V; ++e)
      count_digit(min(key_of(v.e[e]), key_limit), (counted >> e) & 1u, shift, prefix, bins);
  }
}
template <typename Walk>
__device__ __forceinline__ void digit_histogram(const Walk& walk, int shift, unsigned prefix,
                                                unsigned* __restrict__ bins) {
  digit_histogram(walk, shift, prefix, bins, kNoThreshold, [](int64_t) { return ~0u; });
}

// One digit of a row's radix select, from the row's filled bins: the digit whose bin holds the
// need-th largest of the elements counted, to every lane of the group; *need becomes what is
// still to take inside that bin, or 0 where there is nothing to take (need = 0, no row here).
__device__ __forceinline__ unsigned pick_digit(const RowGroup& g, const unsigned* __restrict__ bins, int* need_io) {
  const int need = *need_io, base = g.base(), chunk = g.chunk();
  unsigned mine = 0;
  for (int j = 0; j < chunk; ++j) mine += bins[base + j];
  unsigned incl = mine;   // elements in my bins and in those of the group's lanes above me
  for (int off = 1; off < g.group_lanes; off <<= 1) {
    const unsigned up = __shfl_down(incl, off, kWave);
    if (g.group_lane + off < g.group_lanes) incl += up;
  }
  const unsigned above = incl - mine;
  // the lane whose bins hold the need-th largest element
  const bool owner = need > 0 && above < static_cast<unsigned>(need) && static_cast<unsigned>(need) <= above + mine;
  int digit = 0, left = 0;
  if (owner) {
    unsigned acc = above;
    for (int j = chunk - 1; j >= 0; --j) {
      const unsigned c = bins[base + j];
      if (acc + c >= static_cast<unsigned>(need)) {
        digit = base + j;
        left = need - static_cast<int>(acc);
        break;
      }
      acc += c;
    }
  }
  const unsigned long long who = __ballot(owner) & g.group_mask;
  const int from = who != 0ull ? __ffsll(who) - 1 : g.lane;
  digit = __shfl(digit, from, kWave);
  left = __shfl(left, from, kWave);
  *need_io = who != 0ull ? left : 0;   // (no owner: nothing to take, or no row here)
  return static_cast<unsigned>(digit);
}

// What a selection comes down to: an element is kept iff key > threshold, or key == threshold
// and it is among the first `quota` such elements of its row.
struct Selection {
  unsigned threshold;
  int quota;
};

// The `need` largest keys of the group's row by an MSB-first radix select over P digits in the
// row's 256 LDS bins.  histogram(shift, prefix, bins) counts digit `shift / 8` of the row's keys
// whose higher digits equal the prefix.  Every thread of the workgroup calls it: three barriers
// per digit.
template <int P, typename Histogram>
__device__ __forceinline__ Selection radix_select(const RowGroup& g, unsigned* __restrict__ bins, int need,
                                                  Histogram histogram) {
  const bool any = need > 0;
  const int base = g.base(), chunk = g.chunk();
  unsigned prefix = 0;   // (need: still to take among the elements whose higher digits equal it)
  for (int p = 0; p < P; ++p) {
    const int shift = kDigitBits * (P - 1 - p);
    for (int j = 0; j < chunk; ++j) bins[base + j] = 0u;
    __syncthreads();
    histogram(shift, prefix, bins);
    __syncthreads();
    prefix = (prefix << kDigitBits) | pick_digit(g, bins, &need);
    __syncthreads();   // (the bins are cleared again)
  }
  return {any ? prefix : kNoThreshold, need};
}

// Of the elements of a step whose bit is set in a lane's `flags` -- column order: lane after
// lane, element after element inside a lane -- those in front of my piece and those of the
// whole step.  One ballot per element slot = per 64 elements of the step.
struct Prefix {
  int before, total;
};
template <int V>
__device__ __forceinline__ Prefix group_prefix(const RowGroup& g, unsigned flags) {
  Prefix at = {0, 0};
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const unsigned long long b = __ballot((flags >> e) & 1u);
    at.before += __popcll(b & g.below);
    at.total += __popcll(b & g.group_mask);
  }
  return at;
}

// flags plus those elements of `equal` (the step's ties with the threshold) whose rank among
// the row's ties is below the quota; *ties_seen = the ties of the steps behind.
template <int V>
__device__ __forceinline__ unsigned admit_ties(const RowGroup& g, unsigned flags, unsigned equal, int quota,
                                               int* ties_seen) {
  const Prefix ties = group_prefix<V>(g, equal);
  int rank = *ties_seen + ties.before;
#pragma unroll
  for (int e = 0; e < V; ++e)
    if ((equal >> e) & 1u) {
      if (rank < quota) flags |= 1u << e;
      ++rank;
    }
  *ties_seen += ties.total;
  return flags;
}

// The items of thread threadIdx.x when a workgroup of kScanBlock threads shares `count` items
// in order.
struct Span {
  int64_t begin, end;
};
__device__ __forceinline__ Span thread_span(int64_t count) {
  const int64_t per = (count + kScanBlock - 1) / kScanBlock;
  const int64_t begin = min(count, threadIdx.x * per);
  return {begin, min(count, begin + per)};
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

// out[i] = count(0) + .. + count(i) over all items of the workgroup; `mine` = the sum of
// count over my span.  -> the sum over all items.  One barrier.
template <typename Count>
__device__ __forceinline__ int inclusive_scan_span(const Span& span, int mine, int* __restrict__ wave_sums,
                                                   int* out, Count count) {
  int total;
  int running = block_exclusive_scan(mine, wave_sums, &total);
  for (int64_t i = span.begin; i < span.end; ++i) {
    running += count(i);
    out[i] = running;
  }
  return total;
}

// ---------------------------------------------------------------------------
// The build.
// FILL = false: row_offsets[mask][row + 1] = kept elements of the row.
// FILL = true:  the kept columns (and, VALUES, the kept elements) of the row go to
//               bases[mask] + row_offsets[mask][row] onwards, ascending.
// ---------------------------------------------------------------------------
template <typename U, bool FILL, bool VALUES>
__global__ __launch_bounds__(kBuildBlock) void topology_rows_kernel(
    int m, int n, int rows_per_wave, int blocks_per_mask, const U* __restrict__ dense,
    int64_t batch_stride, int64_t row_stride, U keep, int* __restrict__ row_offsets,
    const int64_t* __restrict__ bases, int* __restrict__ column_indices, U* __restrict__ values) {
  constexpr int V = RowWalk<U>::V;
  const int mask = blockIdx.x / blocks_per_mask;
  const RowGroup g(rows_per_wave, blockIdx.x % blocks_per_mask);
  const RowWalk<U> walk(g, dense + mask * batch_stride, row_stride, m, n);

  int64_t out = 0;
  if constexpr (FILL) {
    if (walk.live) out = bases[mask] + row_offsets[mask * (int64_t{1} + m) + g.row];
  }
  int count = 0;
  for (int s = 0; s < walk.steps; ++s) {
    int64_t c0;
    unsigned valid;   // (an element outside the row reads 0: not kept)
    const Piece<U> v = walk.load(s, &c0, &valid);
    unsigned flags = 0;
#pragma unroll
    for (int e = 0; e < V; ++e) flags |= ((v.e[e] & keep) != 0 ? 1u : 0u) << e;
    if constexpr (!FILL) {
      count += __popc(flags);
    } else {
      const Prefix at = group_prefix<V>(g, flags);
      int64_t p = out + at.before;
#pragma unroll
      for (int e = 0; e < V; ++e)
        if ((flags >> e) & 1u) {
          column_indices[p] = static_cast<int>(c0 + e);
          if constexpr (VALUES) values[p] = v.e[e];
          ++p;
        }
      out += at.total;
    }
  }
  if constexpr (!FILL) {
    for (int o = g.group_lanes / 2; o > 0; o >>= 1) count += __shfl_xor(count, o, kWave);
    if (walk.live && g.group_lane == 0) row_offsets[mask * (int64_t{1} + m) + g.row + 1] = count;
  }
}

// row_offsets[mask][1 .. m] hold the rows' counts: scanned in place into the offsets.
__global__ __launch_bounds__(kScanBlock) void topology_scan_kernel(int m, int* __restrict__ row_offsets,
                                                                   int* __restrict__ nonzeros) {
  __shared__ int wave_sums[kScanBlock / kWave];
  int* __restrict__ offsets = row_offsets + blockIdx.x * (int64_t{1} + m);
  const Span span = thread_span(m);
  const auto count = [&](int64_t i) { return offsets[1 + i]; };
  int mine = 0;
  for (int64_t i = span.begin; i < span.end; ++i) mine += count(i);
  const int total = inclusive_scan_span(span, mine, wave_sums, offsets + 1, count);
  if (threadIdx.x == 0) {
    offsets[0] = 0;
    nonzeros[blockIdx.x] = total;
  }
}

// bases[mask] = sum of nonzeros[0 .. mask)
__global__ __launch_bounds__(kScanBlock) void topology_bases_kernel(int masks, const int* __restrict__ nonzeros,
                                                                    int64_t* __restrict__ bases) {
  __shared__ int64_t wave_sums[kScanBlock / kWave];
  const Span span = thread_span(masks);
  int64_t mine = 0;
  for (int64_t i = span.begin; i < span.end; ++i) mine += nonzeros[i];
  int64_t total;
  int64_t running = block_exclusive_scan(mine, wave_sums, &total);
  for (int64_t i = span.begin; i < span.end; ++i) {
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

// ---------------------------------------------------------------------------
// Attention patterns (sputnik_hip_attention_pattern_*): the build above over a mask that is
// never stored.  topology_rows_kernel with the load replaced by the predicate of
// include/sputnik_hip.h, "Attention patterns": a lane evaluates its V = 4 consecutive columns
// into a flag word, the count pass reduces popcounts, the fill pass places columns with
// group_prefix.  What depends on the row alone is computed once per row (PatternRow): the
// position p, the columns of the window and of the block, the last column a causal row may
// keep, whether the row is global, the row of random blocks.  The only memory read is the
// flag vector of the global tokens: four bytes per lane and step, one aligned load where the
// piece lies inside [0, n).  The random component draws one Philox call per distinct
// (C >> 2, R) a lane meets: the four words stay in registers across the columns of a piece and
// across steps.  All position arithmetic is 64 bit; the host hands over products that are
// already clamped (pattern_ok).
// ---------------------------------------------------------------------------
constexpr int kPatternV = 4;                              // columns per lane and step
constexpr int64_t kPatternReach = int64_t{1} << 33;       // beyond every |c - p|
constexpr int64_t kPatternMaxOffset = int64_t{1} << 30;   // |offset| below it
constexpr int kPatternLaunches = 4;                       // count, scan, fill, row order

struct PatternArgs {
  sputnik_hip_attention_pattern_args rule;
  DropArgs state;   // the Philox state of the random blocks and where it is published
};

struct PatternShape {
  int status = 0;
  int served = 0;
  BuildShape walk;
};
inline PatternShape pattern_shape(int m, int n, int64_t offset) {
  PatternShape s;
  if (m < 0 || n < 0) {
    s.status = SPUTNIK_HIP_INVALID_ARGUMENT;
    return s;
  }
  if (static_cast<int64_t>(m) * n > INT_MAX || offset <= -kPatternMaxOffset || offset >= kPatternMaxOffset ||
      !order_route(1, m, n).served)
    return s;
  s.walk = build_shape(1, m, n, kLoadBytes / kPatternV);
  s.status = s.walk.status;
  s.served = s.status == 0 ? 1 : 0;
  return s;
}

// What the entries refuse: a rule with a field outside its range.  (A rule without a component
// keeps nothing; ops.attention_pattern_csr turns it away.)
inline bool pattern_ok(const sputnik_hip_attention_pattern_args& a) {
  const bool window = a.window_left >= 0;
  if (a.dilation < 1 || a.dilation > kPatternReach || a.block < 0 || a.summary_stride < 0 || a.random_block < 0)
    return false;
  if (window && (a.window_left > kPatternReach || a.window_right < 0 || a.window_right > kPatternReach)) return false;
  if (a.summary_stride > 0 && a.summary_first < 0) return false;
  if (a.random_block > 0 && a.random_threshold > 0x80000000u) return false;
  return a.global_flags == nullptr || aligned_to(a.global_flags, kPatternV);
}

// What a row fixes for all of its columns.
struct PatternRow {
  bool live, full;            // a row of the matrix; a global row: every column
  int64_t p;                  // its position
  int64_t lo, hi;             // the window's columns (lo > hi: none)
  int64_t block_lo, block_hi; // the block's columns (none for p < 0)
  int64_t last;               // the last column kept: p for a causal row, else n - 1
  unsigned random_row;        // R = r / rb

  __device__ __forceinline__ PatternRow(const RowGroup& g, const sputnik_hip_attention_pattern_args& a, int m, int n) {
    live = g.row < m;
    p = g.row + a.offset;
    lo = 1;
    hi = 0;
    if (a.window_left >= 0) {
      lo = max(p - a.window_left, int64_t{0});
      hi = min(p + a.window_right, static_cast<int64_t>(n) - 1);
    }
    block_lo = 1;
    block_hi = 0;
    if (a.block > 0 && p >= 0) {
      block_lo = p / a.block * a.block;
      block_hi = block_lo + a.block - 1;
    }
    last = a.causal ? min(p, static_cast<int64_t>(n) - 1) : static_cast<int64_t>(n) - 1;
    full = live && a.global_flags != nullptr && a.global_rows && p >= 0 && p < n && a.global_flags[p] != 0;
    random_row = a.random_block > 0 ? static_cast<unsigned>(g.row / a.random_block) : 0u;
  }
};

// The random blocks' words a lane holds: those of the last (C >> 2, R) it met.
struct PatternDraw {
  unsigned quad = 0xffffffffu;   // (C >> 2 stays below 2^29)
  uint4 words = make_uint4(0u, 0u, 0u, 0u);
};

// A bit per column c0 .. c0 + 3 of the row that the rule keeps.
__device__ __forceinline__ unsigned pattern_flags(const sputnik_hip_attention_pattern_args& a, const PhiloxKey& key,
                                                  const PatternRow& row, int64_t c0, int n, PatternDraw* draw) {
  constexpr int V = kPatternV;
  if (!row.live || c0 >= n || c0 > row.last) return 0u;
  const int64_t inside = min(static_cast<int64_t>(n) - 1, row.last) - c0 + 1;   // >= 1
  const unsigned open = inside >= V ? (1u << V) - 1u : (1u << inside) - 1u;
  if (row.full) return open;
  unsigned keep = 0u;
  if (c0 + (V - 1) >= row.lo && c0 <= row.hi) {   // the window
    int64_t rem = 0;   // floor-mod of c0 - p
    if (a.dilation > 1) {
      rem = (c0 - row.p) % a.dilation;
      if (rem < 0) rem += a.dilation;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int64_t c = c0 + e, t = rem + e;   // (t < dilation + 4: a multiple is one of four)
      const bool on = a.dilation == 1 || t == 0 || t == a.dilation || t == 2 * a.dilation || t == 3 * a.dilation;
      keep |= (c >= row.lo && c <= row.hi && on ? 1u : 0u) << e;
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) keep |= (c0 + e >= row.block_lo && c0 + e <= row.block_hi ? 1u : 0u) << e;
  if (a.summary_stride > 0) {
    const unsigned stride = static_cast<unsigned>(a.summary_stride), first = static_cast<unsigned>(a.summary_first);
    unsigned t = static_cast<unsigned>(c0) % stride;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      keep |= (t >= first ? 1u : 0u) << e;
      if (++t == stride) t = 0u;
    }
  }
  if (a.global_flags != nullptr) {
    if (c0 + V <= n) {   // (aligned: the vector starts on 4 bytes, c0 is a multiple of 4)
      const unsigned four = *reinterpret_cast<const unsigned*>(a.global_flags + c0);
#pragma unroll
      for (int e = 0; e < V; ++e) keep |= (((four >> (8 * e)) & 0xffu) != 0u ? 1u : 0u) << e;
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (c0 + e < n) keep |= (a.global_flags[c0 + e] != 0 ? 1u : 0u) << e;
    }
  }
  if (a.random_block > 0) {
    const unsigned rb = static_cast<unsigned>(a.random_block);
    unsigned block = static_cast<unsigned>(c0) / rb, at = static_cast<unsigned>(c0) % rb;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if ((open >> e) & 1u) {
        if ((block >> 2) != draw->quad) {
          draw->quad = block >> 2;
          draw->words = philox4x32_10(key, draw->quad, row.random_row);
        }
        const unsigned k = uint4_word(draw->words, static_cast<int>(block & 3u)) & 0x7fffffffu;
        keep |= (k < a.random_threshold ? 1u : 0u) << e;
      }
      if (++at == rb) {
        at = 0u;
        ++block;
      }
    }
  }
  return keep & open;
}

// FILL = false: row_offsets[row + 1] = kept columns of the row.
// FILL = true:  the kept columns of the row go to row_offsets[row] onwards, ascending, inside
//               [0, nonzeros) whatever the offsets say.
template <bool FILL>
__global__ __launch_bounds__(kBuildBlock) void attention_pattern_rows_kernel(
    int m, int n, int rows_per_wave, PatternArgs args, int nonzeros, int* __restrict__ row_offsets,
    int* __restrict__ column_indices) {
  constexpr int V = kPatternV;
  const sputnik_hip_attention_pattern_args& a = args.rule;
  const RowGroup g(rows_per_wave);
  PhiloxKey key = {0u, 0u, 0u, 0u};
  if (a.random_block > 0) key = philox_key(args.state, !FILL && blockIdx.x == 0 && threadIdx.x == 0);
  const PatternRow row(g, a, m, n);
  PatternDraw draw;
  const int64_t span = static_cast<int64_t>(g.group_lanes) * V;
  const int steps = static_cast<int>((static_cast<int64_t>(n) + span - 1) / span);   // (the wave's: ballots)
  // A rule of window and block alone keeps nothing outside their columns: the wave walks the
  // steps from the first such column of its rows to the last one.
  int first_step = 0, end_step = steps;
  if (a.global_flags == nullptr && a.summary_stride == 0 && a.random_block == 0) {
    int64_t from = n, to = -1;
    if (row.live) {
      if (row.lo <= row.hi) {
        from = row.lo;
        to = row.hi;
      }
      if (row.block_lo <= row.block_hi) {
        from = min(from, row.block_lo);
        to = max(to, row.block_hi);
      }
      to = min(to, row.last);
    }
    first_step = to < from ? steps : static_cast<int>(min(from / span, static_cast<int64_t>(steps)));
    end_step = to < from ? 0 : static_cast<int>(min(to / span + 1, static_cast<int64_t>(steps)));
    for (int o = kWave / 2; o > 0; o >>= 1) {
      first_step = min(first_step, __shfl_xor(first_step, o, kWave));
      end_step = max(end_step, __shfl_xor(end_step, o, kWave));
    }
  }

  int64_t out = 0;
  if constexpr (FILL) {
    if (row.live) out = row_offsets[g.row];
  }
  int count = 0;
  for (int s = first_step; s < end_step; ++s) {
    const int64_t c0 = (static_cast<int64_t>(s) * g.group_lanes + g.group_lane) * V;
    const unsigned flags = pattern_flags(a, key, row, c0, n, &draw);
    if constexpr (!FILL) {
      count += __popc(flags);
    } else {
      const Prefix at = group_prefix<V>(g, flags);
      int64_t p = out + at.before;
#pragma unroll
      for (int e = 0; e < V; ++e)
        if ((flags >> e) & 1u) {
          if (p >= 0 && p < nonzeros) column_indices[p] = static_cast<int>(c0 + e);
          ++p;
        }
      out += at.total;
    }
  }
  if constexpr (!FILL) {
    for (int o = g.group_lanes / 2; o > 0; o >>= 1) count += __shfl_xor(count, o, kWave);
    if (row.live && g.group_lane == 0) row_offsets[g.row + 1] = count;
  }
}

inline PatternArgs pattern_args(const sputnik_hip_attention_pattern_args& rule, const sputnik_hip_philox_state& rng,
                                int64_t* rng_state_out) {
  PatternArgs args;
  args.rule = rule;
  args.state.rng = rng;
  args.state.rng_state_out = rng_state_out;
  args.state.threshold = 0u;
  args.state.scale = 0.f;
  args.state.replica0 = 0;
  return args;
}

// ---------------------------------------------------------------------------
// Top-k selection over a dense floating matrix, written straight out as a CSR topology
// (sputnik_hip_topk_to_csr).  Ranking by key (key_of) is ranking by |x|: -0.0 ties with 0.0,
// denormals rank by their bits, inf above every finite value and NaN above inf.  Both modes
// come down to a Selection (T_r, q_r) per row, ties in ascending column order.
//   per row   every row keeps its k largest keys: ONE launch runs radix_select for every row;
//             it writes offsets r * k and row_indices r as well (equal lengths: no sort)
//   total     the matrix keeps its K largest keys, ties to the lowest flat index: after a launch
//             that clears them, one launch per digit (workgroup_digit_pass) merges the
//             workgroups' LDS histograms into 256 global bins (integer atomic adds, order
//             independent); every later workgroup derives the digits chosen so far from those
//             bins itself (total_select).  A rows launch counts g_r = #(key > T) and
//             t_r = #(key == T) (count_against_total), a scan launch (total_scan_kernel) turns
//             Q = K - #(key > T) into the rows' quotas q_r = clamp(Q - ties of the rows in
//             front, 0, t_r) and the offsets.
// The fill (fill_row) is group_prefix + admit_ties per step.  A row is RE-READ per digit pass
// (it comes from L2: a 2048 x 2048 float32 matrix is 16 MB) rather than held in registers,
// which would bound n, or in LDS, which the per-row histograms already fill.  Every count is an
// integer, every store a vector store: results are bitwise reproducible.  Nothing on the host
// depends on the data, and every launch is a kernel: a call is captured into a graph whole.
// ---------------------------------------------------------------------------
struct TopkShape {
  int status = 0;
  int served = 0, digit_passes = 0;
  BuildShape walk;
};
inline TopkShape topk_shape(int m, int n, int element_bytes, int total_mode) {
  TopkShape t;
  if ((element_bytes != 2 && element_bytes != 4) || (total_mode != 0 && total_mode != 1)) {
    t.status = SPUTNIK_HIP_INVALID_ARGUMENT;
    return t;
  }
  t.walk = build_shape(1, m, n, element_bytes);
  t.status = t.walk.status;
  if (t.status != 0) return t;
  t.digit_passes = element_bytes * 8 / kDigitBits;
  // total mode: rows of unequal lengths, ordered by the row-order kernel
  t.served = total_mode ? order_route(1, m, n).served : 1;
  return t;
}

// The workspace of a total selection, in 32-bit words: bins [4][256], threshold [1], for several
// layers the ties handed out so far [1]; then per layer quotas [m], ties [m].
struct TotalWorkspace {
  unsigned *bins, *threshold, *handed;
  int* rows;
  static size_t words(int64_t rows, bool layers) {
    return static_cast<size_t>(kMaxDigitPasses) * kDigitBins + 1 + (layers ? 1 : 0) + 2 * static_cast<size_t>(rows);
  }
  TotalWorkspace(void* workspace, bool layers) {
    bins = static_cast<unsigned*>(workspace);
    threshold = bins + kMaxDigitPasses * kDigitBins;
    handed = layers ? threshold + 1 : nullptr;
    rows = reinterpret_cast<int*>(threshold + 1 + (layers ? 1 : 0));
  }
  // of a layer of m rows: its quotas, and its ties m words on
  int* quotas(int64_t rows_in_front = 0) const { return rows + 2 * rows_in_front; }
};
// per row: thresholds [m], quotas [m].
inline size_t topk_workspace_words(int m, int total_mode) {
  return total_mode ? TotalWorkspace::words(m, false) : 2 * static_cast<size_t>(m);
}

// Per-row mode: (T_r, q_r), the offsets r * k and the row order 0 .. m - 1.
template <typename U>
__global__ __launch_bounds__(kBuildBlock) void topk_row_select_kernel(
    int m, int n, int rows_per_wave, int k, const U* __restrict__ scores, int64_t row_stride,
    unsigned* __restrict__ thresholds, int* __restrict__ quotas, int* __restrict__ row_offsets,
    int* __restrict__ row_indices) {
  constexpr int P = sizeof(U) * 8 / kDigitBits;
  __shared__ unsigned hist[kBuildWaves * kMaxRowsPerWave][kDigitBins];   // 64 KiB
  const RowGroup g(rows_per_wave);
  const RowWalk<U> walk(g, scores, row_stride, m, n);
  const Selection kept = radix_select<P>(g, hist[g.slot], k, [&](int shift, unsigned prefix, unsigned* bins) {
    digit_histogram(walk, shift, prefix, bins);
  });
  if (walk.live && g.group_lane == 0) {
    const int64_t row = g.row;
    thresholds[row] = kept.threshold;
    quotas[row] = kept.quota;
    row_offsets[row] = static_cast<int>(row * k);
    row_indices[row] = static_cast<int>(row);
    if (row == m - 1) row_offsets[m] = static_cast<int>(static_cast<int64_t>(m) * k);
  }
}

// Total mode: the global bins of every digit pass start at zero.  (A kernel, not a memset: a
// captured call clears them on every replay.)
static_assert(kMaxDigitPasses * kDigitBins == kScanBlock, "one thread per bin");
__global__ __launch_bounds__(kScanBlock) void total_clear_kernel(unsigned* __restrict__ bins) {
  bins[threadIdx.x] = 0u;
}

// Total mode: the digits chosen by the first `passes` passes, from their global bins; by EVERY
// thread of a workgroup of at least kDigitBins threads.  *need = what is still to take among
// the keys with that prefix; after the last pass the prefix is T and *need is Q.
// `shared`: kDigitBins / kWave + 2 words.
__device__ __forceinline__ unsigned total_select(const unsigned* bins, int passes, unsigned count,
                                                 unsigned* shared, unsigned* need_out) {
  constexpr int kBinWaves = kDigitBins / kWave;
  const int t = threadIdx.x, lane = t % kWave, wave = t / kWave;
  unsigned prefix = 0, need = count;
  for (int p = 0; p < passes; ++p) {
    const unsigned c = t < kDigitBins ? bins[p * kDigitBins + t] : 0u;
    unsigned incl = c;   // keys in my bin and in the wave's bins above it
    for (int off = 1; off < kWave; off <<= 1) {
      const unsigned up = __shfl_down(incl, off, kWave);
      if (lane + off < kWave) incl += up;
    }
    if (lane == 0 && wave < kBinWaves) shared[wave] = incl;
    __syncthreads();
    unsigned above = incl - c;
    for (int w = wave + 1; w < kBinWaves; ++w) above += shared[w];
    if (t < kDigitBins && need > 0 && above < need && need <= above + c) {
      shared[kBinWaves] = static_cast<unsigned>(t);
      shared[kBinWaves + 1] = need - above;
    }
    __syncthreads();
    if (need > 0) {
      prefix = (prefix << kDigitBits) | shared[kBinWaves];
      need = shared[kBinWaves + 1];
    }
    __syncthreads();
  }
  *need_out = need;
  return prefix;
}
constexpr int kSelectWords = kDigitBins / kWave + 2;

// Total mode, digit pass `pass` of P by one workgroup of kBuildBlock threads:
// walk(shift, prefix, hist) counts the workgroup's keys into an LDS histogram, that goes into
// bins[pass][*] with one integer atomic add per non-empty bin.
template <int P, typename Walk>
__device__ __forceinline__ void workgroup_digit_pass(int pass, unsigned count, unsigned* bins, Walk walk) {
  __shared__ unsigned hist[kDigitBins];
  __shared__ unsigned select[kSelectWords];
  unsigned need;
  const unsigned prefix = total_select(bins, pass, count, select, &need);
  hist[threadIdx.x] = 0u;
  __syncthreads();
  walk(kDigitBits * (P - 1 - pass), prefix, hist);
  __syncthreads();
  const unsigned c = hist[threadIdx.x];
  if (c != 0u) atomicAdd(&bins[pass * kDigitBins + threadIdx.x], c);
}

// One digit pass over the whole matrix: this workgroup's rows.
template <typename U>
__global__ __launch_bounds__(kBuildBlock) void topk_total_hist_kernel(
    int m, int n, int rows_per_wave, int pass, unsigned count, const U* __restrict__ scores,
    int64_t row_stride, unsigned* bins) {
  workgroup_digit_pass<sizeof(U) * 8 / kDigitBits>(pass, count, bins, [&](int shift, unsigned prefix, unsigned* hist) {
    const RowGroup g(rows_per_wave);
    const RowWalk<U> walk(g, scores, row_stride, m, n);
    digit_histogram(walk, shift, prefix, hist);
  });
}

// Total mode: greater[row] = base + #(key > T), ties[row] = #(key == T) of the walk's row, T from
// the filled bins; keys at most key_limit, open(first column) = a bit per element of the piece
// that takes part.
template <typename Walk, typename Open>
__device__ __forceinline__ void count_against_total(const RowGroup& g, const Walk& walk, unsigned count,
                                                    const unsigned* __restrict__ bins, unsigned key_limit, Open open,
                                                    int base, int* __restrict__ greater_out, int* __restrict__ ties) {
  using U = typename Walk::Element;
  __shared__ unsigned select[kSelectWords];
  unsigned need;
  const unsigned prefix = total_select(bins, sizeof(U) * 8 / kDigitBits, count, select, &need);
  const unsigned threshold = count > 0 ? prefix : kNoThreshold;
  int greater = 0, equal = 0;
  for (int s = 0; s < walk.steps; ++s) {
    int64_t c0;
    unsigned valid, above, same;
    const Piece<U> v = walk.load(s, &c0, &valid);
    compare_piece(v, threshold, key_limit, &above, &same);
    const unsigned counted = valid & open(c0);
    greater += __popc(above & counted);
    equal += __popc(same & counted);
  }
  for (int o = g.group_lanes / 2; o > 0; o >>= 1) {
    greater += __shfl_xor(greater, o, kWave);
    equal += __shfl_xor(equal, o, kWave);
  }
  if (walk.live && g.group_lane == 0) {
    greater_out[g.row] = base + greater;
    ties[g.row] = equal;
  }
}
template <typename Walk>
__device__ __forceinline__ void count_against_total(const RowGroup& g, const Walk& walk, unsigned count,
                                                    const unsigned* __restrict__ bins, int* __restrict__ greater_out,
                                                    int* __restrict__ ties) {
  count_against_total(g, walk, count, bins, kNoThreshold, [](int64_t) { return ~0u; }, 0, greater_out, ties);
}

// Total mode: row_offsets[row + 1] = #(key > T), ties[row] = #(key == T).
template <typename U>
__global__ __launch_bounds__(kBuildBlock) void topk_total_rows_kernel(
    int m, int n, int rows_per_wave, unsigned count, const U* __restrict__ scores, int64_t row_stride,
    const unsigned* __restrict__ bins, int* __restrict__ row_offsets, int* __restrict__ ties) {
  const RowGroup g(rows_per_wave);
  const RowWalk<U> walk(g, scores, row_stride, m, n);
  count_against_total(g, walk, count, bins, row_offsets + 1, ties);
}

// Total mode, one workgroup per layer, the layers of a selection in order: quotas[r] =
// clamp(Q - ties handed out in front, 0, ties[r]); the lengths #(key > T) + quotas[r], scanned
// in place into the offsets; *threshold = T.  The ties of the layers in front are *handed_in
// (null: none, the first or only layer); *handed_out = that plus this layer's ties and
// *new_size = the layer's kept entries, where asked for.
__global__ __launch_bounds__(kScanBlock) void total_scan_kernel(
    int m, int digit_passes, unsigned count, const unsigned* __restrict__ bins, const int* __restrict__ ties,
    int* __restrict__ quotas, int* __restrict__ offsets, unsigned* __restrict__ threshold,
    const unsigned* handed_in, unsigned* handed_out, int* new_size) {
  __shared__ int wave_sums[kScanBlock / kWave];
  __shared__ unsigned select[kSelectWords];
  const int64_t in_front = handed_in != nullptr ? static_cast<int64_t>(*handed_in) : int64_t{0};
  unsigned need;
  const unsigned prefix = total_select(bins, digit_passes, count, select, &need);   // (barriers: *handed_in is read)
  const int64_t quota = static_cast<int64_t>(need) - in_front;
  const Span span = thread_span(m);
  int mine = 0;
  for (int64_t i = span.begin; i < span.end; ++i) mine += ties[i];
  int tied_here;
  int64_t ties_before = block_exclusive_scan(mine, wave_sums, &tied_here);
  __syncthreads();   // (wave_sums is written again)
  mine = 0;
  for (int64_t i = span.begin; i < span.end; ++i) {
    const int tied = ties[i];
    const int q = static_cast<int>(max(int64_t{0}, min(static_cast<int64_t>(tied), quota - ties_before)));
    ties_before += tied;
    quotas[i] = q;
    const int length = offsets[1 + i] + q;
    offsets[1 + i] = length;
    mine += length;
  }
  const int total = inclusive_scan_span(span, mine, wave_sums, offsets + 1, [&](int64_t i) { return offsets[1 + i]; });
  if (threadIdx.x == 0) {
    offsets[0] = 0;
    *threshold = count > 0 ? prefix : kNoThreshold;
    if (handed_out != nullptr) *handed_out = static_cast<unsigned>(in_front + tied_here);
    if (new_size != nullptr) *new_size = total;
  }
}

// The elements of the walk's row that `kept` selects into the slots [out, end), in the order of
// the walk: store(slot, the element's index in the row, the element).
template <typename Walk, typename Store>
__device__ __forceinline__ void fill_row(const RowGroup& g, const Walk& walk, Selection kept, int64_t out,
                                         int64_t end, Store store) {
  using U = typename Walk::Element;
  constexpr int V = Walk::V;
  int ties_seen = 0;   // elements equal to the threshold in the steps behind
  for (int s = 0; s < walk.steps; ++s) {
    int64_t c0;
    unsigned valid, greater, equal;
    const Piece<U> v = walk.load(s, &c0, &valid);
    compare_piece(v, kept.threshold, kNoThreshold, &greater, &equal);
    const unsigned flags = admit_ties<V>(g, greater & valid, equal & valid, kept.quota, &ties_seen);
    const Prefix at = group_prefix<V>(g, flags);
    int64_t p = out + at.before;
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (((flags >> e) & 1u) && p < end) {   // (no store ever leaves the row's slots)
        store(p, c0 + e, v.e[e]);
        ++p;
      }
    out += at.total;
  }
}

// The kept columns of every row, ascending, from row_offsets[row] onwards; VB != 0: and the
// elements of `values_from` (VB bytes each) at the kept positions, bit for bit.
template <typename U, int VB>
__global__ __launch_bounds__(kBuildBlock) void topk_fill_kernel(
    int m, int n, int rows_per_wave, const U* __restrict__ scores, int64_t row_stride,
    const unsigned* __restrict__ thresholds, int threshold_stride, const int* __restrict__ quotas,
    const int* __restrict__ row_offsets, const void* __restrict__ values_from, int64_t values_row_stride,
    int* __restrict__ column_indices, void* __restrict__ values) {
  using W = typename std::conditional<VB == 2, uint16_t, uint32_t>::type;
  const RowGroup g(rows_per_wave);
  const RowWalk<U> walk(g, scores, row_stride, m, n);
  const int64_t row = g.row;
  const Selection kept = {walk.live ? thresholds[row * threshold_stride] : kNoThreshold, walk.live ? quotas[row] : 0};
  const W* __restrict__ payload =
      static_cast<const W*>(values_from) + (VB != 0 && walk.live ? row * values_row_stride : int64_t{0});
  fill_row(g, walk, kept, walk.live ? row_offsets[row] : 0, walk.live ? row_offsets[row + 1] : 0,
           [&](int64_t p, int64_t column, U) {
             column_indices[p] = static_cast<int>(column);
             if constexpr (VB != 0) static_cast<W*>(values)[p] = payload[column];
           });
}

// f(uint16_t{}) or f(uint32_t{}): the launch for 2- or 4-byte elements (the entries check the width).
template <typename F>
inline int by_width(int element_bytes, F f) {
  return element_bytes == 2 ? f(uint16_t{}) : f(uint32_t{});
}

// Total mode: the bins cleared, then hist(pass) launches each of the digit passes.
template <typename Hist>
inline void launch_digit_passes(unsigned* bins, int digit_passes, hipStream_t stream, Hist hist) {
  hipLaunchKernelGGL(total_clear_kernel, dim3(1), dim3(kScanBlock), 0, stream, bins);
  for (int p = 0; p < digit_passes; ++p) hist(p);
}

// Total mode: the scan of a layer of m rows whose quotas start at `quotas`; `first`: no layer in front.
inline void launch_total_scan(const TotalWorkspace& w, int* quotas, int m, int digit_passes, unsigned count,
                              int* offsets, bool first, int* new_size, hipStream_t stream) {
  hipLaunchKernelGGL(total_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, m, digit_passes, count, w.bins,
                     quotas + m, quotas, offsets, w.threshold,
                     first ? static_cast<const unsigned*>(nullptr) : w.handed, w.handed, new_size);
}

template <typename U>
int launch_topk(const TopkShape& t, int m, int n, const void* scores_, int64_t row_stride, int total_mode,
                unsigned count, const void* values_from, int value_bytes, int64_t values_row_stride,
                unsigned* workspace, int* row_indices, int* row_offsets, int* column_indices, void* values,
                hipStream_t stream) {
  const U* scores = static_cast<const U*>(scores_);
  const int rows = t.walk.rows_per_wave;
  const dim3 grid(t.walk.grid), block(kBuildBlock);
  const unsigned* thresholds;
  const int* quotas;
  if (!total_mode) {
    unsigned* th = workspace;
    int* q = reinterpret_cast<int*>(workspace + m);
    hipLaunchKernelGGL((topk_row_select_kernel<U>), grid, block, 0, stream, m, n, rows, static_cast<int>(count),
                       scores, row_stride, th, q, row_offsets, row_indices);
    thresholds = th;
    quotas = q;
  } else {
    const TotalWorkspace w(workspace, false);
    launch_digit_passes(w.bins, t.digit_passes, stream, [&](int p) {
      hipLaunchKernelGGL((topk_total_hist_kernel<U>), grid, block, 0, stream, m, n, rows, p, count, scores,
                         row_stride, w.bins);
    });
    hipLaunchKernelGGL((topk_total_rows_kernel<U>), grid, block, 0, stream, m, n, rows, count, scores, row_stride,
                       w.bins, row_offsets, w.quotas() + m);
    launch_total_scan(w, w.quotas(), m, t.digit_passes, count, row_offsets, true, nullptr, stream);
    thresholds = w.threshold;
    quotas = w.quotas();
  }
  int st = launch_status();
  if (st != 0) return st;
  if (count > 0 && column_indices != nullptr) {
    const int stride = total_mode ? 0 : 1;
    const auto fill = [&](auto vb) {
      hipLaunchKernelGGL((topk_fill_kernel<U, decltype(vb)::value>), grid, block, 0, stream, m, n, rows, scores,
                         row_stride, thresholds, stride, quotas, row_offsets, values_from, values_row_stride,
                         column_indices, values);
      return launch_status();
    };
    if (values == nullptr) st = fill(std::integral_constant<int, 0>{});
    else if (value_bytes == 2) st = fill(std::integral_constant<int, 2>{});
    else st = fill(std::integral_constant<int, 4>{});
  }
  return st;
}

// ---------------------------------------------------------------------------
// Per-row drop-and-grow of a CSR topology (sputnik_hip_csr_regrow): every row keeps the c_r of
// its len_r entries with the largest value keys and takes the d_r = len_r - c_r columns outside
// them with the largest score keys, in its own slots.  ONE launch: the group of lanes that
// walks a row decides everything about it, and what the phases hand each other -- (T_v, q_v),
// the old / kept bits of the columns, (T_s, q_s) -- stays in its registers and in its part of
// LDS.  (A select + fill pair, as the top-k build has, would have to write the kept bits of
// every row out and read them back, or mark them twice.)
//   1  radix_select over values[row_offsets[r] ..] (a ragged read, lane after lane): (T_v, q_v)
//   2  the row's entries again: the old columns and the kept ones into two bit planes in LDS
//   3  radix_select over the dense score row outside the kept columns, keys clamped to the
//      largest finite one: (T_s, q_s)
//   4  admit_ties + group_prefix per step of the score row, as fill_row does; a running
//      group_prefix of the old bits is the old entry index of a kept column
// LDS of a row: the 256 bins and 2 * ceil(n / 32) words of bit planes.  Four rows of that at
// one row per wave fit 64 KiB up to n = kRegrowMaxN; 64 rows (16 per wave) do not at any n, so
// the narrowest instance is 8 rows per wave.
// ---------------------------------------------------------------------------
constexpr int kRegrowLdsBytes = 64 * 1024;   // what a launch gets without asking for more
constexpr int kRegrowMaxRowsPerWave = 8;
constexpr int kRegrowMaxN = 32 * ((kRegrowLdsBytes / kBuildWaves - kDigitBins * 4) / 8);
static_assert(kBuildWaves * kRegrowMaxRowsPerWave * (kDigitBins + 2 * 2) * 4 <= kRegrowLdsBytes,
              "8 rows per wave: n <= 8 * 8 columns, 2 words per plane");

struct RegrowShape {
  int status = 0;
  int served = 0, max_n = kRegrowMaxN;
  int rows_per_wave = -1, elements_per_lane = -1, rows_per_workgroup = -1;
  int value_passes = -1, score_passes = -1, words = -1, lds_bytes = -1, grid = -1;
};
inline RegrowShape regrow_shape(int m, int n, int score_bytes, int value_bytes) {
  RegrowShape r;
  if ((score_bytes != 2 && score_bytes != 4) || (value_bytes != 2 && value_bytes != 4)) {
    r.status = SPUTNIK_HIP_INVALID_ARGUMENT;
    return r;
  }
  const BuildShape walk = build_shape(1, m, n, score_bytes);
  r.status = walk.status;
  if (r.status != 0 || n > kRegrowMaxN) return r;
  r.served = 1;
  r.rows_per_wave = min(walk.rows_per_wave, kRegrowMaxRowsPerWave);
  r.elements_per_lane = walk.elements_per_lane;
  r.rows_per_workgroup = kBuildWaves * r.rows_per_wave;
  r.value_passes = value_bytes * 8 / kDigitBits;
  r.score_passes = score_bytes * 8 / kDigitBits;
  r.words = n / 32 + (n % 32 != 0 ? 1 : 0);
  r.lds_bytes = r.rows_per_workgroup * (kDigitBins + 2 * r.words) * static_cast<int>(sizeof(unsigned));
  r.grid = static_cast<int>(ceil_div64(m, r.rows_per_workgroup));
  return r;
}

// Bit e of the result: the plane's bit of column first_column + e, e < 32; columns outside
// the plane read 0.  first_column >= -31 (a piece starts at most V - 1 columns before its row).
__device__ __forceinline__ unsigned plane_bits(const unsigned* __restrict__ plane, int words, int64_t first_column) {
  const int64_t shifted = first_column + 32;
  const int64_t w = (shifted >> 5) - 1;
  const unsigned lo = w >= 0 && w < words ? plane[w] : 0u;
  const unsigned hi = w + 1 < words ? plane[w + 1] : 0u;
  return static_cast<unsigned>(((static_cast<uint64_t>(hi) << 32) | lo) >> (shifted & 31));
}

// The old columns of the row's entries [begin, end) and those of them that `keep` selects, into
// two bit planes of `words` words in LDS.  A column outside 0 .. n - 1 sets no bit.  Every thread
// of the workgroup calls it: two barriers.
template <typename W>
__device__ __forceinline__ void mark_row_planes(const RowGroup& g, int begin, int end, int n, Selection keep,
                                                const int* __restrict__ column_indices, const W* __restrict__ values,
                                                unsigned* __restrict__ old_bits, unsigned* __restrict__ kept_bits,
                                                int words) {
  // steps of the walk over the row's entries, the most of the wave's rows: every lane of the
  // wave takes part in every ballot
  int entry_steps = static_cast<int>((static_cast<int64_t>(end - begin) + g.group_lanes - 1) / g.group_lanes);
  for (int o = kWave / 2; o > 0; o >>= 1) entry_steps = max(entry_steps, __shfl_xor(entry_steps, o, kWave));
  for (int j = g.group_lane; j < words; j += g.group_lanes) {
    old_bits[j] = 0u;
    kept_bits[j] = 0u;
  }
  __syncthreads();
  int ties_seen = 0;
  for (int s = 0; s < entry_steps; ++s) {
    const int64_t i = static_cast<int64_t>(begin) + static_cast<int64_t>(s) * g.group_lanes + g.group_lane;
    const bool in = i < end;
    const unsigned key = in ? key_of(values[i]) : 0u;
    const int column = in ? column_indices[i] : -1;
    const bool tie = in && key == keep.threshold;
    const Prefix ties = group_prefix<1>(g, tie ? 1u : 0u);
    const int rank = ties_seen + ties.before;
    ties_seen += ties.total;
    if (in && static_cast<unsigned>(column) < static_cast<unsigned>(n)) {
      const unsigned bit = 1u << (column & 31);
      atomicOr(&old_bits[column >> 5], bit);
      if (key > keep.threshold || (tie && rank < keep.quota)) atomicOr(&kept_bits[column >> 5], bit);
    }
  }
  __syncthreads();
}

// The new row of a drop-and-grow step, ascending, into the slots [out, out_end): the kept
// columns and those open ones that `grow` selects by their clamped score keys.  admit_ties +
// group_prefix per step of the score row, as fill_row does; a running group_prefix of the old
// bits is the old entry index of a kept column, checked against the old row's end before the
// value is read.  grown(column) = the bits a grown slot stores; it is called for grown slots only,
// in ascending column order.
template <typename Walk, typename W, typename Grown>
__device__ __forceinline__ void regrow_fill_row(const RowGroup& g, const Walk& walk,
                                                const unsigned* __restrict__ old_bits,
                                                const unsigned* __restrict__ kept_bits, int words, Selection grow,
                                                unsigned key_limit, int begin, int end, int64_t out, int64_t out_end,
                                                const W* __restrict__ values, int* __restrict__ out_columns,
                                                W* __restrict__ out_values, int64_t* __restrict__ out_source,
                                                Grown grown) {
  using S = typename Walk::Element;
  constexpr int V = Walk::V;
  int old_seen = 0;    // old columns in the steps behind
  int ties_seen = 0;   // open columns equal to the threshold in the steps behind
  for (int s = 0; s < walk.steps; ++s) {
    int64_t c0;
    unsigned valid, greater, equal;
    const Piece<S> v = walk.load(s, &c0, &valid);
    const unsigned old = valid & plane_bits(old_bits, words, c0);
    const unsigned kept = valid & plane_bits(kept_bits, words, c0);
    compare_piece(v, grow.threshold, key_limit, &greater, &equal);
    const unsigned open = valid & ~kept;
    const unsigned flags = admit_ties<V>(g, kept | (greater & open), equal & open, grow.quota, &ties_seen);
    const Prefix at = group_prefix<V>(g, flags), olds = group_prefix<V>(g, old);
    int64_t p = out + at.before;
    int64_t from = static_cast<int64_t>(begin) + old_seen + olds.before;   // old entries in front of my piece
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (((flags >> e) & 1u) && p < out_end) {   // (no store ever leaves the row's slots)
        const bool carried = ((kept >> e) & 1u) && from < end;
        out_columns[p] = static_cast<int>(c0 + e);
        W bits;
        if (carried) bits = values[from];
        else bits = grown(c0 + e);
        out_values[p] = bits;
        out_source[p] = carried ? from : int64_t{-1};
        ++p;
      }
      from += (old >> e) & 1u;
    }
    out += at.total;
    old_seen += olds.total;
  }
}

// The SCORES of a drop-and-grow step, a kernel argument: walk(g, m, n, publish) = the walk of
// the group's score row, grown<W>(walk) = what a grown slot of that row stores.  Stored scores
// are a dense matrix in memory and grow zeros; KeyScores (below, next to KeyWalk) are generated.
template <typename S>
struct StoredScores {
  using Walk = RowWalk<S>;
  const S* scores;
  int64_t row_stride;
  __device__ __forceinline__ Walk walk(const RowGroup& g, int m, int n, bool) const {
    return Walk(g, scores, row_stride, m, n);
  }
  template <typename W>
  __device__ __forceinline__ auto grown(const Walk&) const {
    return [](int64_t) { return W{0}; };
  }
};

template <typename Scores, typename W>
__global__ __launch_bounds__(kBuildBlock) void csr_regrow_kernel(
    int m, int n, int nonzeros, int rows_per_wave, int words, unsigned key_limit,
    const int* __restrict__ row_offsets, const int* __restrict__ column_indices, const W* __restrict__ values,
    const int* __restrict__ drop_counts, Scores scores, int* __restrict__ out_columns, W* __restrict__ out_values,
    int64_t* __restrict__ out_source) {
  using Walk = typename Scores::Walk;
  constexpr int PV = sizeof(W) * 8 / kDigitBits, PS = sizeof(typename Walk::Element) * 8 / kDigitBits;
  extern __shared__ unsigned regrow_lds[];   // per row: bins [256], old bits [words], kept bits [words]
  const RowGroup g(rows_per_wave);
  const Walk walk = scores.walk(g, m, n, blockIdx.x == 0 && threadIdx.x == 0);
  unsigned* __restrict__ bins = regrow_lds + g.slot * (kDigitBins + 2 * words);
  unsigned* __restrict__ old_bits = bins + kDigitBins;
  unsigned* __restrict__ kept_bits = old_bits + words;

  int begin, end;
  row_slots(row_offsets, g.row, walk.live, nonzeros, &begin, &end);
  const int length = end - begin;
  const int drop = walk.live ? min(max(drop_counts[g.row], 0), length) : 0;

  // 1: (T_v, q_v) of the length - drop largest value keys: a ragged read, lane after lane
  const Selection keep = radix_select<PV>(g, bins, length - drop, [&](int shift, unsigned prefix, unsigned* b) {
    for (int64_t i = static_cast<int64_t>(begin) + g.group_lane; i < end; i += g.group_lanes)
      count_digit(key_of(values[i]), true, shift, prefix, b);
  });

  // 2: the old and the kept columns
  mark_row_planes(g, begin, end, n, keep, column_indices, values, old_bits, kept_bits, words);

  // 3: (T_s, q_s) of the drop largest score keys outside the kept columns, keys clamped
  const Selection grow = radix_select<PS>(g, bins, drop, [&](int shift, unsigned prefix, unsigned* b) {
    digit_histogram(walk, shift, prefix, b, key_limit,
                    [&](int64_t c0) { return ~plane_bits(kept_bits, words, c0); });
  });

  // 4: the new row, ascending, into [begin, end)
  regrow_fill_row(g, walk, old_bits, kept_bits, words, grow, key_limit, begin, end, begin, end, values, out_columns,
                  out_values, out_source, scores.template grown<W>(walk));
}

template <typename Scores, typename W>
int launch_regrow(const RegrowShape& r, int m, int n, int nonzeros, const int* row_offsets,
                  const int* column_indices, const void* values, const int* drop_counts, const Scores& scores,
                  unsigned key_limit, int* out_columns, void* out_values, int64_t* out_source, hipStream_t stream) {
  hipLaunchKernelGGL((csr_regrow_kernel<Scores, W>), dim3(r.grid), dim3(kBuildBlock), r.lds_bytes, stream, m, n,
                     nonzeros, r.rows_per_wave, r.words, key_limit, row_offsets, column_indices,
                     static_cast<const W*>(values), drop_counts, scores, out_columns, static_cast<W*>(out_values),
                     out_source);
  return launch_status();
}

// ---------------------------------------------------------------------------
// Top-k over the entries of a CSR pattern, written out as a smaller CSR pattern
// (sputnik_hip_csr_topk): gradual magnitude pruning of a layer that has no dense weight any
// more.  The keys and the Selection are those of the dense top-k above; what is ranked are
// the nnz stored values, and a kept entry keeps its column, its value bits and its old index.
// The kept set is the old pattern filtered, so its columns are in order already.
//   per row   the new lengths min(len_r, k) follow from the offsets alone: one scan launch; then
//             ONE launch in which the group of lanes that walks a row's entries runs
//             radix_select and fill_row into the row's new slots
//   total     the launches of the dense total mode, the digit passes (flat_digit_pass) over
//             the FLAT values array (entries, not rows)
// A row's entries are walked by entry_walk.  The group width comes from the mean row length
// nnz / m; a longer row takes more steps.
// ---------------------------------------------------------------------------
constexpr int kFlatSteps = 8;   // 16-byte pieces per lane of a workgroup of the flat walk

struct CsrTopkShape {
  int status = 0;
  int served = 0;
  int rows_per_wave = -1, group_lanes = -1, elements_per_lane = -1, rows_per_workgroup = -1;
  int digit_passes = -1, rows_grid = -1, flat_grid = -1;
};
inline CsrTopkShape csr_topk_shape(int m, int nonzeros, int value_bytes, int total_mode) {
  CsrTopkShape s;
  if (m < 0 || nonzeros < 0 || (value_bytes != 2 && value_bytes != 4) || (total_mode != 0 && total_mode != 1)) {
    s.status = SPUTNIK_HIP_INVALID_ARGUMENT;
    return s;
  }
  if (!order_route(1, m, 0).served) return s;   // (rows of unequal lengths in both modes)
  s.served = 1;
  s.elements_per_lane = kLoadBytes / value_bytes;
  const int mean = m > 0 ? nonzeros / m : 0;
  // the most rows per wave whose group of lanes still covers a row of mean length in one step
  s.rows_per_wave = kMaxRowsPerWave;
  while (s.rows_per_wave > 1 && mean > (kWave / s.rows_per_wave) * s.elements_per_lane) s.rows_per_wave /= 2;
  s.group_lanes = kWave / s.rows_per_wave;
  s.rows_per_workgroup = kBuildWaves * s.rows_per_wave;
  s.digit_passes = value_bytes * 8 / kDigitBits;
  s.rows_grid = static_cast<int>(ceil_div64(m, s.rows_per_workgroup));
  // pieces of the flat walk: at most V - 1 elements of lead in front of the array
  const int64_t pieces = static_cast<int64_t>(nonzeros) / s.elements_per_lane + 2;
  s.flat_grid = total_mode && nonzeros > 0 ? static_cast<int>(ceil_div64(pieces, int64_t{kBuildBlock} * kFlatSteps)) : 0;
  return s;
}

// fill_row over a row's entries from slot `begin`: a kept entry's column, value bits and old index.
template <typename U>
__device__ __forceinline__ void csr_fill_row(const RowGroup& g, const RowWalk<U>& walk, int begin, Selection kept,
                                             int64_t out, int64_t end, const int* __restrict__ column_indices,
                                             int* __restrict__ out_columns, U* __restrict__ out_values,
                                             int64_t* __restrict__ out_source) {
  fill_row(g, walk, kept, out, end, [&](int64_t p, int64_t entry, U bits) {
    const int64_t from = begin + entry;   // (a valid element: inside the row's slots)
    out_columns[p] = column_indices[from];
    out_values[p] = bits;
    out_source[p] = from;
  });
}

// The new slots of a row, inside [0, capacity) whatever the offsets say.
__device__ __forceinline__ void new_slots(const int* __restrict__ out_offsets, int64_t row, bool live,
                                          int64_t capacity, int64_t* out, int64_t* end) {
  *out = live ? max(out_offsets[row], 0) : 0;
  *end = live ? min(static_cast<int64_t>(out_offsets[row + 1]), capacity) : 0;
}

// Per-row mode, one workgroup: out_offsets = the scan of min(len_r, k).
__global__ __launch_bounds__(kScanBlock) void csr_topk_lengths_kernel(int m, int nonzeros, int k,
                                                                      const int* __restrict__ row_offsets,
                                                                      int* __restrict__ out_offsets) {
  __shared__ int wave_sums[kScanBlock / kWave];
  const Span span = thread_span(m);
  const auto length = [&](int64_t i) {
    int begin, end;
    row_slots(row_offsets, i, true, nonzeros, &begin, &end);
    return min(end - begin, k);
  };
  int mine = 0;
  for (int64_t i = span.begin; i < span.end; ++i) mine += length(i);
  inclusive_scan_span(span, mine, wave_sums, out_offsets + 1, length);
  if (threadIdx.x == 0) out_offsets[0] = 0;
}

// Per-row mode: select and fill of every row in one launch.
template <typename U>
__global__ __launch_bounds__(kBuildBlock) void csr_topk_rows_kernel(
    int m, int nonzeros, int rows_per_wave, int k, const int* __restrict__ row_offsets,
    const int* __restrict__ column_indices, const U* __restrict__ values, const int* __restrict__ out_offsets,
    int64_t capacity, int* __restrict__ out_columns, U* __restrict__ out_values, int64_t* __restrict__ out_source) {
  constexpr int P = sizeof(U) * 8 / kDigitBits;
  __shared__ unsigned hist[kBuildWaves * kMaxRowsPerWave][kDigitBins];   // 64 KiB
  const RowGroup g(rows_per_wave);
  const bool live = g.row < m;
  int begin, end;
  row_slots(row_offsets, g.row, live, nonzeros, &begin, &end);
  const RowWalk<U> walk = entry_walk(g, values, begin, end, live);
  const Selection kept = radix_select<P>(g, hist[g.slot], min(end - begin, k),
                                         [&](int shift, unsigned prefix, unsigned* bins) {
                                           digit_histogram(walk, shift, prefix, bins);
                                         });
  int64_t out, out_end;
  new_slots(out_offsets, g.row, live, capacity, &out, &out_end);
  csr_fill_row(g, walk, begin, kept, out, out_end, column_indices, out_columns, out_values, out_source);
}

// Total mode, one digit pass over a flat values array: workgroup `block` of the array counts
// its kFlatSteps * 256 pieces.
template <typename U>
__device__ __forceinline__ void flat_digit_pass(const U* __restrict__ values, int64_t nonzeros, int64_t block,
                                                int pass, unsigned count, unsigned* bins) {
  constexpr int V = kLoadBytes / sizeof(U);
  workgroup_digit_pass<sizeof(U) * 8 / kDigitBits>(pass, count, bins, [&](int shift, unsigned prefix, unsigned* hist) {
    const int lead = static_cast<int>((reinterpret_cast<uintptr_t>(values) % kLoadBytes) / sizeof(U));
    for (int s = 0; s < kFlatSteps; ++s) {
      const int64_t piece = (block * kFlatSteps + s) * kBuildBlock + threadIdx.x;
      unsigned valid;
      const Piece<U> v = load_piece(values, piece * V - lead, nonzeros, &valid);
#pragma unroll
      for (int e = 0; e < V; ++e) count_digit(key_of(v.e[e]), (valid >> e) & 1u, shift, prefix, hist);
    }
  });
}

template <typename U>
__global__ __launch_bounds__(kBuildBlock) void csr_topk_flat_hist_kernel(int nonzeros, int pass, unsigned count,
                                                                         const U* __restrict__ values,
                                                                         unsigned* bins) {
  flat_digit_pass(values, static_cast<int64_t>(nonzeros), static_cast<int64_t>(blockIdx.x), pass, count, bins);
}

// Total mode: out_offsets[row + 1] = #(key > T), ties[row] = #(key == T) of the row's entries.
template <typename U>
__global__ __launch_bounds__(kBuildBlock) void csr_topk_total_rows_kernel(
    int m, int nonzeros, int rows_per_wave, unsigned count, const int* __restrict__ row_offsets,
    const U* __restrict__ values, const unsigned* __restrict__ bins, int* __restrict__ out_offsets,
    int* __restrict__ ties) {
  const RowGroup g(rows_per_wave);
  const bool live = g.row < m;
  int begin, end;
  row_slots(row_offsets, g.row, live, nonzeros, &begin, &end);
  const RowWalk<U> walk = entry_walk(g, values, begin, end, live);
  count_against_total(g, walk, count, bins, out_offsets + 1, ties);
}

// Total mode: the fill of every row under the one threshold and the rows' quotas.
template <typename U>
__global__ __launch_bounds__(kBuildBlock) void csr_topk_total_fill_kernel(
    int m, int nonzeros, int rows_per_wave, const int* __restrict__ row_offsets,
    const int* __restrict__ column_indices, const U* __restrict__ values, const unsigned* __restrict__ threshold,
    const int* __restrict__ quotas, const int* __restrict__ out_offsets, int64_t capacity,
    int* __restrict__ out_columns, U* __restrict__ out_values, int64_t* __restrict__ out_source) {
  const RowGroup g(rows_per_wave);
  const bool live = g.row < m;
  int begin, end;
  row_slots(row_offsets, g.row, live, nonzeros, &begin, &end);
  const RowWalk<U> walk = entry_walk(g, values, begin, end, live);
  int64_t out, out_end;
  new_slots(out_offsets, g.row, live, capacity, &out, &out_end);
  csr_fill_row(g, walk, begin, {*threshold, live ? quotas[g.row] : 0}, out, out_end, column_indices, out_columns,
               out_values, out_source);
}

// `fill`: the output arrays are there.  Per-row mode with `offsets`: the scan launch first.
template <typename U>
int launch_csr_topk(const CsrTopkShape& s, int m, int nonzeros, const int* row_offsets, const int* column_indices,
                    const void* values_, int total_mode, unsigned count, bool offsets, bool fill,
                    void* workspace, int* out_offsets, int64_t capacity, int* out_columns, void* out_values_,
                    int64_t* out_source, hipStream_t stream) {
  const U* values = static_cast<const U*>(values_);
  U* out_values = static_cast<U*>(out_values_);
  const dim3 grid(s.rows_grid), block(kBuildBlock);
  if (!total_mode) {
    if (offsets)
      hipLaunchKernelGGL(csr_topk_lengths_kernel, dim3(1), dim3(kScanBlock), 0, stream, m, nonzeros,
                         static_cast<int>(count), row_offsets, out_offsets);
    if (fill)
      hipLaunchKernelGGL((csr_topk_rows_kernel<U>), grid, block, 0, stream, m, nonzeros, s.rows_per_wave,
                         static_cast<int>(count), row_offsets, column_indices, values, out_offsets, capacity,
                         out_columns, out_values, out_source);
    return launch_status();
  }
  const TotalWorkspace w(workspace, false);
  launch_digit_passes(w.bins, s.digit_passes, stream, [&](int p) {
    hipLaunchKernelGGL((csr_topk_flat_hist_kernel<U>), dim3(s.flat_grid), block, 0, stream, nonzeros, p, count,
                       values, w.bins);
  });
  hipLaunchKernelGGL((csr_topk_total_rows_kernel<U>), grid, block, 0, stream, m, nonzeros, s.rows_per_wave, count,
                     row_offsets, values, w.bins, out_offsets, w.quotas() + m);
  launch_total_scan(w, w.quotas(), m, s.digit_passes, count, out_offsets, true, nullptr, stream);
  hipLaunchKernelGGL((csr_topk_total_fill_kernel<U>), grid, block, 0, stream, m, nonzeros, s.rows_per_wave,
                     row_offsets, column_indices, values, w.threshold, w.quotas(), out_offsets, capacity,
                     out_columns, out_values, out_source);
  return launch_status();
}

// ---------------------------------------------------------------------------
// One top-k across the entries of SEVERAL CSR patterns (sputnik_hip_csr_topk_global_*): global
// magnitude pruning.  The total mode above, with the layers' flat values arrays walked into the
// SAME 256 bins, so that every layer derives the one threshold T and the one tie quota Q; the
// quota is handed out in layer order, inside a layer in entry order.
//   digits   one launch per digit serves up to kGlobalLayers layers: a workgroup finds its layer
//            and its piece range in a table that travels as a kernel argument; more layers
//            take further launches of the same pass, which add into the same bins
//   rows     per layer, csr_topk_total_rows_kernel under the shared bins and count
//   scan     per layer and in layer order, total_scan_kernel with the ties handed out to the
//            layers in front read from (and this layer's added to) one word of the workspace;
//            the layer's new size lands in sizes[layer]
//   fill     per layer, csr_topk_total_fill_kernel and the row order, once the caller has read
//            the sizes and has the arrays
// ---------------------------------------------------------------------------
constexpr int kGlobalLayers = 32;   // layers of one digit launch: 520 bytes of kernel arguments

struct GlobalTable {
  const void* values[kGlobalLayers];
  int nonzeros[kGlobalLayers];
  int first_block[kGlobalLayers + 1];   // (unused slots: the grid)
};

inline int global_flat_blocks(int nonzeros, int value_bytes) {
  if (nonzeros <= 0) return 0;
  const int64_t pieces = static_cast<int64_t>(nonzeros) / (kLoadBytes / value_bytes) + 2;
  return static_cast<int>(ceil_div64(pieces, int64_t{kBuildBlock} * kFlatSteps));
}

struct GlobalTopkShape {
  int status = 0;
  int served = 0;
  int digit_passes = -1, layers_per_launch = -1, elements_per_workgroup = -1, digit_launches = -1;
  int64_t entries = 0, rows = 0;
};
inline GlobalTopkShape global_topk_shape(int layers, const int* rows, const int* nonzeros, int value_bytes) {
  GlobalTopkShape g;
  if (layers < 0 || (layers > 0 && (rows == nullptr || nonzeros == nullptr)) ||
      (value_bytes != 2 && value_bytes != 4)) {
    g.status = SPUTNIK_HIP_INVALID_ARGUMENT;
    return g;
  }
  bool served = true;
  for (int l = 0; l < layers; ++l) {
    const CsrTopkShape s = csr_topk_shape(rows[l], nonzeros[l], value_bytes, 1);
    if (s.status != 0) {
      g.status = s.status;
      return g;
    }
    served = served && s.served;
    g.entries += nonzeros[l];
    g.rows += rows[l];
  }
  if (!served || g.entries > INT_MAX) return g;   // (the counts of a bin are 32 bit)
  g.served = 1;
  g.digit_passes = value_bytes * 8 / kDigitBits;
  g.layers_per_launch = kGlobalLayers;
  g.elements_per_workgroup = kBuildBlock * kFlatSteps * (kLoadBytes / value_bytes);
  g.digit_launches = static_cast<int>(ceil_div64(layers, kGlobalLayers));
  return g;
}
inline size_t global_topk_workspace_words(int64_t rows) { return TotalWorkspace::words(rows, true); }

// One digit pass over the flat values arrays of the table's layers: flat_digit_pass with the
// layer and the workgroup's place inside it looked up first.
template <typename U>
__global__ __launch_bounds__(kBuildBlock) void csr_topk_global_hist_kernel(GlobalTable table, int pass,
                                                                           unsigned count, unsigned* bins) {
  const int block = blockIdx.x;
  int layer = 0;   // (an empty layer has no workgroup: it is stepped over)
#pragma unroll
  for (int i = 1; i < kGlobalLayers; ++i) layer += block >= table.first_block[i] ? 1 : 0;
  flat_digit_pass(static_cast<const U*>(table.values[layer]), static_cast<int64_t>(table.nonzeros[layer]),
                  static_cast<int64_t>(block - table.first_block[layer]), pass, count, bins);
}

template <typename U>
int launch_global_select(const GlobalTopkShape& g, int layers, const int* rows, const int* nonzeros,
                         const int* const* row_offsets, const void* const* values, unsigned count,
                         void* workspace, int* const* out_offsets, int* out_sizes, hipStream_t stream) {
  const TotalWorkspace w(workspace, true);
  const dim3 block(kBuildBlock);
  launch_digit_passes(w.bins, g.digit_passes, stream, [&](int p) {
    for (int l0 = 0; l0 < layers; l0 += kGlobalLayers) {
      GlobalTable table;
      int grid = 0;
      for (int i = 0; i < kGlobalLayers; ++i) {
        const bool used = l0 + i < layers;
        table.values[i] = used ? values[l0 + i] : nullptr;
        table.nonzeros[i] = used ? nonzeros[l0 + i] : 0;
        table.first_block[i] = grid;
        if (used) grid += global_flat_blocks(nonzeros[l0 + i], static_cast<int>(sizeof(U)));
      }
      table.first_block[kGlobalLayers] = grid;
      if (grid > 0)
        hipLaunchKernelGGL((csr_topk_global_hist_kernel<U>), dim3(grid), block, 0, stream, table, p, count, w.bins);
    }
  });
  int64_t rows_in_front = 0;
  for (int l = 0; l < layers; ++l) {
    const int m = rows[l];
    const CsrTopkShape s = csr_topk_shape(m, nonzeros[l], static_cast<int>(sizeof(U)), 1);
    int* q = w.quotas(rows_in_front);
    rows_in_front += m;
    if (m > 0)
      hipLaunchKernelGGL((csr_topk_total_rows_kernel<U>), dim3(s.rows_grid), block, 0, stream, m, nonzeros[l],
                         s.rows_per_wave, count, row_offsets[l], static_cast<const U*>(values[l]), w.bins,
                         out_offsets[l], q + m);
    launch_total_scan(w, q, m, g.digit_passes, count, out_offsets[l], l == 0, out_sizes + l, stream);
  }
  return launch_status();
}

template <typename U>
int launch_global_fill(int layers, const int* rows, const int* nonzeros, const int* const* row_offsets,
                       const int* const* column_indices, const void* const* values, void* workspace,
                       const int64_t* capacity, int* const* out_offsets, int* const* out_columns,
                       void* const* out_values, int64_t* const* out_source, hipStream_t stream) {
  const TotalWorkspace w(workspace, true);
  int64_t rows_in_front = 0;
  for (int l = 0; l < layers; ++l) {
    const int m = rows[l];
    const CsrTopkShape s = csr_topk_shape(m, nonzeros[l], static_cast<int>(sizeof(U)), 1);
    const int* q = w.quotas(rows_in_front);
    rows_in_front += m;
    if (m == 0 || capacity[l] == 0) continue;   // (nothing of this layer is kept)
    hipLaunchKernelGGL((csr_topk_total_fill_kernel<U>), dim3(s.rows_grid), dim3(kBuildBlock), 0, stream, m,
                       nonzeros[l], s.rows_per_wave, row_offsets[l], column_indices[l],
                       static_cast<const U*>(values[l]), w.threshold, q, out_offsets[l], capacity[l], out_columns[l],
                       static_cast<U*>(out_values[l]), out_source[l]);
  }
  return launch_status();
}

// ---------------------------------------------------------------------------
// Matrix-wide drop-and-grow of a CSR topology (sputnik_hip_csr_regrow_total): the matrix keeps the
// nnz - d entries of largest value key and takes the d positions outside them of largest clamped
// score key.  The two total selections above composed, nothing read back: nnz does not change,
// so every size is known before the first launch.
//   clear    the global bins of both selections (a kernel: every replay of a captured call)
//   values   the digit passes of sputnik_hip_csr_topk's total mode over the flat values array with
//            count nnz - d, its rows launch and its scan: T_v, the rows' quotas q_r and the scanned
//            kept lengths
//   planes   per row, mark_row_planes under (T_v, q_r) in LDS, then both planes go to the
//            workspace, every word stored by the lanes that own the row.  Written ONCE and read by
//            the launches below (2 * m * ceil(n / 32) words, 1 MiB at 2048 x 2048) rather than
//            rebuilt in LDS by each of them: a rebuild is another walk of the row's entries and two
//            more barriers in up to six launches, and LDS next to the per-row bins would bound n
//            lower.
//   scores   the digit passes of the dense total mode over the score rows with count d, the kept
//            plane as the open mask and the keys clamped; a rows launch that counts the open
//            columns above and at T_s and adds the row's kept length; the scan: the quotas in
//            row-major order and the new row_offsets
//   fill     regrow_fill_row per row into [new_offsets[r], new_offsets[r + 1]), then the row order
// LDS of the planes launch: 2 * ceil(n / 32) words per row; four rows (one per wave) fit 64 KiB up
// to n = kRegrowTotalMaxN.
// ---------------------------------------------------------------------------
constexpr int kRegrowTotalMaxN = 32 * (kRegrowLdsBytes / kBuildWaves / 8);
static_assert(kRegrowTotalMaxN >= kRegrowMaxN, "no narrower than the per-row kernel");

struct RegrowTotalShape {
  int status = 0;
  int served = 0, max_m = kOrderLargeRows, max_n = kRegrowTotalMaxN;
  int rows_per_wave = -1, elements_per_lane = -1, rows_per_workgroup = -1;
  int value_passes = -1, score_passes = -1, words = -1, lds_bytes = -1, grid = -1, launches = -1;
  CsrTopkShape values;   // the launches over the old entries
};
inline RegrowTotalShape regrow_total_shape(int m, int n, int nonzeros, int score_bytes, int value_bytes) {
  RegrowTotalShape r;
  if ((score_bytes != 2 && score_bytes != 4) || nonzeros < 0) {
    r.status = SPUTNIK_HIP_INVALID_ARGUMENT;
    return r;
  }
  r.values = csr_topk_shape(m, nonzeros, value_bytes, 1);
  const BuildShape walk = build_shape(1, m, n, score_bytes);
  r.status = r.values.status != 0 ? r.values.status : walk.status;
  if (r.status != 0 || !r.values.served || n > kRegrowTotalMaxN) return r;
  r.served = 1;
  r.rows_per_wave = walk.rows_per_wave;
  r.elements_per_lane = walk.elements_per_lane;
  r.rows_per_workgroup = walk.rows_per_workgroup;
  r.value_passes = r.values.digit_passes;
  r.score_passes = score_bytes * 8 / kDigitBits;
  r.words = n / 32 + (n % 32 != 0 ? 1 : 0);
  r.lds_bytes = r.rows_per_workgroup * 2 * r.words * static_cast<int>(sizeof(unsigned));
  r.grid = walk.grid;
  // clear; values: digits, rows, scan; planes; scores: digits, rows, scan; fill; row order
  r.launches = m > 0 && nonzeros > 0 ? 1 + (r.value_passes + 2) + 1 + (r.score_passes + 2) + 1 + 1 : (m > 0 ? 1 : 0);
  return r;
}

// The workspace, in 32-bit words: the total workspace of the values, that of the scores, the
// scanned kept lengths [m + 1], the planes [m][2][words] (a row's old plane, then its kept one).
struct RegrowTotalWorkspace {
  TotalWorkspace values, scores;
  int* kept_offsets;
  unsigned* planes;
  static size_t words(int64_t m, int64_t plane_words) {
    return 2 * TotalWorkspace::words(m, false) + static_cast<size_t>(m) + 1 +
           2 * static_cast<size_t>(m) * static_cast<size_t>(plane_words);
  }
  RegrowTotalWorkspace(void* workspace, int m)
      : values(workspace, false),
        scores(static_cast<unsigned*>(workspace) + TotalWorkspace::words(m, false), false),
        kept_offsets(reinterpret_cast<int*>(static_cast<unsigned*>(workspace) + 2 * TotalWorkspace::words(m, false))),
        planes(reinterpret_cast<unsigned*>(kept_offsets + m + 1)) {}
};

// A row's planes in the workspace; a group without a row has planes of no words (plane_bits
// reads nothing then).
struct RowPlanes {
  const unsigned *old_bits, *kept_bits;
  int words;
  __device__ __forceinline__ RowPlanes(const unsigned* __restrict__ planes, int words_, int64_t row, bool live) {
    words = live ? words_ : 0;
    old_bits = planes + (live ? row * 2 * words_ : int64_t{0});
    kept_bits = old_bits + words;
  }
};

// The global bins of both selections start at zero.
__global__ __launch_bounds__(kScanBlock) void regrow_total_clear_kernel(unsigned* __restrict__ value_bins,
                                                                        unsigned* __restrict__ score_bins) {
  value_bins[threadIdx.x] = 0u;
  score_bins[threadIdx.x] = 0u;
}

// The old and the kept columns of every row under (T_v, q_r), marked in LDS and written out.
template <typename W>
__global__ __launch_bounds__(kBuildBlock) void regrow_total_planes_kernel(
    int m, int n, int nonzeros, int rows_per_wave, int words, const int* __restrict__ row_offsets,
    const int* __restrict__ column_indices, const W* __restrict__ values, const unsigned* __restrict__ threshold,
    const int* __restrict__ quotas, unsigned* __restrict__ planes) {
  extern __shared__ unsigned regrow_lds[];   // per row: old bits [words], kept bits [words]
  const RowGroup g(rows_per_wave);
  const bool live = g.row < m;
  unsigned* __restrict__ old_bits = regrow_lds + g.slot * 2 * words;
  unsigned* __restrict__ kept_bits = old_bits + words;
  int begin, end;
  row_slots(row_offsets, g.row, live, nonzeros, &begin, &end);
  mark_row_planes(g, begin, end, n, {*threshold, live ? quotas[g.row] : 0}, column_indices, values, old_bits,
                  kept_bits, words);
  if (live) {
    unsigned* __restrict__ out = planes + g.row * 2 * words;
    for (int j = g.group_lane; j < 2 * words; j += g.group_lanes) out[j] = old_bits[j];
  }
}

// One digit pass over the score rows outside the kept columns, keys clamped.
template <typename Scores>
__global__ __launch_bounds__(kBuildBlock) void regrow_total_hist_kernel(
    int m, int n, int rows_per_wave, int words, int pass, unsigned count, unsigned key_limit, Scores scores,
    const unsigned* __restrict__ planes, unsigned* bins) {
  using Walk = typename Scores::Walk;
  constexpr int P = sizeof(typename Walk::Element) * 8 / kDigitBits;
  workgroup_digit_pass<P>(pass, count, bins, [&](int shift, unsigned prefix, unsigned* hist) {
    const RowGroup g(rows_per_wave);
    const Walk walk = scores.walk(g, m, n, false);
    const RowPlanes row(planes, words, g.row, walk.live);
    digit_histogram(walk, shift, prefix, hist, key_limit,
                    [&](int64_t c0) { return ~plane_bits(row.kept_bits, row.words, c0); });
  });
}

// out_offsets[row + 1] = the row's kept length + #(open key > T_s), ties[row] = #(open key == T_s).
template <typename Scores>
__global__ __launch_bounds__(kBuildBlock) void regrow_total_rows_kernel(
    int m, int n, int rows_per_wave, int words, unsigned count, unsigned key_limit, Scores scores,
    const unsigned* __restrict__ planes, const int* __restrict__ kept_offsets,
    const unsigned* __restrict__ bins, int* __restrict__ out_offsets, int* __restrict__ ties) {
  const RowGroup g(rows_per_wave);
  const typename Scores::Walk walk = scores.walk(g, m, n, false);
  const RowPlanes row(planes, words, g.row, walk.live);
  const int kept = walk.live ? kept_offsets[g.row + 1] - kept_offsets[g.row] : 0;
  count_against_total(g, walk, count, bins, key_limit,
                      [&](int64_t c0) { return ~plane_bits(row.kept_bits, row.words, c0); }, kept, out_offsets + 1,
                      ties);
}

// The new rows under the one score threshold and the rows' quotas; generated scores publish
// their state here.
template <typename Scores, typename W>
__global__ __launch_bounds__(kBuildBlock) void regrow_total_fill_kernel(
    int m, int n, int nonzeros, int rows_per_wave, int words, unsigned key_limit,
    const int* __restrict__ row_offsets, const W* __restrict__ values, Scores scores,
    const unsigned* __restrict__ planes, const unsigned* __restrict__ threshold,
    const int* __restrict__ quotas, const int* __restrict__ out_offsets, int* __restrict__ out_columns,
    W* __restrict__ out_values, int64_t* __restrict__ out_source) {
  const RowGroup g(rows_per_wave);
  const typename Scores::Walk walk = scores.walk(g, m, n, blockIdx.x == 0 && threadIdx.x == 0);
  const RowPlanes row(planes, words, g.row, walk.live);
  int begin, end;
  row_slots(row_offsets, g.row, walk.live, nonzeros, &begin, &end);
  int64_t out, out_end;
  new_slots(out_offsets, g.row, walk.live, nonzeros, &out, &out_end);
  regrow_fill_row(g, walk, row.old_bits, row.kept_bits, row.words, {*threshold, walk.live ? quotas[g.row] : 0},
                  key_limit, begin, end, out, out_end, values, out_columns, out_values, out_source,
                  scores.template grown<W>(walk));
}

// `scores` serves the digit passes and the rows launch, `fill_scores` (the same scores, with what
// a grown slot stores) the fill.
template <typename Scores, typename FillScores, typename W>
int launch_regrow_total(const RegrowTotalShape& r, int m, int n, int nonzeros, const int* row_offsets,
                        const int* column_indices, const void* values_, unsigned drop, const Scores& scores,
                        const FillScores& fill_scores, unsigned key_limit, void* workspace, int* out_offsets,
                        int* out_columns, void* out_values, int64_t* out_source, hipStream_t stream) {
  const W* values = static_cast<const W*>(values_);
  const RegrowTotalWorkspace w(workspace, m);
  const dim3 block(kBuildBlock), grid(r.grid), entry_grid(r.values.rows_grid);
  const unsigned keep = static_cast<unsigned>(nonzeros) - drop;
  hipLaunchKernelGGL(regrow_total_clear_kernel, dim3(1), dim3(kScanBlock), 0, stream, w.values.bins, w.scores.bins);
  for (int p = 0; p < r.value_passes; ++p)
    hipLaunchKernelGGL((csr_topk_flat_hist_kernel<W>), dim3(r.values.flat_grid), block, 0, stream, nonzeros, p, keep,
                       values, w.values.bins);
  hipLaunchKernelGGL((csr_topk_total_rows_kernel<W>), entry_grid, block, 0, stream, m, nonzeros,
                     r.values.rows_per_wave, keep, row_offsets, values, w.values.bins, w.kept_offsets,
                     w.values.quotas() + m);
  launch_total_scan(w.values, w.values.quotas(), m, r.value_passes, keep, w.kept_offsets, true, nullptr, stream);
  hipLaunchKernelGGL((regrow_total_planes_kernel<W>), grid, block, r.lds_bytes, stream, m, n, nonzeros,
                     r.rows_per_wave, r.words, row_offsets, column_indices, values, w.values.threshold,
                     w.values.quotas(), w.planes);
  for (int p = 0; p < r.score_passes; ++p)
    hipLaunchKernelGGL((regrow_total_hist_kernel<Scores>), grid, block, 0, stream, m, n, r.rows_per_wave, r.words, p,
                       drop, key_limit, scores, w.planes, w.scores.bins);
  hipLaunchKernelGGL((regrow_total_rows_kernel<Scores>), grid, block, 0, stream, m, n, r.rows_per_wave, r.words, drop,
                     key_limit, scores, w.planes, w.kept_offsets, w.scores.bins, out_offsets,
                     w.scores.quotas() + m);
  launch_total_scan(w.scores, w.scores.quotas(), m, r.score_passes, drop, out_offsets, true, nullptr, stream);
  hipLaunchKernelGGL((regrow_total_fill_kernel<FillScores, W>), grid, block, 0, stream, m, n, nonzeros, r.rows_per_wave,
                     r.words, key_limit, row_offsets, values, fill_scores, w.planes, w.scores.threshold,
                     w.scores.quotas(), out_offsets, out_columns, static_cast<W*>(out_values), out_source);
  return launch_status();
}

// ---------------------------------------------------------------------------
// A uniformly random CSR topology with its initial values (sputnik_hip_random_csr): the top-k
// selection above over a key matrix that never exists.  With the Philox4x32-10 of philox.h,
// replica = row and entry = column,
//   key(r, c)   = philox(seed, counter (offset/4, c >> 2, r))[c & 3] & key_mask
//   value(r, c) = float(int(philox(seed, counter (offset/4, c >> 2, r | 2^31))[c & 3] >> 8) - 2^23) * scale
// rounded to nearest even into the values type.  KeyWalk computes a piece of four keys with one
// Philox call where RowWalk loads one, and radix_select, digit_histogram, count_against_total
// and fill_row run on it as they run on memory: the Selection, the tie rule and the row order
// are those of the dense top-k.
//   per row   ONE launch: the group of lanes that walks a row selects it (four digit passes in
//             its LDS bins), fills its columns and values and writes its offset r * k and its
//             place r in the row order
//   total     the launches of the dense total mode on generated keys: clear, four digit passes,
//             rows, scan, a fill that also writes the values, the row order -- nine
// A key is recomputed per pass instead of stored: 5 Philox calls per four columns and no
// [m, n] array.  The resolved {seed, offset} is published by one lane of one launch.
// ---------------------------------------------------------------------------
constexpr int kKeyDigitPasses = 4;   // 32-bit keys

struct RandomArgs {
  DropArgs state;      // the Philox state and where it is published (threshold, scale unused)
  unsigned key_mask;   // at most 0x7fffffff
  float scale;         // bound / 2^23
};

// One group of lanes on one row of n generated keys.  No lead: a piece starts at a multiple of 4.
struct KeyWalk {
  using Element = uint32_t;
  static constexpr int V = 4;
  PhiloxKey key;
  unsigned key_mask, row;
  bool live;
  int n, steps, group_lanes, group_lane;

  __device__ __forceinline__ KeyWalk(const RowGroup& g, const PhiloxKey& key_, unsigned key_mask_, int m, int n_) {
    key = key_;
    key_mask = key_mask_;
    group_lanes = g.group_lanes;
    group_lane = g.group_lane;
    live = g.row < m;
    row = static_cast<unsigned>(g.row);
    n = n_;
    const int64_t span = static_cast<int64_t>(group_lanes) * V;
    steps = static_cast<int>((static_cast<int64_t>(n_) + span - 1) / span);
  }
  // My piece of step s, its first column, and a bit per key that lies inside the row.
  __device__ __forceinline__ Piece<uint32_t> load(int s, int64_t* first_column, unsigned* valid) const {
    const int64_t c0 = (static_cast<int64_t>(s) * group_lanes + group_lane) * V;
    *first_column = c0;
    Piece<uint32_t> v = {{0u, 0u, 0u, 0u}};
    unsigned in = 0;
    if (live && c0 < n) {
      const uint4 w = philox4x32_10(key, static_cast<unsigned>(c0 >> 2), row);
      v.e[0] = w.x & key_mask;
      v.e[1] = w.y & key_mask;
      v.e[2] = w.z & key_mask;
      v.e[3] = w.w & key_mask;
      const int64_t inside = static_cast<int64_t>(n) - c0;
      in = inside >= V ? (1u << V) - 1u : (1u << inside) - 1u;
    }
    *valid = in;
    return v;
  }
};

template <typename T>
__device__ __forceinline__ T random_value(unsigned word, float scale) {
  const float x = static_cast<float>(static_cast<int>(word >> 8) - (1 << 23)) * scale;
  return static_cast<T>(x);
}

// fill_row over a row of generated keys: a kept column and its value.  The value words of a
// piece are drawn once, for its first kept column.
template <typename T>
__device__ __forceinline__ void random_fill_row(const RowGroup& g, const KeyWalk& walk, Selection kept, int64_t out,
                                                int64_t end, float scale, int* __restrict__ column_indices,
                                                T* __restrict__ values) {
  int64_t drawn = -1;
  uint4 words = make_uint4(0u, 0u, 0u, 0u);
  fill_row(g, walk, kept, out, end, [&](int64_t p, int64_t column, uint32_t) {
    const int64_t piece = column >> 2;
    if (piece != drawn) {
      words = philox4x32_10(walk.key, static_cast<unsigned>(piece), walk.row | 0x80000000u);
      drawn = piece;
    }
    column_indices[p] = static_cast<int>(column);
    values[p] = random_value<T>(uint4_word(words, static_cast<int>(column & 3)), scale);
  });
}

// Per-row mode: select and fill of every row, its offset and its place in the row order.
template <typename T>
__global__ __launch_bounds__(kBuildBlock) void random_rows_kernel(
    int m, int n, int rows_per_wave, int k, RandomArgs args, int* __restrict__ row_offsets,
    int* __restrict__ row_indices, int* __restrict__ column_indices, T* __restrict__ values) {
  __shared__ unsigned hist[kBuildWaves * kMaxRowsPerWave][kDigitBins];   // 64 KiB
  const PhiloxKey key = philox_key(args.state, blockIdx.x == 0 && threadIdx.x == 0);
  const RowGroup g(rows_per_wave);
  const KeyWalk walk(g, key, args.key_mask, m, n);
  const Selection kept = radix_select<kKeyDigitPasses>(g, hist[g.slot], k,
                                                       [&](int shift, unsigned prefix, unsigned* bins) {
                                                         digit_histogram(walk, shift, prefix, bins);
                                                       });
  const int64_t out = g.row * k;
  if (walk.live && g.group_lane == 0) {
    row_offsets[g.row] = static_cast<int>(out);
    row_indices[g.row] = static_cast<int>(g.row);
    if (g.row == m - 1) row_offsets[m] = static_cast<int>(out + k);
  }
  random_fill_row(g, walk, kept, walk.live ? out : 0, walk.live ? out + k : 0, args.scale, column_indices, values);
}

// Total mode, one digit pass over the generated keys: this workgroup's rows.
__global__ __launch_bounds__(kBuildBlock) void random_total_hist_kernel(int m, int n, int rows_per_wave, int pass,
                                                                       unsigned count, RandomArgs args,
                                                                       unsigned* bins) {
  const PhiloxKey key = philox_key(args.state, false);
  workgroup_digit_pass<kKeyDigitPasses>(pass, count, bins, [&](int shift, unsigned prefix, unsigned* hist) {
    const RowGroup g(rows_per_wave);
    const KeyWalk walk(g, key, args.key_mask, m, n);
    digit_histogram(walk, shift, prefix, hist);
  });
}

// Total mode: row_offsets[row + 1] = #(key > T), ties[row] = #(key == T).
__global__ __launch_bounds__(kBuildBlock) void random_total_rows_kernel(
    int m, int n, int rows_per_wave, unsigned count, RandomArgs args, const unsigned* __restrict__ bins,
    int* __restrict__ row_offsets, int* __restrict__ ties) {
  const PhiloxKey key = philox_key(args.state, false);
  const RowGroup g(rows_per_wave);
  const KeyWalk walk(g, key, args.key_mask, m, n);
  count_against_total(g, walk, count, bins, row_offsets + 1, ties);
}

// Total mode: the fill of every row under the one threshold and the rows' quotas; publishes the state.
template <typename T>
__global__ __launch_bounds__(kBuildBlock) void random_total_fill_kernel(
    int m, int n, int rows_per_wave, int64_t capacity, RandomArgs args, const unsigned* __restrict__ threshold,
    const int* __restrict__ quotas, const int* __restrict__ row_offsets, int* __restrict__ column_indices,
    T* __restrict__ values) {
  const PhiloxKey key = philox_key(args.state, blockIdx.x == 0 && threadIdx.x == 0);
  const RowGroup g(rows_per_wave);
  const KeyWalk walk(g, key, args.key_mask, m, n);
  int64_t out, end;
  new_slots(row_offsets, g.row, walk.live, capacity, &out, &end);
  random_fill_row(g, walk, {*threshold, walk.live ? quotas[g.row] : 0}, out, end, args.scale, column_indices, values);
}

struct RandomShape {
  int status = 0;
  int served = 0, launches = 0;
  BuildShape walk;
};
inline RandomShape random_shape(int m, int n, int total_mode) {
  RandomShape r;
  if (total_mode != 0 && total_mode != 1) {
    r.status = SPUTNIK_HIP_INVALID_ARGUMENT;
    return r;
  }
  r.walk = build_shape(1, m, n, static_cast<int>(sizeof(uint32_t)));
  r.status = r.walk.status;
  if (r.status != 0) return r;
  r.served = total_mode ? order_route(1, m, n).served : 1;
  // total: clear, digits, rows, scan, fill, row order
  r.launches = total_mode ? 1 + kKeyDigitPasses + 4 : 1;
  return r;
}

template <typename T>
int launch_random(const RandomShape& r, int m, int n, int total_mode, unsigned count, const RandomArgs& args,
                  void* workspace, int* row_indices, int* row_offsets, int* column_indices, void* values_,
                  hipStream_t stream) {
  T* values = static_cast<T*>(values_);
  const int rows = r.walk.rows_per_wave;
  const dim3 grid(r.walk.grid), block(kBuildBlock);
  if (!total_mode) {
    hipLaunchKernelGGL((random_rows_kernel<T>), grid, block, 0, stream, m, n, rows, static_cast<int>(count), args,
                       row_offsets, row_indices, column_indices, values);
    return launch_status();
  }
  const TotalWorkspace w(workspace, false);
  launch_digit_passes(w.bins, kKeyDigitPasses, stream, [&](int p) {
    hipLaunchKernelGGL(random_total_hist_kernel, grid, block, 0, stream, m, n, rows, p, count, args, w.bins);
  });
  hipLaunchKernelGGL(random_total_rows_kernel, grid, block, 0, stream, m, n, rows, count, args, w.bins, row_offsets,
                     w.quotas() + m);
  launch_total_scan(w, w.quotas(), m, kKeyDigitPasses, count, row_offsets, true, nullptr, stream);
  hipLaunchKernelGGL((random_total_fill_kernel<T>), grid, block, 0, stream, m, n, rows, static_cast<int64_t>(count),
                     args, w.threshold, w.quotas(), row_offsets, column_indices, values);
  return launch_status();
}

// ---------------------------------------------------------------------------
// Drop-and-grow under random scores that are never stored (sputnik_hip_csr_regrow_random,
// sputnik_hip_csr_regrow_total_random): SET's step.  The regrow kernels above, instantiated on
// KeyScores where the RigL step has StoredScores: the score half walks a KeyWalk, so a score key
// is key(r, c) of the random topology under a mask of at most 30 bits -- read as float32 bits a
// finite, non-negative number, which the clamp of the regrow rule never touches.  The step is
// therefore exactly the stored one under dense float32 scores whose bits are the keys.  A key is
// recomputed per pass: per four columns of a row the per-row kernel makes 5 Philox calls (four
// digit passes and the fill), the matrix-wide step 6 (four digit launches, rows, fill), plus one
// of the value stream where a piece grows an entry and the grown entries are initialised.
//   KeyScores           the walk; a grown slot stores +0.0 (hist and rows launches, and a fill
//                       that is not asked for values)
//   KeyScoresOf<T>      a grown slot stores value(r, c) of the random topology in T, drawn once
//                       per piece of four columns as random_fill_row draws it; `draw` = 0: +0.0
// The per-row kernel and the matrix-wide fill publish the resolved state.
// ---------------------------------------------------------------------------
constexpr unsigned kRegrowKeyMask = 0x3fffffffu;

struct KeyScores {
  using Walk = KeyWalk;
  RandomArgs args;
  int draw;   // grown slots take the value stream (else +0.0)
  __device__ __forceinline__ Walk walk(const RowGroup& g, int m, int n, bool publish) const {
    return KeyWalk(g, philox_key(args.state, publish), args.key_mask, m, n);
  }
  template <typename W>
  __device__ __forceinline__ auto grown(const Walk&) const {
    return [](int64_t) { return W{0}; };
  }
};

// random_value with the float32 product held in a register before it is rounded into T.  Left
// to itself the compiler fuses a multiply and a rounding to float16 into one v_fma_mixlo_f16
// with a +0.0 addend, which turns a -0.0 product (scale = 0: grow_bound = 0) into +0.0; the
// rule says one float32 multiply, then one rounding.
template <typename T>
__device__ __forceinline__ T grown_value(unsigned word, float scale) {
  float x = static_cast<float>(static_cast<int>(word >> 8) - (1 << 23)) * scale;
  asm volatile("" : "+v"(x));
  return static_cast<T>(x);
}

// The bits of value(r, c) in T for the grown columns of one row, asked for in ascending order.
template <typename T, typename W>
struct GrownValue {
  static_assert(sizeof(T) == sizeof(W), "the values array is read as W");
  PhiloxKey key;
  unsigned row;
  float scale;
  bool draw;
  int64_t drawn;
  uint4 words;
  __device__ __forceinline__ W operator()(int64_t column) {
    if (!draw) return W{0};
    const int64_t piece = column >> 2;
    if (piece != drawn) {
      words = philox4x32_10(key, static_cast<unsigned>(piece), row | 0x80000000u);
      drawn = piece;
    }
    const T x = grown_value<T>(uint4_word(words, static_cast<int>(column & 3)), scale);
    W bits;
    __builtin_memcpy(&bits, &x, sizeof(W));
    return bits;
  }
};

template <typename T>
struct KeyScoresOf : KeyScores {
  template <typename W>
  __device__ __forceinline__ GrownValue<T, W> grown(const KeyWalk& walk) const {
    return GrownValue<T, W>{walk.key, walk.row, args.scale, draw != 0, int64_t{-1}, make_uint4(0u, 0u, 0u, 0u)};
  }
};

// f(float{}), f(_Float16{}) or f(__bf16{}) for a checked SPUTNIK_HIP_F32 / F16 / BF16.
template <typename F>
inline int by_dtype(int dtype, F f) {
  return dtype == SPUTNIK_HIP_F32 ? f(float{}) : dtype == SPUTNIK_HIP_F16 ? f(_Float16{}) : f(__bf16{});
}

inline KeyScores key_scores(const sputnik_hip_philox_state& rng, int64_t* rng_state_out, unsigned key_mask,
                            int grow_values, float grow_scale) {
  KeyScores k;
  k.args.state.rng = rng;
  k.args.state.rng_state_out = rng_state_out;
  k.args.state.threshold = 0u;
  k.args.state.scale = 0.f;
  k.args.state.replica0 = 0;
  k.args.key_mask = key_mask;
  k.args.scale = grow_scale;
  k.draw = grow_values != 0 ? 1 : 0;
  return k;
}

// What both entries check alike: the dtype, the mask, the scale and where the state goes.
inline bool key_scores_ok(int dtype, unsigned key_mask, int grow_values, float grow_scale,
                          const int64_t* rng_state_out) {
  return (dtype == SPUTNIK_HIP_F32 || dtype == SPUTNIK_HIP_F16 || dtype == SPUTNIK_HIP_BF16) &&
         key_mask <= kRegrowKeyMask && (grow_values == 0 || (grow_scale >= 0.f && grow_scale < INFINITY)) &&
         (rng_state_out == nullptr || aligned_to(rng_state_out, sizeof(int64_t)));
}

inline void put(int* p, int v) {
  if (p) *p = v;
}

}  // namespace
}  // namespace sputnik_hip

using namespace sputnik_hip;

extern "C" {

int sputnik_hip_dense_to_csr_launch_shape(int masks, int m, int n, int element_bytes, int* rows_per_wave,
                                          int* elements_per_lane, int* rows_per_workgroup, int* grid) {
  const BuildShape s = build_shape(masks, m, n, element_bytes);
  if (s.status != 0) return s.status;
  put(rows_per_wave, s.rows_per_wave);
  put(elements_per_lane, s.elements_per_lane);
  put(rows_per_workgroup, s.rows_per_workgroup);
  put(grid, s.grid);
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
  put(served, r.served);
  put(capacity, r.capacity);
  put(threads, r.threads);
  put(sort_size, r.sort_size);
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

int sputnik_hip_attention_pattern_launch_shape(int m, int n, int64_t offset, int* served, int* rows_per_wave,
                                               int* columns_per_lane, int* rows_per_workgroup, int* grid,
                                               int* launches) {
  const PatternShape s = pattern_shape(m, n, offset);
  if (s.status != 0) return s.status;
  put(served, s.served);
  put(rows_per_wave, s.served ? s.walk.rows_per_wave : -1);
  put(columns_per_lane, s.served ? s.walk.elements_per_lane : -1);
  put(rows_per_workgroup, s.served ? s.walk.rows_per_workgroup : -1);
  put(grid, s.served ? s.walk.grid : -1);
  put(launches, s.served ? kPatternLaunches : -1);
  return 0;
}

int sputnik_hip_attention_pattern_count(int m, int n, const sputnik_hip_attention_pattern_args* pattern,
                                        sputnik_hip_philox_state rng, int64_t* rng_state_out, int* row_offsets,
                                        int* nonzeros, sputnik_hip_stream_t stream_) {
  if (pattern == nullptr) return SPUTNIK_HIP_INVALID_ARGUMENT;
  const PatternShape s = pattern_shape(m, n, pattern->offset);
  if (s.status != 0) return s.status;
  if (!s.served || !pattern_ok(*pattern) || row_offsets == nullptr || !aligned_to(row_offsets, sizeof(int)) ||
      nonzeros == nullptr || !aligned_to(nonzeros, sizeof(int)) ||
      (rng_state_out != nullptr && !aligned_to(rng_state_out, sizeof(int64_t))))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const PatternArgs args = pattern_args(*pattern, rng, pattern->random_block > 0 ? rng_state_out : nullptr);
  if (s.walk.grid > 0) {
    hipLaunchKernelGGL((attention_pattern_rows_kernel<false>), dim3(s.walk.grid), dim3(kBuildBlock), 0, stream, m, n,
                       s.walk.rows_per_wave, args, 0, row_offsets, static_cast<int*>(nullptr));
  } else if (pattern->random_block > 0) {
    const int st = publish_rng_state(args.state, stream);   // (no row to publish it)
    if (st != 0) return st;
  }
  hipLaunchKernelGGL(topology_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, m, row_offsets, nonzeros);
  return launch_status();
}

int sputnik_hip_attention_pattern_fill(int m, int n, const sputnik_hip_attention_pattern_args* pattern,
                                       sputnik_hip_philox_state rng, int nonzeros, const int* row_offsets,
                                       int* row_indices, int* column_indices, sputnik_hip_stream_t stream_) {
  if (pattern == nullptr) return SPUTNIK_HIP_INVALID_ARGUMENT;
  const PatternShape s = pattern_shape(m, n, pattern->offset);
  if (s.status != 0) return s.status;
  if (!s.served || !pattern_ok(*pattern) || nonzeros < 0 || row_offsets == nullptr ||
      !aligned_to(row_offsets, sizeof(int)) ||
      (m > 0 && (row_indices == nullptr || !aligned_to(row_indices, sizeof(int)))) ||
      (nonzeros > 0 && (column_indices == nullptr || !aligned_to(column_indices, sizeof(int)))))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (s.walk.grid > 0 && nonzeros > 0) {
    const PatternArgs args = pattern_args(*pattern, rng, nullptr);
    hipLaunchKernelGGL((attention_pattern_rows_kernel<true>), dim3(s.walk.grid), dim3(kBuildBlock), 0, stream, m, n,
                       s.walk.rows_per_wave, args, nonzeros, const_cast<int*>(row_offsets), column_indices);
    const int st = launch_status();
    if (st != 0) return st;
  }
  return sputnik_hip_csr_row_order(1, m, n, row_offsets, row_indices, stream_);
}

int sputnik_hip_topk_to_csr_launch_shape(int m, int n, int element_bytes, int total_mode, int* served,
                                         int* rows_per_wave, int* elements_per_lane, int* rows_per_workgroup,
                                         int* digit_passes, int* grid) {
  const TopkShape t = topk_shape(m, n, element_bytes, total_mode);
  if (t.status != 0) return t.status;
  put(served, t.served);
  put(rows_per_wave, t.walk.rows_per_wave);
  put(elements_per_lane, t.walk.elements_per_lane);
  put(rows_per_workgroup, t.walk.rows_per_workgroup);
  put(digit_passes, t.digit_passes);
  put(grid, t.walk.grid);
  return 0;
}

size_t sputnik_hip_topk_to_csr_workspace_bytes(int m, int n, int total_mode) {
  if (m < 0 || n < 0) return 0;
  return sizeof(unsigned) * topk_workspace_words(m, total_mode != 0);
}

int sputnik_hip_topk_to_csr(int m, int n, const void* scores, int element_bytes, int64_t row_stride,
                            int total_mode, int64_t count, const void* values_from, int value_bytes,
                            int64_t values_row_stride, void* workspace, size_t workspace_bytes,
                            int* row_indices, int* row_offsets, int* column_indices, void* values,
                            sputnik_hip_stream_t stream_) {
  const TopkShape t = topk_shape(m, n, element_bytes, total_mode);
  if (t.status != 0) return t.status;
  if (!t.served) return SPUTNIK_HIP_INVALID_ARGUMENT;
  const int64_t most = total_mode ? static_cast<int64_t>(m) * n : n;
  if (count < 0 || count > most || row_offsets == nullptr) return SPUTNIK_HIP_INVALID_ARGUMENT;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (m == 0) return static_cast<int>(hipMemsetAsync(row_offsets, 0, sizeof(int), stream));
  const int64_t nonzeros = total_mode ? count : count * m;
  if (row_indices == nullptr || (nonzeros > 0 && column_indices == nullptr) ||
      (n > 0 && !dense_ok(scores, element_bytes, 0, row_stride)) || workspace == nullptr ||
      !aligned_to(workspace, sizeof(unsigned)) ||
      workspace_bytes < sizeof(unsigned) * topk_workspace_words(m, total_mode))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  if (values != nullptr &&
      ((value_bytes != 2 && value_bytes != 4) || values_row_stride < 0 || !aligned_to(values, value_bytes) ||
       (nonzeros > 0 && (values_from == nullptr || !aligned_to(values_from, value_bytes)))))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  const int st = by_width(element_bytes, [&](auto u) {
    return launch_topk<decltype(u)>(t, m, n, scores, row_stride, total_mode, static_cast<unsigned>(count), values_from,
                                    value_bytes, values_row_stride, static_cast<unsigned*>(workspace), row_indices,
                                    row_offsets, column_indices, values, stream);
  });
  if (st != 0 || !total_mode) return st;
  return sputnik_hip_csr_row_order(1, m, n, row_offsets, row_indices, stream_);
}

int sputnik_hip_csr_regrow_launch_shape(int m, int n, int score_bytes, int value_bytes, int* served,
                                        int* rows_per_wave, int* elements_per_lane, int* rows_per_workgroup,
                                        int* value_digit_passes, int* score_digit_passes, int* lds_bytes,
                                        int* max_n, int* grid) {
  const RegrowShape r = regrow_shape(m, n, score_bytes, value_bytes);
  if (r.status != 0) return r.status;
  put(served, r.served);
  put(rows_per_wave, r.rows_per_wave);
  put(elements_per_lane, r.elements_per_lane);
  put(rows_per_workgroup, r.rows_per_workgroup);
  put(value_digit_passes, r.value_passes);
  put(score_digit_passes, r.score_passes);
  put(lds_bytes, r.lds_bytes);
  put(max_n, r.max_n);
  put(grid, r.grid);
  return 0;
}

size_t sputnik_hip_csr_regrow_workspace_bytes(int m, int n, int nonzeros) {
  return 0;   // one launch: what its phases hand each other stays in registers and LDS
}

int sputnik_hip_csr_regrow(int m, int n, int nonzeros, const int* row_offsets, const int* column_indices,
                           const void* values, int value_bytes, const int* drop_counts, const void* scores,
                           int score_bytes, int64_t scores_row_stride, unsigned score_key_limit,
                           void* workspace, size_t workspace_bytes, int* out_column_indices, void* out_values,
                           int64_t* out_source, sputnik_hip_stream_t stream_) {
  const RegrowShape r = regrow_shape(m, n, score_bytes, value_bytes);
  if (r.status != 0) return r.status;
  if (!r.served || nonzeros < 0 || scores_row_stride < 0 ||
      score_key_limit >= (1u << (8 * score_bytes - 1)))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  if (m == 0 || nonzeros == 0) return 0;
  if (row_offsets == nullptr || column_indices == nullptr || drop_counts == nullptr || values == nullptr ||
      !aligned_to(values, value_bytes) || scores == nullptr || !aligned_to(scores, score_bytes) ||
      out_column_indices == nullptr || out_values == nullptr || !aligned_to(out_values, value_bytes) ||
      out_source == nullptr || !aligned_to(out_source, sizeof(int64_t)) ||
      !aligned_to(row_offsets, sizeof(int)) || !aligned_to(column_indices, sizeof(int)) ||
      !aligned_to(drop_counts, sizeof(int)) || !aligned_to(out_column_indices, sizeof(int)))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  return by_width(score_bytes, [&](auto s) {
    return by_width(value_bytes, [&](auto w) {
      using S = decltype(s);
      const StoredScores<S> stored = {static_cast<const S*>(scores), scores_row_stride};
      return launch_regrow<StoredScores<S>, decltype(w)>(r, m, n, nonzeros, row_offsets, column_indices, values,
                                                         drop_counts, stored, score_key_limit, out_column_indices,
                                                         out_values, out_source, stream);
    });
  });
}

int sputnik_hip_csr_regrow_total_launch_shape(int m, int n, int nonzeros, int score_bytes, int value_bytes,
                                              int* served, int* rows_per_wave, int* elements_per_lane,
                                              int* rows_per_workgroup, int* value_digit_passes,
                                              int* score_digit_passes, int* lds_bytes, int* max_m, int* max_n,
                                              int* grid, int* value_rows_per_wave, int* value_rows_grid,
                                              int* flat_grid, int* launches) {
  const RegrowTotalShape r = regrow_total_shape(m, n, nonzeros, score_bytes, value_bytes);
  if (r.status != 0) return r.status;
  put(served, r.served);
  put(rows_per_wave, r.rows_per_wave);
  put(elements_per_lane, r.elements_per_lane);
  put(rows_per_workgroup, r.rows_per_workgroup);
  put(value_digit_passes, r.value_passes);
  put(score_digit_passes, r.score_passes);
  put(lds_bytes, r.lds_bytes);
  put(max_m, r.max_m);
  put(max_n, r.max_n);
  put(grid, r.grid);
  put(value_rows_per_wave, r.served ? r.values.rows_per_wave : -1);
  put(value_rows_grid, r.served ? r.values.rows_grid : -1);
  put(flat_grid, r.served ? r.values.flat_grid : -1);
  put(launches, r.launches);
  return 0;
}

size_t sputnik_hip_csr_regrow_total_workspace_bytes(int m, int n, int nonzeros) {
  if (m < 0 || n < 0 || nonzeros < 0) return 0;
  return sizeof(unsigned) * RegrowTotalWorkspace::words(m, n / 32 + (n % 32 != 0 ? 1 : 0));
}

int sputnik_hip_csr_regrow_total(int m, int n, int nonzeros, const int* row_offsets, const int* column_indices,
                                 const void* values, int value_bytes, int64_t drop, const void* scores,
                                 int score_bytes, int64_t scores_row_stride, unsigned score_key_limit,
                                 void* workspace, size_t workspace_bytes, int* out_row_indices,
                                 int* out_row_offsets, int* out_column_indices, void* out_values,
                                 int64_t* out_source, sputnik_hip_stream_t stream_) {
  const RegrowTotalShape r = regrow_total_shape(m, n, nonzeros, score_bytes, value_bytes);
  if (r.status != 0) return r.status;
  if (!r.served || drop < 0 || drop > nonzeros || scores_row_stride < 0 ||
      score_key_limit >= (1u << (8 * score_bytes - 1)) || out_row_offsets == nullptr ||
      !aligned_to(out_row_offsets, sizeof(int)) ||
      (m > 0 && (out_row_indices == nullptr || !aligned_to(out_row_indices, sizeof(int)))))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (m == 0 || nonzeros == 0) {
    // no entries: the zero offsets and the row order 0 .. m - 1 of equal lengths
    if (hipMemsetAsync(out_row_offsets, 0, sizeof(int) * (static_cast<size_t>(m) + 1), stream) != hipSuccess)
      return launch_status();
    if (m == 0) return launch_status();
    return sputnik_hip_csr_row_order(1, m, n, out_row_offsets, out_row_indices, stream_);
  }
  if (row_offsets == nullptr || !aligned_to(row_offsets, sizeof(int)) || column_indices == nullptr ||
      !aligned_to(column_indices, sizeof(int)) || values == nullptr || !aligned_to(values, value_bytes) ||
      scores == nullptr || !aligned_to(scores, score_bytes) || out_column_indices == nullptr ||
      !aligned_to(out_column_indices, sizeof(int)) || out_values == nullptr || !aligned_to(out_values, value_bytes) ||
      out_source == nullptr || !aligned_to(out_source, sizeof(int64_t)) || workspace == nullptr ||
      !aligned_to(workspace, sizeof(unsigned)) ||
      workspace_bytes < sputnik_hip_csr_regrow_total_workspace_bytes(m, n, nonzeros))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  const int st = by_width(score_bytes, [&](auto s) {
    return by_width(value_bytes, [&](auto w) {
      using S = decltype(s);
      const StoredScores<S> stored = {static_cast<const S*>(scores), scores_row_stride};
      return launch_regrow_total<StoredScores<S>, StoredScores<S>, decltype(w)>(
          r, m, n, nonzeros, row_offsets, column_indices, values, static_cast<unsigned>(drop), stored, stored,
          score_key_limit, workspace, out_row_offsets, out_column_indices, out_values, out_source, stream);
    });
  });
  if (st != 0) return st;
  return sputnik_hip_csr_row_order(1, m, n, out_row_offsets, out_row_indices, stream_);
}

int sputnik_hip_csr_topk_launch_shape(int m, int n, int nonzeros, int value_bytes, int total_mode, int* served,
                                      int* rows_per_wave, int* group_lanes, int* elements_per_lane,
                                      int* rows_per_workgroup, int* digit_passes, int* rows_grid, int* flat_grid) {
  if (n < 0) return SPUTNIK_HIP_INVALID_ARGUMENT;
  const CsrTopkShape s = csr_topk_shape(m, nonzeros, value_bytes, total_mode);
  if (s.status != 0) return s.status;
  put(served, s.served);
  put(rows_per_wave, s.rows_per_wave);
  put(group_lanes, s.group_lanes);
  put(elements_per_lane, s.elements_per_lane);
  put(rows_per_workgroup, s.rows_per_workgroup);
  put(digit_passes, s.digit_passes);
  put(rows_grid, s.rows_grid);
  put(flat_grid, s.flat_grid);
  return 0;
}

size_t sputnik_hip_csr_topk_workspace_bytes(int m, int n, int nonzeros, int total_mode) {
  if (m < 0 || n < 0 || nonzeros < 0 || !total_mode) return 0;   // per row: registers and LDS only
  return sizeof(unsigned) * topk_workspace_words(m, 1);
}

int sputnik_hip_csr_topk(int m, int n, int nonzeros, const int* row_offsets, const int* column_indices,
                         const void* values, int value_bytes, int total_mode, int64_t count, void* workspace,
                         size_t workspace_bytes, int* out_row_indices, int* out_row_offsets,
                         int* out_column_indices, void* out_values, int64_t* out_source, int64_t out_capacity,
                         sputnik_hip_stream_t stream_) {
  if (n < 0) return SPUTNIK_HIP_INVALID_ARGUMENT;
  const CsrTopkShape s = csr_topk_shape(m, nonzeros, value_bytes, total_mode);
  if (s.status != 0) return s.status;
  if (!s.served || count < 0 || count > (total_mode ? static_cast<int64_t>(nonzeros) : static_cast<int64_t>(n)) ||
      out_capacity < 0 || out_row_offsets == nullptr || !aligned_to(out_row_offsets, sizeof(int)))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  const bool empty = m == 0 || nonzeros == 0 || count == 0;
  // per-row mode in two halves: no columns = offsets and row order only; columns but no
  // row_indices = the fill under the offsets a former call wrote.  Total mode is one call.
  const bool fill = total_mode || out_column_indices != nullptr;
  const bool offsets = total_mode || !fill || out_row_indices != nullptr;
  if ((m > 0 && offsets && out_row_indices == nullptr) ||
      (out_row_indices != nullptr && !aligned_to(out_row_indices, sizeof(int))) ||
      (total_mode && out_capacity < count))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  if (fill && !empty &&
      (out_column_indices == nullptr || !aligned_to(out_column_indices, sizeof(int)) || out_values == nullptr ||
       !aligned_to(out_values, value_bytes) || out_source == nullptr || !aligned_to(out_source, sizeof(int64_t))))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!empty) {
    if (row_offsets == nullptr || !aligned_to(row_offsets, sizeof(int)) ||
        (fill && (column_indices == nullptr || !aligned_to(column_indices, sizeof(int)) || values == nullptr ||
                  !aligned_to(values, value_bytes))))
      return SPUTNIK_HIP_INVALID_ARGUMENT;
    const size_t ws_bytes = sputnik_hip_csr_topk_workspace_bytes(m, n, nonzeros, total_mode);
    if (ws_bytes > 0 && (workspace == nullptr || !aligned_to(workspace, sizeof(unsigned)) || workspace_bytes < ws_bytes))
      return SPUTNIK_HIP_INVALID_ARGUMENT;
  }
  if (empty) {
    // nothing is kept: the zero offsets and the row order 0 .. m - 1 of equal lengths
    if (offsets && hipMemsetAsync(out_row_offsets, 0, sizeof(int) * (static_cast<size_t>(m) + 1), stream) != hipSuccess)
      return launch_status();
  } else {
    const int st = by_width(value_bytes, [&](auto u) {
      return launch_csr_topk<decltype(u)>(s, m, nonzeros, row_offsets, column_indices, values, total_mode,
                                          static_cast<unsigned>(count), offsets, fill, workspace, out_row_offsets,
                                          out_capacity, out_column_indices, out_values, out_source, stream);
    });
    if (st != 0) return st;
  }
  if (out_row_indices == nullptr || m == 0) return launch_status();
  return sputnik_hip_csr_row_order(1, m, n, out_row_offsets, out_row_indices, stream_);
}

int sputnik_hip_csr_topk_global_launch_shape(int layers, const int* rows, const int* nonzeros, int value_bytes,
                                             int* served, int* digit_passes, int* layers_per_launch,
                                             int* elements_per_workgroup, int* digit_launches) {
  const GlobalTopkShape g = global_topk_shape(layers, rows, nonzeros, value_bytes);
  if (g.status != 0) return g.status;
  put(served, g.served);
  put(digit_passes, g.digit_passes);
  put(layers_per_launch, g.layers_per_launch);
  put(elements_per_workgroup, g.elements_per_workgroup);
  put(digit_launches, g.digit_launches);
  return 0;
}

size_t sputnik_hip_csr_topk_global_workspace_bytes(int layers, const int* rows) {
  if (layers < 0 || (layers > 0 && rows == nullptr)) return 0;
  int64_t all = 0;
  for (int l = 0; l < layers; ++l) {
    if (rows[l] < 0) return 0;
    all += rows[l];
  }
  return sizeof(unsigned) * global_topk_workspace_words(all);
}

int sputnik_hip_csr_topk_global_select(int layers, const int* rows, const int* nonzeros,
                                       const int* const* row_offsets, const void* const* values, int value_bytes,
                                       int64_t count, void* workspace, size_t workspace_bytes,
                                       int* const* out_row_offsets, int* out_nonzeros, sputnik_hip_stream_t stream_) {
  const GlobalTopkShape g = global_topk_shape(layers, rows, nonzeros, value_bytes);
  if (g.status != 0) return g.status;
  if (!g.served || count < 0 || count > g.entries) return SPUTNIK_HIP_INVALID_ARGUMENT;
  if (layers == 0) return 0;
  if (row_offsets == nullptr || values == nullptr || out_row_offsets == nullptr || out_nonzeros == nullptr ||
      !aligned_to(out_nonzeros, sizeof(int)) || workspace == nullptr || !aligned_to(workspace, sizeof(unsigned)) ||
      workspace_bytes < sizeof(unsigned) * global_topk_workspace_words(g.rows))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  for (int l = 0; l < layers; ++l)
    if (out_row_offsets[l] == nullptr || !aligned_to(out_row_offsets[l], sizeof(int)) ||
        (rows[l] > 0 && (row_offsets[l] == nullptr || !aligned_to(row_offsets[l], sizeof(int)))) ||
        (nonzeros[l] > 0 && (values[l] == nullptr || !aligned_to(values[l], value_bytes))))
      return SPUTNIK_HIP_INVALID_ARGUMENT;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  return by_width(value_bytes, [&](auto u) {
    return launch_global_select<decltype(u)>(g, layers, rows, nonzeros, row_offsets, values,
                                             static_cast<unsigned>(count), workspace, out_row_offsets, out_nonzeros,
                                             stream);
  });
}

int sputnik_hip_csr_topk_global_fill(int layers, const int* rows, const int* nonzeros,
                                     const int* const* row_offsets, const int* const* column_indices,
                                     const void* const* values, int value_bytes, void* workspace,
                                     size_t workspace_bytes, const int64_t* out_capacity,
                                     int* const* out_row_indices, int* const* out_row_offsets,
                                     int* const* out_column_indices, void* const* out_values,
                                     int64_t* const* out_source, sputnik_hip_stream_t stream_) {
  const GlobalTopkShape g = global_topk_shape(layers, rows, nonzeros, value_bytes);
  if (g.status != 0) return g.status;
  if (!g.served) return SPUTNIK_HIP_INVALID_ARGUMENT;
  if (layers == 0) return 0;
  if (row_offsets == nullptr || column_indices == nullptr || values == nullptr || out_capacity == nullptr ||
      out_row_indices == nullptr || out_row_offsets == nullptr || out_column_indices == nullptr ||
      out_values == nullptr || out_source == nullptr || workspace == nullptr ||
      !aligned_to(workspace, sizeof(unsigned)) ||
      workspace_bytes < sizeof(unsigned) * global_topk_workspace_words(g.rows))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  for (int l = 0; l < layers; ++l) {
    if (out_capacity[l] < 0 || out_capacity[l] > nonzeros[l] || out_row_offsets[l] == nullptr ||
        !aligned_to(out_row_offsets[l], sizeof(int)) ||
        (rows[l] > 0 && (out_row_indices[l] == nullptr || !aligned_to(out_row_indices[l], sizeof(int)))))
      return SPUTNIK_HIP_INVALID_ARGUMENT;
    if (rows[l] > 0 && out_capacity[l] > 0 &&
        (row_offsets[l] == nullptr || !aligned_to(row_offsets[l], sizeof(int)) || column_indices[l] == nullptr ||
         !aligned_to(column_indices[l], sizeof(int)) || values[l] == nullptr ||
         !aligned_to(values[l], value_bytes) || out_column_indices[l] == nullptr ||
         !aligned_to(out_column_indices[l], sizeof(int)) || out_values[l] == nullptr ||
         !aligned_to(out_values[l], value_bytes) || out_source[l] == nullptr ||
         !aligned_to(out_source[l], sizeof(int64_t))))
      return SPUTNIK_HIP_INVALID_ARGUMENT;
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int st = by_width(value_bytes, [&](auto u) {
    return launch_global_fill<decltype(u)>(layers, rows, nonzeros, row_offsets, column_indices, values, workspace,
                                           out_capacity, out_row_offsets, out_column_indices, out_values, out_source,
                                           stream);
  });
  if (st != 0) return st;
  for (int l = 0; l < layers; ++l)
    if (rows[l] > 0) {
      const int order = sputnik_hip_csr_row_order(1, rows[l], 0, out_row_offsets[l], out_row_indices[l], stream_);
      if (order != 0) return order;
    }
  return launch_status();
}

int sputnik_hip_random_csr_launch_shape(int m, int n, int total_mode, int* served, int* rows_per_wave,
                                        int* elements_per_lane, int* rows_per_workgroup, int* digit_passes,
                                        int* grid, int* launches) {
  const RandomShape r = random_shape(m, n, total_mode);
  if (r.status != 0) return r.status;
  put(served, r.served);
  put(rows_per_wave, r.walk.rows_per_wave);
  put(elements_per_lane, r.walk.elements_per_lane);
  put(rows_per_workgroup, r.walk.rows_per_workgroup);
  put(digit_passes, kKeyDigitPasses);
  put(grid, r.walk.grid);
  put(launches, r.launches);
  return 0;
}

size_t sputnik_hip_random_csr_workspace_bytes(int m, int n, int total_mode) {
  if (m < 0 || n < 0 || !total_mode) return 0;   // per row: registers and LDS only
  return sizeof(unsigned) * topk_workspace_words(m, 1);
}

int sputnik_hip_random_csr(int m, int n, int total_mode, int64_t count, int dtype, float scale, unsigned key_mask,
                           sputnik_hip_philox_state rng, int64_t* rng_state_out, void* workspace,
                           size_t workspace_bytes, int* row_indices, int* row_offsets, int* column_indices,
                           void* values, sputnik_hip_stream_t stream_) {
  const RandomShape r = random_shape(m, n, total_mode);
  if (r.status != 0) return r.status;
  if (!r.served || key_mask > 0x7fffffffu ||
      (dtype != SPUTNIK_HIP_F32 && dtype != SPUTNIK_HIP_F16 && dtype != SPUTNIK_HIP_BF16))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  const int64_t most = total_mode ? static_cast<int64_t>(m) * n : n;
  if (count < 0 || count > most || row_offsets == nullptr || !aligned_to(row_offsets, sizeof(int)) ||
      (rng_state_out != nullptr && !aligned_to(rng_state_out, sizeof(int64_t))) ||
      (m > 0 && (row_indices == nullptr || !aligned_to(row_indices, sizeof(int)))))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  RandomArgs args;
  args.state.rng = rng;
  args.state.rng_state_out = rng_state_out;
  args.state.threshold = 0u;
  args.state.scale = 0.f;
  args.state.replica0 = 0;
  args.key_mask = key_mask;
  args.scale = scale;
  if (m == 0 || count == 0) {
    // nothing is kept: the zero offsets, the row order 0 .. m - 1 of equal lengths, and the state
    if (hipMemsetAsync(row_offsets, 0, sizeof(int) * (static_cast<size_t>(m) + 1), stream) != hipSuccess)
      return launch_status();
    if (m > 0) {
      const int order = sputnik_hip_csr_row_order(1, m, n, row_offsets, row_indices, stream_);
      if (order != 0) return order;
    }
    return publish_rng_state(args.state, stream);
  }
  const int value_bytes = dtype == SPUTNIK_HIP_F32 ? 4 : 2;
  const size_t ws_bytes = sputnik_hip_random_csr_workspace_bytes(m, n, total_mode);
  if (column_indices == nullptr || !aligned_to(column_indices, sizeof(int)) || values == nullptr ||
      !aligned_to(values, value_bytes) ||
      (ws_bytes > 0 && (workspace == nullptr || !aligned_to(workspace, sizeof(unsigned)) || workspace_bytes < ws_bytes)))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  int st;
  if (dtype == SPUTNIK_HIP_F32)
    st = launch_random<float>(r, m, n, total_mode, static_cast<unsigned>(count), args, workspace, row_indices,
                              row_offsets, column_indices, values, stream);
  else if (dtype == SPUTNIK_HIP_F16)
    st = launch_random<_Float16>(r, m, n, total_mode, static_cast<unsigned>(count), args, workspace, row_indices,
                                 row_offsets, column_indices, values, stream);
  else
    st = launch_random<__bf16>(r, m, n, total_mode, static_cast<unsigned>(count), args, workspace, row_indices,
                               row_offsets, column_indices, values, stream);
  if (st != 0 || !total_mode) return st;
  return sputnik_hip_csr_row_order(1, m, n, row_offsets, row_indices, stream_);
}

int sputnik_hip_csr_regrow_random_launch_shape(int m, int n, int nonzeros, int value_bytes, int total_mode,
                                               int* served, int* rows_per_wave, int* elements_per_lane,
                                               int* rows_per_workgroup, int* value_digit_passes,
                                               int* score_digit_passes, int* lds_bytes, int* max_m, int* max_n,
                                               int* grid, int* launches) {
  if ((total_mode != 0 && total_mode != 1) || nonzeros < 0) return SPUTNIK_HIP_INVALID_ARGUMENT;
  constexpr int key_bytes = static_cast<int>(sizeof(uint32_t));
  if (total_mode) {
    const RegrowTotalShape r = regrow_total_shape(m, n, nonzeros, key_bytes, value_bytes);
    if (r.status != 0) return r.status;
    put(served, r.served);
    put(rows_per_wave, r.rows_per_wave);
    put(elements_per_lane, r.elements_per_lane);
    put(rows_per_workgroup, r.rows_per_workgroup);
    put(value_digit_passes, r.value_passes);
    put(score_digit_passes, r.score_passes);
    put(lds_bytes, r.lds_bytes);
    put(max_m, r.max_m);
    put(max_n, r.max_n);
    put(grid, r.grid);
    // (without entries: the row order if there are rows, and the lane that publishes the state)
    put(launches, r.served ? (m > 0 && nonzeros > 0 ? r.launches : r.launches + 1) : -1);
    return 0;
  }
  const RegrowShape r = regrow_shape(m, n, key_bytes, value_bytes);
  if (r.status != 0) return r.status;
  put(served, r.served);
  put(rows_per_wave, r.rows_per_wave);
  put(elements_per_lane, r.elements_per_lane);
  put(rows_per_workgroup, r.rows_per_workgroup);
  put(value_digit_passes, r.value_passes);
  put(score_digit_passes, r.score_passes);
  put(lds_bytes, r.lds_bytes);
  put(max_m, -1);
  put(max_n, r.max_n);
  put(grid, r.grid);
  put(launches, r.served ? 1 : -1);   // (without entries: the lane that publishes the state)
  return 0;
}

size_t sputnik_hip_csr_regrow_random_workspace_bytes(int m, int n, int nonzeros, int total_mode) {
  return total_mode ? sputnik_hip_csr_regrow_total_workspace_bytes(m, n, nonzeros) : 0;
}

int sputnik_hip_csr_regrow_random(int m, int n, int nonzeros, const int* row_offsets, const int* column_indices,
                                  const void* values, int dtype, const int* drop_counts,
                                  sputnik_hip_philox_state rng, int64_t* rng_state_out, unsigned key_mask,
                                  int grow_values, float grow_scale, void* workspace, size_t workspace_bytes,
                                  int* out_column_indices, void* out_values, int64_t* out_source,
                                  sputnik_hip_stream_t stream_) {
  if (!key_scores_ok(dtype, key_mask, grow_values, grow_scale, rng_state_out)) return SPUTNIK_HIP_INVALID_ARGUMENT;
  const int value_bytes = dtype == SPUTNIK_HIP_F32 ? 4 : 2;
  const RegrowShape r = regrow_shape(m, n, static_cast<int>(sizeof(uint32_t)), value_bytes);
  if (r.status != 0) return r.status;
  if (!r.served || nonzeros < 0) return SPUTNIK_HIP_INVALID_ARGUMENT;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const KeyScores keys = key_scores(rng, rng_state_out, key_mask, grow_values, grow_scale);
  if (m == 0 || nonzeros == 0) return publish_rng_state(keys.args.state, stream);   // no entry, but a state
  if (row_offsets == nullptr || column_indices == nullptr || drop_counts == nullptr || values == nullptr ||
      !aligned_to(values, value_bytes) || out_column_indices == nullptr || out_values == nullptr ||
      !aligned_to(out_values, value_bytes) || out_source == nullptr || !aligned_to(out_source, sizeof(int64_t)) ||
      !aligned_to(row_offsets, sizeof(int)) || !aligned_to(column_indices, sizeof(int)) ||
      !aligned_to(drop_counts, sizeof(int)) || !aligned_to(out_column_indices, sizeof(int)))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    KeyScoresOf<T> typed;
    static_cast<KeyScores&>(typed) = keys;
    return by_width(value_bytes, [&](auto w) {
      if constexpr (sizeof(w) == sizeof(T))
        return launch_regrow<KeyScoresOf<T>, decltype(w)>(r, m, n, nonzeros, row_offsets, column_indices, values,
                                                          drop_counts, typed, kNoThreshold, out_column_indices,
                                                          out_values, out_source, stream);
      else
        return static_cast<int>(SPUTNIK_HIP_INVALID_ARGUMENT);
    });
  });
}

int sputnik_hip_csr_regrow_total_random(int m, int n, int nonzeros, const int* row_offsets,
                                        const int* column_indices, const void* values, int dtype, int64_t drop,
                                        sputnik_hip_philox_state rng, int64_t* rng_state_out, unsigned key_mask,
                                        int grow_values, float grow_scale, void* workspace, size_t workspace_bytes,
                                        int* out_row_indices, int* out_row_offsets, int* out_column_indices,
                                        void* out_values, int64_t* out_source, sputnik_hip_stream_t stream_) {
  if (!key_scores_ok(dtype, key_mask, grow_values, grow_scale, rng_state_out)) return SPUTNIK_HIP_INVALID_ARGUMENT;
  const int value_bytes = dtype == SPUTNIK_HIP_F32 ? 4 : 2;
  const RegrowTotalShape r = regrow_total_shape(m, n, nonzeros, static_cast<int>(sizeof(uint32_t)), value_bytes);
  if (r.status != 0) return r.status;
  if (!r.served || drop < 0 || drop > nonzeros || out_row_offsets == nullptr ||
      !aligned_to(out_row_offsets, sizeof(int)) ||
      (m > 0 && (out_row_indices == nullptr || !aligned_to(out_row_indices, sizeof(int)))))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const KeyScores keys = key_scores(rng, rng_state_out, key_mask, grow_values, grow_scale);
  if (m == 0 || nonzeros == 0) {
    // no entries: the zero offsets, the row order 0 .. m - 1 of equal lengths, and the state
    if (hipMemsetAsync(out_row_offsets, 0, sizeof(int) * (static_cast<size_t>(m) + 1), stream) != hipSuccess)
      return launch_status();
    if (m > 0) {
      const int order = sputnik_hip_csr_row_order(1, m, n, out_row_offsets, out_row_indices, stream_);
      if (order != 0) return order;
    }
    return publish_rng_state(keys.args.state, stream);
  }
  if (row_offsets == nullptr || !aligned_to(row_offsets, sizeof(int)) || column_indices == nullptr ||
      !aligned_to(column_indices, sizeof(int)) || values == nullptr || !aligned_to(values, value_bytes) ||
      out_column_indices == nullptr || !aligned_to(out_column_indices, sizeof(int)) || out_values == nullptr ||
      !aligned_to(out_values, value_bytes) || out_source == nullptr || !aligned_to(out_source, sizeof(int64_t)) ||
      workspace == nullptr || !aligned_to(workspace, sizeof(unsigned)) ||
      workspace_bytes < sputnik_hip_csr_regrow_total_workspace_bytes(m, n, nonzeros))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  const int st = by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    KeyScoresOf<T> typed;
    static_cast<KeyScores&>(typed) = keys;
    return by_width(value_bytes, [&](auto w) {
      if constexpr (sizeof(w) == sizeof(T))
        return launch_regrow_total<KeyScores, KeyScoresOf<T>, decltype(w)>(
            r, m, n, nonzeros, row_offsets, column_indices, values, static_cast<unsigned>(drop), keys, typed,
            kNoThreshold, workspace, out_row_offsets, out_column_indices, out_values, out_source, stream);
      else
        return static_cast<int>(SPUTNIK_HIP_INVALID_ARGUMENT);
    });
  });
  if (st != 0) return st;
  return sputnik_hip_csr_row_order(1, m, n, out_row_offsets, out_row_indices, stream_);
}

}  // extern "C"
