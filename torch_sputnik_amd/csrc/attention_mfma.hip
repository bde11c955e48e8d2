// Fused sparse attention forward on the matrix cores, for float16 / bfloat16 head views and
// head dimension 64 or 128:
//
//   out[i, :] = sum_j softmax_j(scale * <q_i, k_j>) * v_j      j over the stored columns of row i
//
// as a MASKED FLASH ATTENTION over 64-column key tiles.  The vector kernel (attention.hip)
// spends a v_dot2 chain and an element-wise widening of V on every mask entry; at attention
// densities every 128 x 64 tile of the mask holds entries, so the products of a tile are dense
// contractions for v_mfma_f32_32x32x16_{f16,bf16}, and the structured patterns
// (topology.AttentionPattern) are made of full tiles with empty ones between them, which are
// never visited.
//
// The plan (topology only, three launches, no host synchronisation):
//   bitmap [rows padded to 128][ceil(n / 64)] 64-bit words: bit c & 63 of word c >> 6 of row r
//          is set iff (r, c) is an entry (cleared, then one OR per entry: any column order);
//   lists  [row blocks][1 + ceil(n / 64)] ints: the number of occupied key tiles of a block of
//          128 rows, then the tiles, ascending.
//
// The kernel: one workgroup of four waves per (replica, 128-row block), a wave owns 32 query
// rows.  Q is read once into registers as MFMA operand fragments.  Per occupied tile, K and V
// (64 rows of 2 d bytes each) are staged in LDS by direct global->LDS copies, double buffered:
//   1. S^T = K Q^T (A = K tile rows from LDS, B = the Q fragments): in the 32 x 32 accumulator
//      layout a lane then holds ONE query row (lane & 31) and 2 x 16 key columns, so the row's
//      64-bit mask word masks all of them by selects, and the row maximum is 31 in-lane
//      operations and one exchange between the two lane halves;
//   2. online softmax in float32 on scale * log2(e) * s with exp2; the row sum is kept as a
//      partial sum per lane half (of the UNROUNDED weights) and joined once, in the epilogue;
//   3. O^T += V^T P^T: the weights, rounded once to T, stay in registers as the B operand.  A
//      lane's accumulator registers 8s .. 8s + 7 of a 32-key block are keys 16s + 8t + 4h + i
//      (h = lane >> 5; t, i from the register), and V's A operand is read from LDS in exactly
//      that order by the transposing 4 x 16 read (ds_read_b64_tr_b16), whose four rows are the
//      keys 16s + 8t + 4h .. + 3.  The accumulator again holds one query row per lane, so the
//      rescale by exp2(old max - new max) is one factor per lane.
// LDS images are swizzled in the copies' per-lane SOURCE address (mfma_gemm.h).  At d = 64 (two
// rows span the 64 banks) K's 16-byte slot g of row r lands in slot g ^ ((r >> 1) & 7) for the
// ds_read_b128 fragments, V's 64-byte half c of row r in half c ^ ((r >> 1) & 1), which spreads
// the four rows of a transposing read over all 64 banks.  At d = 128 a row IS the 64 banks and
// every row starts on bank 0: K's slot g (of 16) lands in slot g ^ (r & 15), so that 16 lanes on
// consecutive rows and one fragment slot read 16 different slots, V's 64-byte quarter c in
// quarter c ^ (r & 3), so that the four rows 4 j .. 4 j + 3 of a transposing read, which all ask
// for one quarter, find it in four different ones (K_SWIZZLE / V_SWIZZLE below).
#include <algorithm>
#include <type_traits>

#include "mfma_tiles.h"

namespace sputnik_hip {
namespace {

using namespace mfma_tiles;
using tiled::xcd_local_index;

constexpr int kBM = 128;        // query rows per workgroup
constexpr int kBN = 64;         // key rows per tile: one mask word per query row
constexpr int kThreads = 256;   // four waves of 32 query rows

// What depends on the head dimension D: the K / V tile images in LDS and their swizzles.
template <int D>
struct Geometry {
  static_assert(D == 64 || D == 128, "head dimension 64 or 128");
  static constexpr int kRowBytes = D * 2;                // 128 / 256
  static constexpr int kTileBytes = kBN * kRowBytes;     // 8 / 16 KiB: one of K / V
  static constexpr int kSlotBits = D == 64 ? 3 : 4;
  static constexpr int kSlots = 1 << kSlotBits;          // 16-byte slots of a row: 8 / 16
  static constexpr int kPieceRows = 1024 / kRowBytes;    // rows of a 1 KiB lane-linear copy: 8 / 4
  static constexpr int kWavePieces = kBN / kPieceRows / 4;   // copies per operand, tile and wave: 2 / 4
  static constexpr int kSteps = D / 16;                  // k-steps of the scores
  static constexpr int kBlocks = D / 32;                 // 32 x 32 accumulators of O^T
};
// Source slot g of row `row` lands in slot g ^ swizzle: K's in g ^ K_SWIZZLE(D, row), V's 64-byte
// part c in part c ^ V_SWIZZLE(D, row).  (Macros: the d = 64 instances are to stay, instruction
// for instruction, what they were before the kernel had a D.)
#define K_SWIZZLE(D, row) ((D) == 64 ? ((row) >> 1) & 7 : (row) & 15)
#define V_SWIZZLE(D, row) ((D) == 64 ? ((row) >> 1) & 1 : (row) & 3)
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

using u64 = unsigned long long;
typedef short s4v __attribute__((__vector_size__(8)));
typedef short s8v __attribute__((__vector_size__(16)));
using f4v = float __attribute__((ext_vector_type(4)));
using f8v = float __attribute__((ext_vector_type(8)));

struct View {   // a strided head view (sputnik_hip.h), strides in elements
  const void* base;
  int64_t batch, head, row;
};

// ---- the plan ----
inline int tiles_of(int n) { return ceil_div(n, kBN); }
inline int blocks_of(int m) { return ceil_div(m, kBM); }
inline int64_t list_bytes(int m, int n) {   // a multiple of 16: the bitmap sits behind the lists
  return (static_cast<int64_t>(blocks_of(m)) * (1 + tiles_of(n)) * 4 + 15) / 16 * 16;
}
inline int64_t bitmap_words(int m, int n) { return static_cast<int64_t>(blocks_of(m)) * kBM * tiles_of(n); }
inline int64_t plan_bytes_of(int m, int n) {
  if (m <= 0 || n <= 0) return 0;
  return list_bytes(m, n) + bitmap_words(m, n) * 8;
}

// (words is even: the rows are padded to 128)
__global__ __launch_bounds__(256) void attention_tiles_clear_kernel(uint4* __restrict__ bitmap, int64_t pairs) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < pairs;
       i += static_cast<int64_t>(gridDim.x) * 256)
    bitmap[i] = make_uint4(0u, 0u, 0u, 0u);
}

// One wave per row: a bit per entry.  OR commutes, so the bitmap does not depend on the order
// of the atomics, nor on the order of the columns inside the row.
__global__ __launch_bounds__(256) void attention_tiles_bits_kernel(
    int m, int n, int nt, const int* __restrict__ row_offsets, const int* __restrict__ column_indices,
    u64* __restrict__ bitmap) {
  const int lane = threadIdx.x & 63;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= m) return;
  const int p1 = row_offsets[row + 1];
  for (int p = row_offsets[row] + lane; p < p1; p += 64) {
    const int c = column_indices[p];
    if (static_cast<unsigned>(c) < static_cast<unsigned>(n))
      atomicOr(bitmap + row * nt + (c >> 6), u64{1} << (c & 63));
  }
}

// One workgroup per block of 128 rows: ORs its rows' words tile by tile (thread = tile) and
// compacts the occupied tiles, ascending, behind their count.
__global__ __launch_bounds__(256) void attention_tiles_list_kernel(int nt, const u64* __restrict__ bitmap,
                                                                   int* __restrict__ lists) {
  __shared__ int wave_count[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64* __restrict__ rows = bitmap + static_cast<int64_t>(blockIdx.x) * kBM * nt;
  int* __restrict__ list = lists + static_cast<int64_t>(blockIdx.x) * (1 + nt);
  int total = 0;
  for (int base = 0; base < nt; base += 256) {
    const int t = base + threadIdx.x;
    u64 any = 0;
    if (t < nt)
      for (int r = 0; r < kBM; ++r) any |= rows[static_cast<int64_t>(r) * nt + t];
    const u64 occupied = __builtin_amdgcn_ballot_w64(any != 0);
    if (lane == 0) wave_count[wave] = __popcll(occupied);
    __syncthreads();
    int at = total + __popcll(occupied & ((u64{1} << lane) - 1));
    for (int w = 0; w < 4; ++w) {
      at += w < wave ? wave_count[w] : 0;
      total += wave_count[w];
    }
    if (any != 0) list[1 + at] = t;
    __syncthreads();
  }
  if (threadIdx.x == 0) list[0] = total;
}

// ---- the attention kernel ----

// Stages key rows key0 .. key0 + 63 of K and V into `stage` ([K tile | V tile]) with 1 KiB
// copies of 8 rows, two of each per wave (d = 128: of 4 rows, four of each).  Rows at n and
// beyond are ZERO-FILLED by the lanes that would have copied them (those lanes issue no
// copy): 0 x garbage never reaches an accumulator.
template <int D, typename T>
__device__ __forceinline__ void stage_tile(char* stage, const T* k, unsigned k_row_bytes, const T* v,
                                           unsigned v_row_bytes, int n, int key0, int wave, int lane) {
  using G = Geometry<D>;
#pragma unroll
  for (int j = 0; j < G::kWavePieces; ++j) {
    const int piece = wave + 4 * j;
    const int row = G::kPieceRows * piece + (lane >> G::kSlotBits), slot = lane & (G::kSlots - 1);
    char* k_dst = stage + piece * 1024;
    char* v_dst = stage + G::kTileBytes + piece * 1024;
    const unsigned key = static_cast<unsigned>(key0 + row);
    if (key0 + row < n) {
      copy_piece(k, key * k_row_bytes + static_cast<unsigned>(slot ^ K_SWIZZLE(D, row)) * 16u, k_dst);
      copy_piece(v, key * v_row_bytes + static_cast<unsigned>(slot ^ (V_SWIZZLE(D, row) * 4)) * 16u, v_dst);
    } else {
      *reinterpret_cast<uint4*>(k_dst + lane * 16) = make_uint4(0u, 0u, 0u, 0u);
      *reinterpret_cast<uint4*>(v_dst + lane * 16) = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

// D: head dimension; T: storage type of q, k, v; TO: of the context (float, or T).  Replicas
// replica0 .. replica0 + gridDim.y - 1 of the call (a grid slice); the row blocks of a replica
// read the same K and V and the heads of a batch element neighbouring columns of the same
// rows: the work index is decoded XCD-locally (xcd_local_index).
template <int D, typename T, typename TO>
__global__ __launch_bounds__(kThreads) void sparse_attention_tiles_kernel(
    int m, int n, int nt, int heads, int replica0, const int* __restrict__ lists,
    const u64* __restrict__ bitmap, View qv, View kv, View vv, float scale_log2e, View ov,
    float* __restrict__ lse, int64_t lse_stride) {
  using G = Geometry<D>;
  enum { kRowBytes = G::kRowBytes, kTileBytes = G::kTileBytes };
  using H8 = typename Half8<T>::type;
  using T4 = T __attribute__((ext_vector_type(4)));
  using T8 = T __attribute__((ext_vector_type(8)));
  using O4 = typename std::conditional<std::is_same<TO, float>::value, f4v, T4>::type;
  __shared__ __attribute__((aligned(16))) char stage[2][2 * kTileBytes];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qr = lane & 31, h = lane >> 5;
  const u64 work = xcd_local_index();
  const int mblock = static_cast<int>(work % gridDim.x);
  const int replica = replica0 + static_cast<int>(work / gridDim.x);
  const int64_t b = replica / heads, hd = replica - b * heads;
  const T* __restrict__ q = static_cast<const T*>(qv.base) + (b * qv.batch + hd * qv.head);
  const T* __restrict__ k = uniform_ptr(static_cast<const T*>(kv.base) + (b * kv.batch + hd * kv.head));
  const T* __restrict__ v = uniform_ptr(static_cast<const T*>(vv.base) + (b * vv.batch + hd * vv.head));
  TO* __restrict__ out = static_cast<TO*>(const_cast<void*>(ov.base)) + (b * ov.batch + hd * ov.head);
  const unsigned k_bytes = static_cast<unsigned>(kv.row) * 2u, v_bytes = static_cast<unsigned>(vv.row) * 2u;

  const int row = mblock * kBM + wave * 32 + qr;       // this lane's query row
  const int* __restrict__ list = lists + static_cast<int64_t>(mblock) * (1 + nt);
  const int count = list[0];
  // (rows at m and beyond are bitmap padding: all zero)
  const u64* __restrict__ words = bitmap + static_cast<int64_t>(row) * nt;

  // Q as B operand fragments: column = query row, k = head elements 16 ks + 8 h .. + 7
  H8 qf[G::kSteps];
  {
    const T* q_row = q + static_cast<unsigned>(min(row, m - 1)) * static_cast<unsigned>(qv.row);
#pragma unroll
    for (int ks = 0; ks < G::kSteps; ++ks) qf[ks] = *reinterpret_cast<const H8*>(q_row + 16 * ks + 8 * h);
  }

  f32x16 o[G::kBlocks] = {};   // O^T: head elements db * 32 + 8 (r / 4) + 4 h + r % 4 of this lane's row
  float mx = -INFINITY;    // running maximum, in units of log2
  float l = 0.f;           // this lane half's part of the row sum

  // fragment addresses inside a stage: K row qr (+ 32 kb), slot 2 ks + h; V rows 4 h + q4 (+ the
  // step's first key), columns 32 db + 16 g1 + 4 p .. + 3
  const unsigned k_at = static_cast<unsigned>(qr * kRowBytes + ((h ^ K_SWIZZLE(D, qr)) * 16));
  const int q4 = (lane & 15) >> 2;
  const unsigned v_at = static_cast<unsigned>(kTileBytes + (4 * h + q4) * kRowBytes + (V_SWIZZLE(D, q4) * 64) +
                                              32 * ((lane >> 4) & 1) + 8 * (lane & 3));

  u64 word = 0;
  if (count > 0) {
    const int t0 = list[1];
    stage_tile<D>(stage[0], k, k_bytes, v, v_bytes, n, t0 * kBN, wave, lane);
    word = words[t0];
    tiled::wait_vm<0>();
    __syncthreads();
  }

  for (int i = 0; i < count; ++i) {
    const char* st = stage[i & 1];
    u64 next_word = 0;
    if (i + 1 < count) {
      const int t1 = list[i + 2];
      stage_tile<D>(stage[(i & 1) ^ 1], k, k_bytes, v, v_bytes, n, t1 * kBN, wave, lane);
      next_word = words[t1];
    }

    // 1. scores, transposed: s[kb] register r = key kb * 32 + 8 (r / 4) + 4 h + r % 4
    f32x16 s[2] = {};
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ks = 0; ks < G::kSteps; ++ks) {
        const H8 a = *reinterpret_cast<const H8*>(st + kb * 32 * kRowBytes + (k_at ^ (ks * 32u)));
        s[kb] = Half8<T>::mfma(a, qf[ks], s[kb]);
      }

    // the row's mask word: absent entries become -inf by select
    float tile_max = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const unsigned bits = static_cast<unsigned>(word >> (32 * kb)) >> (4 * h);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool kept = (bits >> (8 * (r / 4) + r % 4)) & 1u;
        s[kb][r] = kept ? s[kb][r] * scale_log2e : -INFINITY;
        tile_max = fmaxf(tile_max, s[kb][r]);
      }
    }
    tile_max = fmaxf(tile_max, __shfl_xor(tile_max, 32));

    // 2. online softmax.  A row without an entry so far keeps mx = -inf; it subtracts 0, so
    // its weights are exp2(-inf) = 0 and not exp2(-inf + inf).
    const float m_new = fmaxf(mx, tile_max);
    const float m_sub = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(mx - m_sub);
    mx = m_new;
    float sum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[kb][r] = __builtin_amdgcn_exp2f(s[kb][r] - m_sub);
        sum += s[kb][r];
      }
    l = l * alpha + sum;
    o[0] *= alpha;   // (written out, not a loop: see K_SWIZZLE)
    o[1] *= alpha;
    if constexpr (D == 128) {
      o[2] *= alpha;
      o[3] *= alpha;
    }

    // 3. O^T += V^T P^T, the weights rounded once to T
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        f8v p8;
#pragma unroll
        for (int j = 0; j < 8; ++j) p8[j] = s[kb][8 * ss + j];
        const H8 pf = __builtin_bit_cast(H8, __builtin_convertvector(p8, T8));
#pragma unroll
        for (int db = 0; db < G::kBlocks; ++db) {
          const char* at = st + (kb * 32 + ss * 16) * kRowBytes + (v_at ^ (db * 64u));
          const s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(at));
          const s4v hi =
              __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(at + 8 * kRowBytes));
          const s8v both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          o[db] = Half8<T>::mfma(__builtin_bit_cast(H8, both), pf, o[db]);
        }
      }

    word = next_word;
    tiled::wait_vm<0>();   // the next tiles have landed
    __syncthreads();       // ... for every wave, and this stage is free
  }

  // epilogue: rows without entries (l = 0) store zeros and lse = -inf
  l += __shfl_xor(l, 32);
  if (row >= m) return;
  const float inv = l > 0.f ? 1.f / l : 0.f;
  TO* out_row = out + static_cast<unsigned>(row) * static_cast<unsigned>(ov.row);
#pragma unroll
  for (int db = 0; db < G::kBlocks; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f4v r4 = {o[db][4 * g] * inv, o[db][4 * g + 1] * inv, o[db][4 * g + 2] * inv,
                      o[db][4 * g + 3] * inv};
      *reinterpret_cast<O4*>(out_row + db * 32 + 8 * g + 4 * h) = __builtin_convertvector(r4, O4);
    }
  if (lse != nullptr && h == 0)
    lse[replica * lse_stride + row] = l > 0.f ? mx * kLn2 + __logf(l) : -INFINITY;
}

// What the kernel assumes about a head view of `rows` rows of d elements: a 16-byte aligned
// base and strides, non-negative strides, and a replica's extent below 2^32 bytes (its
// in-replica offsets are 32-bit).  The vector kernel's check (attention.hip) is this one at
// its own head dimension, 64.
bool view_ok(const View& w, int rows, int d, int elem_bytes) {
  if (w.base == nullptr || !aligned_to(w.base, 16)) return false;
  if (w.batch < 0 || w.head < 0 || w.row < 0) return false;
  if ((w.batch * elem_bytes) % 16 != 0 || (w.head * elem_bytes) % 16 != 0 || (w.row * elem_bytes) % 16 != 0)
    return false;
  return (static_cast<int64_t>(rows - 1) * w.row + d) * elem_bytes < (int64_t{1} << 32);
}

template <int D, typename T, typename TO>
void launch_tiles(int m, int n, int heads, int r0, int count, const void* plan, const View& q, const View& k,
                  const View& v, float scale, const View& o, float* lse, int64_t lse_stride,
                  hipStream_t stream) {
  const int* lists = static_cast<const int*>(plan);
  const u64* bitmap = reinterpret_cast<const u64*>(static_cast<const char*>(plan) + list_bytes(m, n));
  hipLaunchKernelGGL((sparse_attention_tiles_kernel<D, T, TO>), dim3(blocks_of(m), count), dim3(kThreads), 0,
                     stream, m, n, tiles_of(n), heads, r0, lists, bitmap, q, k, v, scale * kLog2e, o, lse,
                     lse_stride);
}

}  // namespace
}  // namespace sputnik_hip

using namespace sputnik_hip;

extern "C" {

size_t sputnik_hip_sparse_attention_tiles_plan_bytes(int m, int n) {
  return static_cast<size_t>(plan_bytes_of(m, n));
}

int sputnik_hip_sparse_attention_tiles_plan(int m, int n, int nonzeros, const int* row_offsets,
                                            const int* column_indices, void* plan, size_t plan_bytes,
                                            sputnik_hip_stream_t stream) {
  if (m < 0 || n < 0 || nonzeros < 0) return SPUTNIK_HIP_INVALID_ARGUMENT;
  const int64_t need = plan_bytes_of(m, n);
  if (need == 0 || need >= (int64_t{1} << 31)) return SPUTNIK_HIP_UNSUPPORTED;
  if (plan == nullptr || !aligned_to(plan, 16) || plan_bytes < static_cast<size_t>(need) ||
      row_offsets == nullptr || (nonzeros > 0 && column_indices == nullptr))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  const int nt = tiles_of(n);
  u64* bitmap = reinterpret_cast<u64*>(static_cast<char*>(plan) + list_bytes(m, n));
  const int64_t pairs = bitmap_words(m, n) / 2;
  hipLaunchKernelGGL(attention_tiles_clear_kernel,
                     dim3(static_cast<unsigned>(std::min<int64_t>(ceil_div64(pairs, 256), 4096))), dim3(256),
                     0, stream, reinterpret_cast<uint4*>(bitmap), pairs);
  hipLaunchKernelGGL(attention_tiles_bits_kernel, dim3(ceil_div(m, 4)), dim3(256), 0, stream, m, n, nt,
                     row_offsets, column_indices, bitmap);
  hipLaunchKernelGGL(attention_tiles_list_kernel, dim3(blocks_of(m)), dim3(256), 0, stream, nt, bitmap,
                     static_cast<int*>(plan));
  return launch_status();
}

int sputnik_hip_sparse_attention_tiles_supported(
    int m, int n, int d, int nonzeros, int batch, int heads, int dtype, int out_type, const void* q,
    int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride, const void* k,
    int64_t k_batch_stride, int64_t k_head_stride, int64_t k_row_stride, const void* v,
    int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride, const void* out,
    int64_t out_batch_stride, int64_t out_head_stride, int64_t out_row_stride) {
  // the heads contract with this kernel's head dimensions (half storage, a mask with entries
  // and n below 2^24, aligned views with 32-bit extents), and a plan its 32-bit offsets reach
  if (d != 64 && d != 128) return 0;
  if (m <= 0 || n <= 0 || nonzeros <= 0 || n >= (1 << 24)) return 0;
  if (dtype != SPUTNIK_HIP_F16 && dtype != SPUTNIK_HIP_BF16) return 0;
  if (out_type != SPUTNIK_HIP_F32 && out_type != dtype) return 0;
  if (batch <= 0 || heads <= 0 || static_cast<int64_t>(batch) * heads >= (int64_t{1} << 31)) return 0;
  const int out_bytes = out_type == SPUTNIK_HIP_F32 ? 4 : 2;
  if (!view_ok(View{q, q_batch_stride, q_head_stride, q_row_stride}, m, d, 2) ||
      !view_ok(View{k, k_batch_stride, k_head_stride, k_row_stride}, n, d, 2) ||
      !view_ok(View{v, v_batch_stride, v_head_stride, v_row_stride}, n, d, 2) ||
      !view_ok(View{out, out_batch_stride, out_head_stride, out_row_stride}, m, d, out_bytes))
    return 0;
  return plan_bytes_of(m, n) < (int64_t{1} << 31) ? 1 : 0;
}

int sputnik_hip_sparse_attention_tiles_forward(
    int m, int n, int d, int nonzeros, int batch, int heads, const int* row_indices, const int* row_offsets,
    const int* column_indices, int dtype, const void* q, int64_t q_batch_stride, int64_t q_head_stride,
    int64_t q_row_stride, const void* k, int64_t k_batch_stride, int64_t k_head_stride, int64_t k_row_stride,
    const void* v, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride, float scale, void* out,
    int out_type, int64_t out_batch_stride, int64_t out_head_stride, int64_t out_row_stride, float* lse,
    int64_t lse_stride, const void* plan, size_t plan_bytes, sputnik_hip_stream_t stream) {
  if (m < 0 || n < 0 || d < 0 || nonzeros < 0 || batch < 0 || heads < 0) return SPUTNIK_HIP_INVALID_ARGUMENT;
  if (m == 0 || batch == 0 || heads == 0) return 0;
  if (!sputnik_hip_sparse_attention_tiles_supported(
          m, n, d, nonzeros, batch, heads, dtype, out_type, q, q_batch_stride, q_head_stride, q_row_stride, k,
          k_batch_stride, k_head_stride, k_row_stride, v, v_batch_stride, v_head_stride, v_row_stride, out,
          out_batch_stride, out_head_stride, out_row_stride))
    return SPUTNIK_HIP_UNSUPPORTED;
  if (plan == nullptr || !aligned_to(plan, 16) || plan_bytes < static_cast<size_t>(plan_bytes_of(m, n)))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  const View qv{q, q_batch_stride, q_head_stride, q_row_stride}, kv{k, k_batch_stride, k_head_stride, k_row_stride},
      vv{v, v_batch_stride, v_head_stride, v_row_stride}, ov{out, out_batch_stride, out_head_stride, out_row_stride};
  const int replicas = batch * heads;   // (below 2^31: the heads contract)
  for (int r0 = 0; r0 < replicas; r0 += kMaxGridYZ) {
    const int count = min(replicas - r0, kMaxGridYZ);
    auto go = [&](auto launch) { launch(m, n, heads, r0, count, plan, qv, kv, vv, scale, ov, lse, lse_stride, stream); };
    const bool f16 = dtype == SPUTNIK_HIP_F16, wide = out_type == SPUTNIK_HIP_F32;
    if (d == 64) {
      if (f16 && wide) go(launch_tiles<64, _Float16, float>);
      else if (f16) go(launch_tiles<64, _Float16, _Float16>);
      else if (wide) go(launch_tiles<64, __bf16, float>);
      else go(launch_tiles<64, __bf16, __bf16>);
    } else {
      if (f16 && wide) go(launch_tiles<128, _Float16, float>);
      else if (f16) go(launch_tiles<128, _Float16, _Float16>);
      else if (wide) go(launch_tiles<128, __bf16, float>);
      else go(launch_tiles<128, __bf16, __bf16>);
    }
    const int st = launch_status();
    if (st != 0) return st;
  }
  return 0;
}

}  // extern "C"
