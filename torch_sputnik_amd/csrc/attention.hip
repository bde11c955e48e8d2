// Fused sparse attention forward for gfx950:
//
//   out[i, :] = sum_j softmax_j(scale * <q_i, k_j>) * v_j      j over the stored
//                                                               columns of mask row i
//
// One kernel for the chain the reference runs as three library calls and an
// elementwise pass -- sddmm, "/ sqrt(d)", sparse_softmax, spmm
// (modules/sparse_attention.py:66-82) -- so the [replicas, nnz] score and
// weight arrays never exist: HBM traffic is Q, K, V and the output only.
//
// Decomposition (the 64-column SpMM kernel's, spmm_tiled64.hip): a workgroup
// owns 128 query rows and walks the key/value rows in chunks of 128; each
// chunk's K rows and V rows are staged into LDS by direct global->LDS copies
// (double buffered).  A 16-lane row group owns one query row: its q fragment,
// running maximum, running sum and 4 output columns per lane stay in registers
// for the whole walk (online softmax).  Per 16-entry window of a row's columns
// inside the chunk:
//   1. scores in the QUAD form of sddmm_tiled.hip -- the four quads of a row group work
//      on four different entries, lane (quad q, t) holds a quarter of the q row (16
//      elements, chunk order rotated by q: no LDS bank conflict) and two quad_perm adds
//      close a dot product; lane (q, t) ends up with the score of entry 4t + q, which is
//      where that entry's column lives (the kernel is 80 % busy issuing vector
//      instructions, profiles/r3e_pmc_sq_attention_ops.json; the 16-lane form before it
//      spent a third of them on broadcasts and a 45-instruction transposing reduction);
//   2. window maximum and sum with two 16-lane DPP all-reduces, one exp per
//      lane, rescale of the accumulators;
//   3. the weights go back out to all lanes entry by entry, paired with the
//      tile offset in one 64-bit DPP broadcast, against the V rows (same
//      offsets: the V tile sits at a fixed distance from the K tile; step 3 finds
//      entry u in lane 4 (u % 4) + u / 4).
// Needs ascending columns inside rows (checked by the shared pre-pass); row
// blocks that fail take an order-independent path (K, V gathered from L2).
//
// ONE kernel body, sparse_attention_kernel<T, TO, MANY, Drop...>, serves float32 [R, S, 64]
// operands (T = TO = float) and float16 / bfloat16 head views (TO = float or T).  What
// differs between the storage types is in Storage<T>: bytes per staged row, how q is kept,
// the inner product of step 1 and where the scale goes, and how rows are addressed.
//
// Attention dropout (philox.h): the instances with a DropArgs argument decide
// per entry, in step 2, whether the weight handed to step 3 is kept; l and lse still take
// every entry.
#include "philox.h"
#include "spmm_tiled_common.h"

namespace sputnik_hip {
namespace {

using namespace tiled;

constexpr int kD = 64;      // head dimension served by this kernel
constexpr int kWaves = 16;  // waves per workgroup
constexpr int kRQ = 2;      // row quads per wave (4 query rows each)
constexpr int kBK = 128;    // key/value rows per LDS stage
constexpr int kBM = kWaves * kRQ * 4;
constexpr int kThreads = kWaves * kWave;
constexpr int kTile = kBK * kD;  // elements of one of K / V per stage: 32 KiB float32, 16 KiB half
constexpr int kWin = 2;          // 16-entry windows prefetched per row and chunk

using f4v = float __attribute__((ext_vector_type(4)));
using v2f = float __attribute__((ext_vector_type(2)));

// An operand as a strided HEAD VIEW: element (b, h, row, c) at base + b * batch + h * head +
// row * row_stride + c, replica r = b * heads + h -- so half q, k, v and the context can stay
// [B, S, E] tensors (head h = columns h*64 .. h*64+63) with no head split or merge pass.
// A float32 [R, S, 64] operand with replica stride s is the view (0, s, 64) of one batch
// element with R heads (Storage<float>::batch_of).
struct HeadView {
  const void* base;
  int64_t batch, head, row;   // strides in elements
};

template <typename T>
struct Vec4;
template <>
struct Vec4<_Float16> {
  using type = _Float16 __attribute__((ext_vector_type(4)));
  using pair = _Float16 __attribute__((ext_vector_type(2)));
  // a.x b.x + a.y b.y + c: the products exact, the sum float32 (v_dot2_f32_f16)
  static __device__ __forceinline__ float dot2(pair a, pair b, float c) {
    return __builtin_amdgcn_fdot2(a, b, c, false);
  }
};
template <>
struct Vec4<__bf16> {
  using type = __bf16 __attribute__((ext_vector_type(4)));
  using pair = __bf16 __attribute__((ext_vector_type(2)));
  static __device__ __forceinline__ float dot2(pair a, pair b, float c) {
    return __builtin_amdgcn_fdot2_f32_bf16(a, b, c, false);
  }
};
template <>
struct Vec4<float> {
  using type = f4v;
};

// four consecutive elements (8-byte aligned for half storage), widened
template <typename T>
__device__ __forceinline__ f4v load4(const T* p) {
  return __builtin_convertvector(*reinterpret_cast<const typename Vec4<T>::type*>(p), f4v);
}

// What the kernel body leaves to the storage type T of q, k and v.  Half (this one): q is
// kept as STORED and step 1 multiplies half pairs with v_dot2_f32_* (exact products, float32
// sums -- no widening instruction per element, which left the issue-bound kernel a quarter
// longer), the scale is applied to the float32 score; rows are addressed through the view's
// row stride with 32-bit offsets inside a replica (heads_served guarantees they fit).
template <typename T>
struct Storage {
  using V4 = typename Vec4<T>::type;
  using P2 = typename Vec4<T>::pair;
  struct Q {
    P2 lo, hi;
  };
  static constexpr int kRowBytes = kD * static_cast<int>(sizeof(T));   // one tile row
  // replica r = b * heads + h of the view's (batch element, head)
  static __device__ __forceinline__ int batch_of(int replica, int heads) { return replica / heads; }
  static __device__ __forceinline__ unsigned row(int r, unsigned stride) {   // element offset
    return static_cast<unsigned>(r) * stride;
  }
  static __device__ __forceinline__ unsigned row_bytes(unsigned stride) { return stride * 2u; }
  static __device__ __forceinline__ Q keep_q(V4 q, float) { return Q{P2{q.x, q.y}, P2{q.z, q.w}}; }
  static __device__ __forceinline__ void mac(v2f& a, const Q& q, V4 b) {
    a.x = Vec4<T>::dot2(q.lo, P2{b.x, b.y}, a.x);
    a.y = Vec4<T>::dot2(q.hi, P2{b.z, b.w}, a.y);
  }
  static __device__ __forceinline__ float score(float s, float scale) { return s * scale; }
};
// float32: q is scaled once at load and step 1 is a chain of packed FMAs; rows are 64
// contiguous elements, and q / out row offsets are 64-bit (supported() bounds only n).  The
// R replicas of an [R, S, 64] operand are the heads of ONE batch element: no division.
template <>
struct Storage<float> {
  using V4 = f4v;
  using Q = f4v;
  static constexpr int kRowBytes = kD * 4;
  static __device__ __forceinline__ int batch_of(int, int) { return 0; }   // one batch element, R heads
  static __device__ __forceinline__ int64_t row(int r, unsigned) { return static_cast<int64_t>(r) * kD; }
  static __device__ __forceinline__ unsigned row_bytes(unsigned) { return kRowBytes; }
  static __device__ __forceinline__ Q keep_q(V4 q, float scale) { return q * scale; }
  static __device__ __forceinline__ void mac(v2f& a, const Q& q, V4 b) {
    a = __builtin_elementwise_fma(v2f{q.x, q.y}, v2f{b.x, b.y}, a);
    a = __builtin_elementwise_fma(v2f{q.z, q.w}, v2f{b.z, b.w}, a);
  }
  static __device__ __forceinline__ float score(float s, float) { return s; }
};

// Stages key/value rows jc .. jc + kBK - 1 into `tile` ([K rows | V rows]) with 1 KiB copies:
// 4 float32 or 8 half rows each, 16 bytes per lane.
template <typename T>
__device__ __forceinline__ void stage_kv(T* __restrict__ tile, const T* __restrict__ k,
                                         unsigned k_row_bytes, const T* __restrict__ v,
                                         unsigned v_row_bytes, int n, int jc, int wave, int lane) {
  constexpr int kRows = 1024 / Storage<T>::kRowBytes;   // rows per copy
  constexpr int kLanes = kWave / kRows;                 // lanes per row
  constexpr int kCopiesPerWave = (kBK / kRows) / kWaves;
  static_assert((kBK / kRows) % kWaves == 0, "stage copies split evenly over the waves");
  const int g = lane / kLanes, i = lane % kLanes;
#pragma unroll
  for (int j = 0; j < kCopiesPerWave; ++j) {
    const int r0 = (wave + j * kWaves) * kRows;
    const unsigned src_row = static_cast<unsigned>(min(jc + r0 + g, n - 1));  // past the last key: the last row
    lds_dma_row(reinterpret_cast<const float*>(k), src_row * k_row_bytes + i * 16u,
                reinterpret_cast<const float*>(tile + r0 * kD));
    lds_dma_row(reinterpret_cast<const float*>(v), src_row * v_row_bytes + i * 16u,
                reinterpret_cast<const float*>(tile + kTile + r0 * kD));
  }
}

template <typename T>
struct RowAcc {
  // elements 16t + 4((c + quad) % 4) .. +3 of the q row for c = 0..3 (lane = (quad, t))
  typename Storage<T>::Q q[4];
  float4 acc;  // unnormalised output columns 4i .. 4i+3
  float mx, l;
};

template <int S>
__device__ __forceinline__ int quad_bcast_add(int v, int add) {
  // add + (v of lane S of the quad): v_add_u32_dpp quad_perm:[S,S,S,S]
  return __builtin_amdgcn_update_dpp(0, v, S * 0x55, 0xF, 0xF, true) + add;
}

__device__ __forceinline__ float dot4(const f4v& a, const f4v& b) {
  float s = a.x * b.x;
  s = fmaf(a.y, b.y, s);
  s = fmaf(a.z, b.z, s);
  return fmaf(a.w, b.w, s);
}

// Online-softmax update of one row with `e`-weighted V contributions still to
// be added by the caller: returns the factor the old accumulators were scaled by.
template <typename R>
__device__ __forceinline__ void rescale(R& r, float m_new) {
  const float alpha = __expf(r.mx - m_new);  // mx = -inf gives 0
  r.l *= alpha;
  r.acc.x *= alpha;
  r.acc.y *= alpha;
  r.acc.z *= alpha;
  r.acc.w *= alpha;
  r.mx = m_new;
}

// "Many mask" launches (MANY = true; common.h, select_mask): one topology per batch element,
// shared by its `heads` replicas, every mask and replica in ONE launch.  The plan holds one
// region per mask (row_ok, chunk table: spmm_chunk_table_masks_kernel) and the masks' start
// order (mask_start_word).  The replicas are dealt over the XCDs whole (their row blocks
// share K and V: one L2), several masks to each XCD (xcd_spread_replicas_index), and the
// heads of the densest masks start first: their workgroups take several times the mean,
// and started last they would run on alone.  MANY = false is the single-mask code as it was.
__host__ __device__ __forceinline__ int64_t mask_plan_ints(int slots, int nchunks) {
  // one mask's region: row_ok (row_ok_bytes), the chunk table, the spare start-order word;
  // in 256-byte steps
  const int64_t ints = (slots + 63) / 64 * 64 + static_cast<int64_t>(nchunks + 1) * slots + 1;
  return (ints + 63) / 64 * 64;
}

struct WorkItem {
  int mblock, replica;
};
// Grid work -> (row block, replica) of a many-mask launch, and the replica's topology and
// plan; `nonzeros` becomes the mask's entry count.
__device__ __forceinline__ WorkItem many_mask_work(int heads, int m, int slots, int nchunks,
                                                   int& nonzeros,
                                                   const int* __restrict__& row_indices,
                                                   const int* __restrict__& row_offsets,
                                                   const int* __restrict__& column_indices,
                                                   const int* __restrict__& table,
                                                   const int* __restrict__& row_ok) {
  const int64_t plan_ints = mask_plan_ints(slots, nchunks);
  const unsigned long long work = xcd_spread_replicas_index(gridDim.x, gridDim.y);
  const int mblock = static_cast<int>(work % gridDim.x);
  int replica = static_cast<int>(work / gridDim.x);
  replica = row_ok[mask_start_word(replica / heads, plan_ints)] * heads + replica % heads;
  const MaskPlace place = select_mask(heads, replica, m, 0, row_offsets);
  row_offsets += static_cast<int64_t>(place.mask) * (m + 1);
  row_indices += static_cast<int64_t>(place.mask) * m;
  column_indices += place.first;
  table += place.mask * plan_ints;
  row_ok += place.mask * plan_ints;
  nonzeros = place.nonzeros;
  return WorkItem{mblock, replica};
}

// Drop: attention dropout (philox.h), DROP = the pack holds one DropArgs.  The lane that
// owns entry e16 of a window owns CSR position ps + w0 + e16 and decides whether it is kept
// (replica r = b * heads + h); the row sum still takes every entry (lse is that of the
// undropped scores), only the weight handed to step 3 becomes 0 for a dropped entry, and
// finish() applies 1 / l and the keep scale together.  DROP is a trailing parameter pack, not
// a bool and an argument, so that the instances without it keep their argument list.
template <typename... D>
__device__ __forceinline__ DropArgs drop_of(D... d) {
  if constexpr (sizeof...(D) == 0) return DropArgs{};
  else return (d, ...);
}

// T: storage type of q, k, v (Storage<T>); TO: of the context (float, or T).
// MANY = false: one mask for the grid's replicas replica0 .. replica0 + gridDim.y - 1 (a
// slice of the call's), `nonzeros` its entry count.  MANY = true: batch element b uses mask
// b; `nonzeros` and `replica0` are not used (each mask's count is read from its row_offsets,
// and the grid holds every replica).
// The body stays in the __global__ function: moved into an inlined device function it
// compiles to other code (§3.9a of DESIGN.md).
template <typename T, typename TO, bool MANY, typename... Drop>
__global__ __launch_bounds__(kThreads) void sparse_attention_kernel(
    int m, int n, int nonzeros, int slots, int nchunks, int heads, int replica0,
    const int* __restrict__ row_indices, const int* __restrict__ row_offsets,
    const int* __restrict__ column_indices, const int* __restrict__ table,
    const int* __restrict__ row_ok, HeadView qv, HeadView kv, HeadView vv, float scale,
    HeadView ov, float* __restrict__ lse, int64_t lse_stride, Drop... drop_arg) {
  constexpr bool DROP = sizeof...(Drop) > 0;
  const DropArgs drop = drop_of(drop_arg...);
  using S = Storage<T>;
  using V4 = typename S::V4;
  __shared__ __attribute__((aligned(16))) T tile[2][2 * kTile];  // [buffer][K rows | V rows]

  const int lane = threadIdx.x % kWave;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int g = lane >> 4, i = lane & 15;
  const int qd = i >> 2, tq = i & 3;   // quad of the row group, lane of the quad
  const int e16 = 4 * tq + qd;         // this lane's entry of a 16-entry window
  // (the row blocks of a replica read the same K and V: one XCD, see xcd_local_index)
  WorkItem item;
  if constexpr (MANY) {
    item = many_mask_work(heads, m, slots, nchunks, nonzeros, row_indices, row_offsets,
                          column_indices, table, row_ok);
  } else {
    const unsigned long long work = xcd_local_index();
    item = WorkItem{static_cast<int>(work % gridDim.x), replica0 + static_cast<int>(work / gridDim.x)};
  }
  const int mblock = item.mblock;
  const int replica = item.replica;
  PhiloxKey key{};
  if constexpr (DROP) key = philox_key(drop, blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0);
  const int drop_r = replica;
  const int64_t b = S::batch_of(replica, heads), h = replica - b * heads;
  const T* __restrict__ q = static_cast<const T*>(qv.base) + (b * qv.batch + h * qv.head);
  const T* __restrict__ k = static_cast<const T*>(kv.base) + (b * kv.batch + h * kv.head);
  const T* __restrict__ v = static_cast<const T*>(vv.base) + (b * vv.batch + h * vv.head);
  TO* __restrict__ out = static_cast<TO*>(const_cast<void*>(ov.base)) + (b * ov.batch + h * ov.head);
  if (lse != nullptr) lse += replica * lse_stride;
  const unsigned q_rs = static_cast<unsigned>(qv.row), k_rs = static_cast<unsigned>(kv.row),
                 v_rs = static_cast<unsigned>(vv.row), o_rs = static_cast<unsigned>(ov.row);
  const int slot0 = mblock * kBM + wave * (kRQ * 4);
  const int last = nonzeros - 1;

  RowAcc<T> st[kRQ];
  int my_row[kRQ];
#pragma unroll
  for (int t = 0; t < kRQ; ++t) {
    const int entry = dealt_index(slot0 + 4 * t + g, slots, kBM);
    my_row[t] = entry < m ? row_indices[entry] : -1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      V4 qs = {};
      if (my_row[t] >= 0)
        qs = *reinterpret_cast<const V4*>(q + (S::row(my_row[t], q_rs) + 16 * tq + 4 * ((c + qd) & 3)));
      st[t].q[c] = S::keep_q(qs, scale);
    }
    st[t].acc = make_float4(0.f, 0.f, 0.f, 0.f);
    st[t].mx = -INFINITY;
    st[t].l = 0.f;
  }

  auto finish = [&]() {
#pragma unroll
    for (int t = 0; t < kRQ; ++t) {
      if (my_row[t] < 0) continue;
      float inv = st[t].l > 0.f ? 1.f / st[t].l : 0.f;  // rows without entries give zeros
      if constexpr (DROP) inv *= drop.scale;
      const f4v r = {st[t].acc.x * inv, st[t].acc.y * inv, st[t].acc.z * inv, st[t].acc.w * inv};
      *reinterpret_cast<typename Vec4<TO>::type*>(out + (S::row(my_row[t], o_rs) + 4 * i)) =
          __builtin_convertvector(r, typename Vec4<TO>::type);
      if (lse != nullptr && i == 0)
        lse[my_row[t]] = st[t].l > 0.f ? st[t].mx + __logf(st[t].l) : -INFINITY;
    }
  };

  if constexpr (MANY) {
    if (nonzeros == 0) {   // a mask without entries (none of its column_indices is read)
      finish();
      return;
    }
  }

  // Row blocks whose columns do not ascend inside rows: order-independent path,
  // one entry at a time, K and V rows gathered from global memory.
  if (!block_rows_ok(row_ok, mblock * kBM, kBM)) {
    for (int t = 0; t < kRQ; ++t) {
      const int p0 = my_row[t] >= 0 ? row_offsets[my_row[t]] : 0;
      const int p1 = my_row[t] >= 0 ? row_offsets[my_row[t] + 1] : 0;
      f4v q16 = {0.f, 0.f, 0.f, 0.f};   // elements 4i .. 4i+3 of scale * q
      if (my_row[t] >= 0) q16 = load4(q + (S::row(my_row[t], q_rs) + 4 * i)) * scale;
      for (int p = p0; p < p1; ++p) {
        const int col = column_indices[p];
        const f4v kf = load4(k + (S::row(col, k_rs) + 4 * i));
        const f4v vf = load4(v + (S::row(col, v_rs) + 4 * i));
        const float s = group_sum<16>(dot4(q16, kf));
        if (s > st[t].mx) rescale(st[t], s);
        const float e = __expf(s - st[t].mx);
        st[t].l += e;
        float ek = e;
        if constexpr (DROP) ek = philox_keep(key, drop.threshold, drop_r, p) ? e : 0.f;
        st[t].acc.x = fmaf(ek, vf.x, st[t].acc.x);
        st[t].acc.y = fmaf(ek, vf.y, st[t].acc.y);
        st[t].acc.z = fmaf(ek, vf.z, st[t].acc.z);
        st[t].acc.w = fmaf(ek, vf.w, st[t].acc.w);
      }
    }
    finish();
    return;
  }

  const int* __restrict__ my_table = table + slot0 + g;
  int ps[kRQ], pe[kRQ], wcol[kRQ][kWin];
#pragma unroll
  for (int t = 0; t < kRQ; ++t) {
    ps[t] = my_table[4 * t];
    pe[t] = my_table[slots + 4 * t];
#pragma unroll
    for (int w = 0; w < kWin; ++w) wcol[t][w] = column_indices[min(ps[t] + 16 * w + e16, last)];
  }

  const unsigned k_bytes = S::row_bytes(k_rs), v_bytes = S::row_bytes(v_rs);
  stage_kv(tile[0], k, k_bytes, v, v_bytes, n, 0, wave, lane);
  wait_vm<0>();
  __syncthreads();

  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < nchunks;
    if (more) stage_kv(tile[buf ^ 1], k, k_bytes, v, v_bytes, n, (c + 1) * kBK, wave, lane);

    int pe_next[kRQ], ncol[kRQ][kWin];
#pragma unroll
    for (int t = 0; t < kRQ; ++t) {
      pe_next[t] = more ? my_table[static_cast<int64_t>(c + 2) * slots + 4 * t] : pe[t];
#pragma unroll
      for (int w = 0; w < kWin; ++w)
        ncol[t][w] = more ? column_indices[min(pe[t] + 16 * w + e16, last)] : 0;
    }

    const char* __restrict__ v_base =
        reinterpret_cast<const char*>(&tile[buf][0] + kTile) + i * 4 * sizeof(T);
    const int jc = c * kBK;
    const int k_lds = static_cast<int>(static_cast<unsigned>(
        reinterpret_cast<uintptr_t>(AS_LDS(&tile[buf][0]))));   // LDS byte address of the K tile

#pragma unroll
    for (int t = 0; t < kRQ; ++t) {
      const int cnt = pe[t] - ps[t];  // this group's row; the same in its 16 lanes

      auto window = [&](int ecol, int w0) {
        const int left = cnt - w0;
        if (left <= 0) return;
        const bool valid = e16 < left;
        const int roff = valid ? ((ecol - jc) * S::kRowBytes) : 0;

        // 1. scores, quad form: step S = entries 4S .. 4S+3, one per quad
        float s = 0.f;
        const int kq = k_lds + (S::kRowBytes / 4) * tq;   // this lane's quarter of tile row 0
        auto scores4 = [&](auto Sc) {
          constexpr int kS = decltype(Sc)::value;
          V4 bk[4];
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4)
            bk[c4] = *reinterpret_cast<const __attribute__((address_space(3))) V4*>(
                static_cast<unsigned>(quad_bcast_add<kS>(roff, kq + (S::kRowBytes / 16) * ((c4 + qd) & 3))));
          v2f a2 = {0.f, 0.f};
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4) S::mac(a2, st[t].q[c4], bk[c4]);
          const float total = group_sum<4>(a2.x + a2.y);
          s = (tq == kS) ? total : s;
        };
        scores4(std::integral_constant<int, 0>{});
        if (left > 4) scores4(std::integral_constant<int, 1>{});
        if (left > 8) scores4(std::integral_constant<int, 2>{});
        if (left > 12) scores4(std::integral_constant<int, 3>{});
        s = valid ? S::score(s, scale) : -INFINITY;

        // 2. online softmax over the window (at least one entry is valid)
        const float m_new = fmaxf(st[t].mx, group_max<16>(s));
        rescale(st[t], m_new);
        const float e = valid ? __expf(s - m_new) : 0.f;
        st[t].l += group_sum<16>(e);

        // 3. weighted V rows; padded entries carry weight 0 and offset 0
        float ek = e;
        if constexpr (DROP) ek = philox_keep(key, drop.threshold, drop_r, ps[t] + w0 + e16) ? e : 0.f;
        const entry_pair ent = make_entry(roff, ek);
        float a4[4] = {st[t].acc.x, st[t].acc.y, st[t].acc.z, st[t].acc.w};
        auto values4 = [&](auto G) {
          constexpr int kG = decltype(G)::value;
          // (entries kG .. kG+3 of the window sit in lanes kG/4, 4 + kG/4, 8 + kG/4, 12 + kG/4)
          const entry_pair e0 = row_bcast_entry<0 + kG / 4>(ent), e1 = row_bcast_entry<4 + kG / 4>(ent);
          const entry_pair e2 = row_bcast_entry<8 + kG / 4>(ent), e3 = row_bcast_entry<12 + kG / 4>(ent);
          const f4v b0 = load4(reinterpret_cast<const T*>(v_base + entry_off(e0)));
          const f4v b1 = load4(reinterpret_cast<const T*>(v_base + entry_off(e1)));
          const f4v b2 = load4(reinterpret_cast<const T*>(v_base + entry_off(e2)));
          const f4v b3 = load4(reinterpret_cast<const T*>(v_base + entry_off(e3)));
          SPUTNIK_HIP_FMA4(a4, entry_val(e0), b0);
          SPUTNIK_HIP_FMA4(a4, entry_val(e1), b1);
          SPUTNIK_HIP_FMA4(a4, entry_val(e2), b2);
          SPUTNIK_HIP_FMA4(a4, entry_val(e3), b3);
        };
        values4(std::integral_constant<int, 0>{});
        if (left > 4) values4(std::integral_constant<int, 4>{});
        if (left > 8) values4(std::integral_constant<int, 8>{});
        if (left > 12) values4(std::integral_constant<int, 12>{});
        st[t].acc = make_float4(a4[0], a4[1], a4[2], a4[3]);
      };
#pragma unroll
      for (int w = 0; w < kWin; ++w) window(wcol[t][w], 16 * w);
      // more than 32 entries of one row inside one chunk: fetch on demand
      const int longest = max(max(__builtin_amdgcn_readlane(cnt, 0), __builtin_amdgcn_readlane(cnt, 16)),
                              max(__builtin_amdgcn_readlane(cnt, 32), __builtin_amdgcn_readlane(cnt, 48)));
      for (int w0 = 16 * kWin; w0 < longest; w0 += 16)
        window(column_indices[min(ps[t] + w0 + e16, last)], w0);
    }

#pragma unroll
    for (int t = 0; t < kRQ; ++t) {
      ps[t] = pe[t];
      pe[t] = pe_next[t];
#pragma unroll
      for (int w = 0; w < kWin; ++w) wcol[t][w] = ncol[t][w];
    }
    wait_vm<0>();     // the next K/V tiles have landed
    __syncthreads();  // ... for every wave, and the current buffer is free
  }
  finish();
}

inline int slots_of(int m) { return ceil_div(m, kBM) * kBM; }
inline int chunks_of(int n) { return ceil_div(n, kBK); }

bool supported(int m, int n, int d, int nonzeros) {
  return d == kD && m > 0 && n > 0 && nonzeros > 0 &&
         static_cast<int64_t>(n) * kD * 4 < (int64_t{1} << 32);
}

bool half_code(int t) { return t == SPUTNIK_HIP_F16 || t == SPUTNIK_HIP_BF16; }

// Everything the kernel assumes about half head views, checked on the host: a served
// mask (supported), 16-byte aligned bases and strides, non-negative strides, and every
// replica's extent below 2^32 bytes (the kernel's in-replica offsets are 32-bit).
bool view_ok(const HeadView& w, int rows, int elem_bytes) {
  if (w.base == nullptr || !aligned_to(w.base, 16)) return false;
  if (w.batch < 0 || w.head < 0 || w.row < 0) return false;
  if ((w.batch * elem_bytes) % 16 != 0 || (w.head * elem_bytes) % 16 != 0 || (w.row * elem_bytes) % 16 != 0)
    return false;
  return (static_cast<int64_t>(rows - 1) * w.row + kD) * elem_bytes < (int64_t{1} << 32);
}

bool heads_served(int m, int n, int d, int nonzeros, int batch, int heads, int dtype, int out_type,
                  const HeadView& q, const HeadView& k, const HeadView& v, const HeadView& o) {
  if (!supported(m, n, d, nonzeros) || !half_code(dtype)) return false;
  if (out_type != SPUTNIK_HIP_F32 && out_type != dtype) return false;
  if (batch <= 0 || heads <= 0 || static_cast<int64_t>(batch) * heads >= (int64_t{1} << 31)) return false;
  return view_ok(q, m, 2) && view_ok(k, n, 2) && view_ok(v, n, 2) &&
         view_ok(o, m, out_type == SPUTNIK_HIP_F32 ? 4 : 2);
}

}  // namespace
}  // namespace sputnik_hip

using namespace sputnik_hip;

// ---------------------------------------------------------------------------
// Host side.  Every forward entry point (operand layout x mask layout x planned x dropout)
// fills one ForwardCall and goes through forward(): the checks, the pre-pass and the loop
// over grid slices are written once, launch() picks the kernel instance.
// ---------------------------------------------------------------------------
namespace {

struct ForwardCall {
  bool many;             // one mask per batch element (`masks` of them), else one for every replica
  bool half;             // operands are head views of `dtype`, else float32 with heads = 1
  int masks;
  const int* nonzeros;   // [masks], or the address of the single mask's count
  int m, n, d, batch, heads;   // float32 operands: batch = replicas
  const int *row_indices, *row_offsets, *column_indices;
  int dtype, out_type;
  HeadView q, k, v, o;   // float32 operands: (0, replica stride, 64), one batch element of R heads
  float scale;
  float* lse;
  int64_t lse_stride;
  void* workspace;
  size_t workspace_bytes;
  bool planned;          // the workspace holds the pre-pass results already
  hipStream_t stream;
  const DropArgs* drop;
};

struct Plan {   // the workspace as the kernel reads it
  int slots, nchunks;
  const int *row_ok, *table;
};

size_t mask_plan_bytes(int m, int n) {   // one mask's region of a many-mask plan
  return sizeof(int) * static_cast<size_t>(mask_plan_ints(slots_of(m), chunks_of(n)));
}

// Checks every many-mask entry point shares.  *largest = the largest entry count (the
// kernels serve the launch when they serve it for the densest mask).
int many_mask_args(int masks, int m, int n, int d, const int* nonzeros, int replicas, int* largest) {
  if (masks <= 0 || m < 0 || n < 0 || d < 0 || replicas < 0 || nonzeros == nullptr)
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  if (replicas % masks != 0) return SPUTNIK_HIP_INVALID_ARGUMENT;
  *largest = 0;
  for (int i = 0; i < masks; ++i) {
    if (nonzeros[i] < 0) return SPUTNIK_HIP_INVALID_ARGUMENT;
    *largest = max(*largest, nonzeros[i]);
  }
  return 0;
}

// One launch holds every replica (grid y; the masks' start order covers the whole batch).
// A launch with no entry at all is served too: every mask gives zeros.
bool many_mask_supported(int masks, int m, int n, int d, int largest, int replicas) {
  return masks <= kMaxGridYZ && replicas <= kMaxGridYZ && supported(m, n, d, max(largest, 1));
}

size_t many_mask_workspace(int masks, int m, int n, int d, int largest) {
  if (masks <= 0 || !many_mask_supported(masks, m, n, d, largest, masks)) return 0;
  return static_cast<size_t>(masks) * mask_plan_bytes(m, n);
}

size_t plan_bytes(int m, int n, int d, int nonzeros) {
  if (!supported(m, n, d, nonzeros)) return 0;
  return row_ok_bytes(slots_of(m)) + sizeof(int) * static_cast<size_t>(chunks_of(n) + 1) * slots_of(m);
}

// The topology-only pre-pass: row_ok and the chunk table, one region per mask.
int prepass(bool many, int masks, int m, int n, const int* row_indices, const int* row_offsets,
            const int* column_indices, void* workspace, hipStream_t stream) {
  const int slots = slots_of(m);
  int* row_ok = static_cast<int*>(workspace);
  int* table = reinterpret_cast<int*>(static_cast<char*>(workspace) + row_ok_bytes(slots));
  if (many)
    hipLaunchKernelGGL((spmm_chunk_table_masks_kernel<kBK>), dim3(ceil_div(slots, 4), masks), dim3(256),
                       0, stream, m, n, slots, kBM, chunks_of(n), row_indices, row_offsets,
                       column_indices, table, row_ok,
                       static_cast<int64_t>(mask_plan_bytes(m, n) / sizeof(int)));
  else
    hipLaunchKernelGGL((spmm_chunk_table_kernel<kBK>), dim3(ceil_div(slots, 4)), dim3(256), 0, stream,
                       m, n, slots, kBM, chunks_of(n), row_indices, row_offsets, column_indices, table,
                       row_ok);
  return launch_status();
}

// Replicas r0 .. r0 + count - 1 of a call (every replica of a many-mask one): the views
// stay, the kernel numbers its replicas from r0 itself.  `heads` is what the many-mask form
// deals by: the replicas per mask.
template <typename T, typename TO, bool MANY, typename... Drop>
void launch_kernel(const ForwardCall& c, const Plan& p, int r0, int count, Drop... drop) {
  const int heads = c.half ? c.heads : MANY ? c.batch / c.masks : 1;
  hipLaunchKernelGGL((sparse_attention_kernel<T, TO, MANY, Drop...>), dim3(p.slots / kBM, count),
                     dim3(kThreads), 0, c.stream, c.m, c.n, MANY ? 0 : *c.nonzeros, p.slots, p.nchunks,
                     heads, r0, c.row_indices, c.row_offsets, c.column_indices, p.table, p.row_ok, c.q,
                     c.k, c.v, c.scale, c.o, c.lse, c.lse_stride, drop...);
}

// Picks the kernel instance from (half, dtype, out_type, many, drop != nullptr) and launches it.
void launch(const ForwardCall& c, const Plan& p, int r0, int count) {
  auto pick = [&](auto many, auto... drop) {
    constexpr bool MANY = decltype(many)::value;
    if (!c.half) launch_kernel<float, float, MANY>(c, p, r0, count, drop...);
    else if (c.dtype == SPUTNIK_HIP_F16 && c.out_type == SPUTNIK_HIP_F32)
      launch_kernel<_Float16, float, MANY>(c, p, r0, count, drop...);
    else if (c.dtype == SPUTNIK_HIP_F16) launch_kernel<_Float16, _Float16, MANY>(c, p, r0, count, drop...);
    else if (c.out_type == SPUTNIK_HIP_F32) launch_kernel<__bf16, float, MANY>(c, p, r0, count, drop...);
    else launch_kernel<__bf16, __bf16, MANY>(c, p, r0, count, drop...);
  };
  if (c.drop == nullptr) {
    if (c.many) pick(std::true_type{});
    else pick(std::false_type{});
    return;
  }
  DropArgs dr = *c.drop;   // only the first launch publishes the rng state
  if (r0 > 0) dr.rng_state_out = nullptr;
  if (c.many) pick(std::true_type{}, dr);
  else pick(std::false_type{}, dr);
}

// A float32 single-mask call whose every row is empty: zeros (and -inf log-sum-exp).
int fill_empty(const ForwardCall& c) {
  if (c.drop != nullptr) {
    const int e = publish_rng_state(*c.drop, c.stream);
    if (e != 0) return e;
  }
  float* out = const_cast<float*>(static_cast<const float*>(c.o.base));
  for (int r = 0; r < c.batch; ++r) {
    hipError_t e = hipMemsetAsync(out + r * c.o.head, 0, sizeof(float) * c.m * c.d, c.stream);
    if (e != hipSuccess) return static_cast<int>(e);
    if (c.lse != nullptr) {
      e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c.lse + r * c.lse_stride),
                            static_cast<int>(0xff800000u), c.m, c.stream);
      if (e != hipSuccess) return static_cast<int>(e);
    }
  }
  return 0;
}

// What a call returns, in the order the conditions are tried.  The four forms (float32 or
// half operands x one or many masks) came from four functions and do not agree everywhere;
// the differences are kept and marked (*).  INVALID = SPUTNIK_HIP_INVALID_ARGUMENT,
// UNSUPPORTED = SPUTNIK_HIP_UNSUPPORTED, "empty" = 0 after publishing the rng state when
// dropping (every form), replicas = batch * heads.
//
//   float32, one mask     1. m, n, d, nonzeros or replicas < 0: INVALID
//                         2. m == 0 or replicas == 0: empty
//                     (*) 3. nonzeros == 0 or n == 0: served here -- rng state published, out
//                            set to 0, lse to -inf, no kernel and no look at the workspace
//                         4. not supported(m, n, d, nonzeros), a base not 16-byte aligned or
//                            a stride not a multiple of 4: UNSUPPORTED
//                         5. workspace NULL, unaligned or too small: INVALID
//   half, one mask        1. as above, with batch and heads for replicas
//                         2. m == 0, batch == 0 or heads == 0: empty
//                     (*) 3. no branch for nonzeros == 0 or n == 0: heads_served refuses them
//                            with everything else it refuses (types, views, batch * heads >=
//                            2^31): UNSUPPORTED
//                         4. workspace: INVALID
//   float32, many masks   1. masks <= 0, m, n, d or replicas < 0, nonzeros NULL, replicas not
//                            a multiple of masks, a count < 0: INVALID
//                         2. m == 0 or replicas == 0: empty
//                     (*) 3. more than 65535 masks or replicas, not supported for the densest
//                            mask -- counted as 1 entry when all are empty, so a launch
//                            without entries IS served, by the kernel -- or alignment as for
//                            one mask: UNSUPPORTED.  (n == 0 is therefore UNSUPPORTED here.)
//                         4. workspace: INVALID
//   half, many masks  (*) 0. batch or heads < 0: INVALID; then batch * heads >= 2^31:
//                            UNSUPPORTED; then batch != masks: INVALID -- all before step 1, so
//                            the overflow is UNSUPPORTED even with otherwise invalid arguments
//                         1. as float32 many masks
//                         2. m == 0 or heads == 0: empty (batch == 0 was INVALID: masks <= 0)
//                         3. as float32 many masks, with heads_served for the densest mask
//                            (at least 1) in place of the alignment: UNSUPPORTED
//                         4. workspace: INVALID
// Then every form returns the first failing launch's hipError_t (pre-pass unless planned,
// kernel), else 0.
int forward(const ForwardCall& c) {
  // (exact wherever it is used: the half forms refuse a product of 2^31 or more before)
  const int replicas = static_cast<int>(static_cast<int64_t>(c.batch) * c.heads);
  int largest = 0;   // entries of the densest mask
  if (c.many) {
    if (c.half) {
      if (c.batch < 0 || c.heads < 0) return SPUTNIK_HIP_INVALID_ARGUMENT;
      if (static_cast<int64_t>(c.batch) * c.heads >= (int64_t{1} << 31)) return SPUTNIK_HIP_UNSUPPORTED;
      if (c.batch != c.masks) return SPUTNIK_HIP_INVALID_ARGUMENT;
    }
    const int st = many_mask_args(c.masks, c.m, c.n, c.d, c.nonzeros, replicas, &largest);
    if (st != 0) return st;
  } else {
    largest = *c.nonzeros;
    if (c.m < 0 || c.n < 0 || c.d < 0 || largest < 0 || c.batch < 0 || c.heads < 0)
      return SPUTNIK_HIP_INVALID_ARGUMENT;
  }
  if (c.m == 0 || c.batch == 0 || c.heads == 0)
    return c.drop != nullptr ? publish_rng_state(*c.drop, c.stream) : 0;
  if (!c.many && !c.half && (largest == 0 || c.n == 0)) return fill_empty(c);

  const int densest = c.many ? max(largest, 1) : largest;
  bool served = !c.many || many_mask_supported(c.masks, c.m, c.n, c.d, largest, replicas);
  if (c.half)
    served = served && heads_served(c.m, c.n, c.d, densest, c.batch, c.heads, c.dtype, c.out_type, c.q,
                                    c.k, c.v, c.o);
  else
    served = served && supported(c.m, c.n, c.d, densest) && aligned_to(c.q.base, 16) &&
             aligned_to(c.k.base, 16) && aligned_to(c.v.base, 16) && aligned_to(c.o.base, 16) &&
             c.q.head % 4 == 0 && c.k.head % 4 == 0 && c.v.head % 4 == 0 && c.o.head % 4 == 0;
  if (!served) return SPUTNIK_HIP_UNSUPPORTED;
  const size_t need = c.many ? many_mask_workspace(c.masks, c.m, c.n, c.d, largest)
                             : plan_bytes(c.m, c.n, c.d, largest);
  if (c.workspace == nullptr || !aligned_to(c.workspace, 16) || c.workspace_bytes < need)
    return SPUTNIK_HIP_INVALID_ARGUMENT;

  if (!c.planned) {
    const int st = prepass(c.many, c.masks, c.m, c.n, c.row_indices, c.row_offsets, c.column_indices,
                           c.workspace, c.stream);
    if (st != 0) return st;
  }
  const int slots = slots_of(c.m);
  const Plan p{slots, chunks_of(c.n), static_cast<const int*>(c.workspace),
               reinterpret_cast<const int*>(static_cast<const char*>(c.workspace) + row_ok_bytes(slots))};
  // (many masks: one launch, the replicas fit the grid)
  for (int r0 = 0; r0 < replicas; r0 += kMaxGridYZ) {
    launch(c, p, r0, min(replicas - r0, kMaxGridYZ));
    const int st = launch_status();
    if (st != 0) return st;
  }
  return 0;
}

// The forms with attention dropout (sputnik_hip.h, "Attention dropout"): the same call with
// the DROP kernels; p = 0 is the form without.
int forward_dropout(ForwardCall c, double p, const sputnik_hip_philox_state& rng, int64_t* rng_state_out) {
  DropArgs drop;
  if (!drop_args(p, rng, rng_state_out, &drop)) return SPUTNIK_HIP_INVALID_ARGUMENT;
  if (p > 0.0) c.drop = &drop;
  return forward(c);
}

// The argument lists of the C entry points as a ForwardCall: float32 operands ...
ForwardCall float_call(bool many, int masks, const int* nonzeros, int m, int n, int d, int replicas,
                       const int* row_indices, const int* row_offsets, const int* column_indices,
                       const float* q, int64_t q_stride, const float* k, int64_t k_stride, const float* v,
                       int64_t v_stride, float scale, float* out, int64_t out_stride, float* lse,
                       int64_t lse_stride, const void* workspace, size_t workspace_bytes, bool planned,
                       hipStream_t stream) {
  return ForwardCall{many, /*half=*/false, masks, nonzeros, m, n, d, replicas, /*heads=*/1,
                     row_indices, row_offsets, column_indices, SPUTNIK_HIP_F32, SPUTNIK_HIP_F32,
                     HeadView{q, 0, q_stride, kD}, HeadView{k, 0, k_stride, kD}, HeadView{v, 0, v_stride, kD},
                     HeadView{out, 0, out_stride, kD}, scale, lse, lse_stride, const_cast<void*>(workspace),
                     workspace_bytes, planned, stream, /*drop=*/nullptr};
}

// ... and half head views.
ForwardCall heads_call(bool many, int masks, const int* nonzeros, int m, int n, int d, int batch, int heads,
                       const int* row_indices, const int* row_offsets, const int* column_indices, int dtype,
                       const void* q, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride,
                       const void* k, int64_t k_batch_stride, int64_t k_head_stride, int64_t k_row_stride,
                       const void* v, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride,
                       float scale, void* out, int out_type, int64_t out_batch_stride,
                       int64_t out_head_stride, int64_t out_row_stride, float* lse, int64_t lse_stride,
                       const void* workspace, size_t workspace_bytes, bool planned, hipStream_t stream) {
  return ForwardCall{many, /*half=*/true, masks, nonzeros, m, n, d, batch, heads, row_indices, row_offsets,
                     column_indices, dtype, out_type,
                     HeadView{q, q_batch_stride, q_head_stride, q_row_stride},
                     HeadView{k, k_batch_stride, k_head_stride, k_row_stride},
                     HeadView{v, v_batch_stride, v_head_stride, v_row_stride},
                     HeadView{out, out_batch_stride, out_head_stride, out_row_stride}, scale, lse,
                     lse_stride, const_cast<void*>(workspace), workspace_bytes, planned, stream,
                     /*drop=*/nullptr};
}

}  // namespace

extern "C" {

int sputnik_hip_sparse_attention_supported(int m, int n, int d, int nonzeros) {
  return supported(m, n, d, nonzeros) ? 1 : 0;
}

size_t sputnik_hip_sparse_attention_workspace_bytes(int m, int n, int d, int nonzeros) {
  return plan_bytes(m, n, d, nonzeros);
}

int sputnik_hip_sparse_attention_plan(int m, int n, int d, int nonzeros, const int* row_indices,
                                      const int* row_offsets, const int* column_indices,
                                      void* workspace, size_t workspace_bytes,
                                      sputnik_hip_stream_t stream) {
  if (m < 0 || n < 0 || d < 0 || nonzeros < 0) return SPUTNIK_HIP_INVALID_ARGUMENT;
  if (!supported(m, n, d, nonzeros)) return SPUTNIK_HIP_UNSUPPORTED;
  if (workspace == nullptr || !aligned_to(workspace, 16) ||
      workspace_bytes < plan_bytes(m, n, d, nonzeros))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  return prepass(false, 0, m, n, row_indices, row_offsets, column_indices, workspace, stream);
}

int sputnik_hip_sparse_attention_forward(int m, int n, int d, int nonzeros, int replicas,
                                         const int* row_indices, const int* row_offsets,
                                         const int* column_indices, const float* q,
                                         int64_t q_stride, const float* k, int64_t k_stride,
                                         const float* v, int64_t v_stride, float scale,
                                         float* out, int64_t out_stride, float* lse,
                                         int64_t lse_stride, void* workspace,
                                         size_t workspace_bytes, sputnik_hip_stream_t stream) {
  return forward(float_call(false, 0, &nonzeros, m, n, d, replicas, row_indices, row_offsets,
                            column_indices, q, q_stride, k, k_stride, v, v_stride, scale, out,
                            out_stride, lse, lse_stride, workspace, workspace_bytes,
                            /*planned=*/false, stream));
}

int sputnik_hip_sparse_attention_forward_planned(
    int m, int n, int d, int nonzeros, int replicas, const int* row_indices,
    const int* row_offsets, const int* column_indices, const float* q, int64_t q_stride,
    const float* k, int64_t k_stride, const float* v, int64_t v_stride, float scale, float* out,
    int64_t out_stride, float* lse, int64_t lse_stride, const void* workspace,
    size_t workspace_bytes, sputnik_hip_stream_t stream) {
  return forward(float_call(false, 0, &nonzeros, m, n, d, replicas, row_indices, row_offsets,
                            column_indices, q, q_stride, k, k_stride, v, v_stride, scale, out,
                            out_stride, lse, lse_stride, workspace, workspace_bytes,
                            /*planned=*/true, stream));
}

int sputnik_hip_sparse_attention_forward_dropout(
    int m, int n, int d, int nonzeros, int replicas, const int* row_indices, const int* row_offsets,
    const int* column_indices, const float* q, int64_t q_stride, const float* k, int64_t k_stride,
    const float* v, int64_t v_stride, float scale, float* out, int64_t out_stride, float* lse,
    int64_t lse_stride, double p, sputnik_hip_philox_state rng, int64_t* rng_state_out,
    void* workspace, size_t workspace_bytes, sputnik_hip_stream_t stream) {
  return forward_dropout(float_call(false, 0, &nonzeros, m, n, d, replicas, row_indices, row_offsets,
                                    column_indices, q, q_stride, k, k_stride, v, v_stride, scale, out,
                                    out_stride, lse, lse_stride, workspace, workspace_bytes,
                                    /*planned=*/false, stream),
                         p, rng, rng_state_out);
}

int sputnik_hip_sparse_attention_forward_planned_dropout(
    int m, int n, int d, int nonzeros, int replicas, const int* row_indices, const int* row_offsets,
    const int* column_indices, const float* q, int64_t q_stride, const float* k, int64_t k_stride,
    const float* v, int64_t v_stride, float scale, float* out, int64_t out_stride, float* lse,
    int64_t lse_stride, double p, sputnik_hip_philox_state rng, int64_t* rng_state_out,
    const void* workspace, size_t workspace_bytes, sputnik_hip_stream_t stream) {
  return forward_dropout(float_call(false, 0, &nonzeros, m, n, d, replicas, row_indices, row_offsets,
                                    column_indices, q, q_stride, k, k_stride, v, v_stride, scale, out,
                                    out_stride, lse, lse_stride, workspace, workspace_bytes,
                                    /*planned=*/true, stream),
                         p, rng, rng_state_out);
}

// ---- half storage, strided head views ----
int sputnik_hip_sparse_attention_heads_supported(
    int m, int n, int d, int nonzeros, int batch, int heads, int dtype, int out_type, const void* q,
    int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride, const void* k,
    int64_t k_batch_stride, int64_t k_head_stride, int64_t k_row_stride, const void* v,
    int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride, const void* out,
    int64_t out_batch_stride, int64_t out_head_stride, int64_t out_row_stride) {
  return heads_served(m, n, d, nonzeros, batch, heads, dtype, out_type,
                      HeadView{q, q_batch_stride, q_head_stride, q_row_stride},
                      HeadView{k, k_batch_stride, k_head_stride, k_row_stride},
                      HeadView{v, v_batch_stride, v_head_stride, v_row_stride},
                      HeadView{out, out_batch_stride, out_head_stride, out_row_stride})
             ? 1 : 0;
}

size_t sputnik_hip_sparse_attention_heads_workspace_bytes(int m, int n, int d, int nonzeros) {
  return plan_bytes(m, n, d, nonzeros);
}

int sputnik_hip_sparse_attention_heads_forward(
    int m, int n, int d, int nonzeros, int batch, int heads, const int* row_indices,
    const int* row_offsets, const int* column_indices, int dtype, const void* q,
    int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride, const void* k,
    int64_t k_batch_stride, int64_t k_head_stride, int64_t k_row_stride, const void* v,
    int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride, float scale, void* out,
    int out_type, int64_t out_batch_stride, int64_t out_head_stride, int64_t out_row_stride,
    float* lse, int64_t lse_stride, void* workspace, size_t workspace_bytes,
    sputnik_hip_stream_t stream) {
  return forward(heads_call(false, 0, &nonzeros, m, n, d, batch, heads, row_indices, row_offsets,
                            column_indices, dtype, q, q_batch_stride, q_head_stride, q_row_stride, k,
                            k_batch_stride, k_head_stride, k_row_stride, v, v_batch_stride, v_head_stride,
                            v_row_stride, scale, out, out_type, out_batch_stride, out_head_stride,
                            out_row_stride, lse, lse_stride, workspace, workspace_bytes,
                            /*planned=*/false, stream));
}

int sputnik_hip_sparse_attention_heads_forward_planned(
    int m, int n, int d, int nonzeros, int batch, int heads, const int* row_indices,
    const int* row_offsets, const int* column_indices, int dtype, const void* q,
    int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride, const void* k,
    int64_t k_batch_stride, int64_t k_head_stride, int64_t k_row_stride, const void* v,
    int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride, float scale, void* out,
    int out_type, int64_t out_batch_stride, int64_t out_head_stride, int64_t out_row_stride,
    float* lse, int64_t lse_stride, const void* workspace, size_t workspace_bytes,
    sputnik_hip_stream_t stream) {
  return forward(heads_call(false, 0, &nonzeros, m, n, d, batch, heads, row_indices, row_offsets,
                            column_indices, dtype, q, q_batch_stride, q_head_stride, q_row_stride, k,
                            k_batch_stride, k_head_stride, k_row_stride, v, v_batch_stride, v_head_stride,
                            v_row_stride, scale, out, out_type, out_batch_stride, out_head_stride,
                            out_row_stride, lse, lse_stride, workspace, workspace_bytes,
                            /*planned=*/true, stream));
}

int sputnik_hip_sparse_attention_heads_forward_dropout(
    int m, int n, int d, int nonzeros, int batch, int heads, const int* row_indices,
    const int* row_offsets, const int* column_indices, int dtype, const void* q,
    int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride, const void* k,
    int64_t k_batch_stride, int64_t k_head_stride, int64_t k_row_stride, const void* v,
    int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride, float scale, void* out,
    int out_type, int64_t out_batch_stride, int64_t out_head_stride, int64_t out_row_stride,
    float* lse, int64_t lse_stride, double p, sputnik_hip_philox_state rng, int64_t* rng_state_out,
    void* workspace, size_t workspace_bytes, sputnik_hip_stream_t stream) {
  return forward_dropout(
      heads_call(false, 0, &nonzeros, m, n, d, batch, heads, row_indices, row_offsets, column_indices,
                 dtype, q, q_batch_stride, q_head_stride, q_row_stride, k, k_batch_stride, k_head_stride,
                 k_row_stride, v, v_batch_stride, v_head_stride, v_row_stride, scale, out, out_type,
                 out_batch_stride, out_head_stride, out_row_stride, lse, lse_stride, workspace,
                 workspace_bytes, /*planned=*/false, stream),
      p, rng, rng_state_out);
}

int sputnik_hip_sparse_attention_heads_forward_planned_dropout(
    int m, int n, int d, int nonzeros, int batch, int heads, const int* row_indices,
    const int* row_offsets, const int* column_indices, int dtype, const void* q,
    int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride, const void* k,
    int64_t k_batch_stride, int64_t k_head_stride, int64_t k_row_stride, const void* v,
    int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride, float scale, void* out,
    int out_type, int64_t out_batch_stride, int64_t out_head_stride, int64_t out_row_stride,
    float* lse, int64_t lse_stride, double p, sputnik_hip_philox_state rng, int64_t* rng_state_out,
    const void* workspace, size_t workspace_bytes, sputnik_hip_stream_t stream) {
  return forward_dropout(
      heads_call(false, 0, &nonzeros, m, n, d, batch, heads, row_indices, row_offsets, column_indices,
                 dtype, q, q_batch_stride, q_head_stride, q_row_stride, k, k_batch_stride, k_head_stride,
                 k_row_stride, v, v_batch_stride, v_head_stride, v_row_stride, scale, out, out_type,
                 out_batch_stride, out_head_stride, out_row_stride, lse, lse_stride, workspace,
                 workspace_bytes, /*planned=*/true, stream),
      p, rng, rng_state_out);
}

// ---- many masks (sputnik_hip.h, "many mask" family): one topology per batch element, all of
// them served by ONE pre-pass launch and ONE attention launch ----
size_t sputnik_hip_sparse_attention_many_mask_workspace_bytes(int masks, int m, int n, int d,
                                                              int largest_nonzeros) {
  if (m < 0 || n < 0 || d < 0 || largest_nonzeros < 0) return 0;
  return many_mask_workspace(masks, m, n, d, largest_nonzeros);
}

int sputnik_hip_sparse_attention_many_mask_plan(int masks, int m, int n, int d, const int* nonzeros,
                                                const int* row_indices, const int* row_offsets,
                                                const int* column_indices, void* workspace,
                                                size_t workspace_bytes, sputnik_hip_stream_t stream) {
  int largest = 0;
  const int st = many_mask_args(masks, m, n, d, nonzeros, masks, &largest);
  if (st != 0) return st;
  if (!many_mask_supported(masks, m, n, d, largest, masks)) return SPUTNIK_HIP_UNSUPPORTED;
  if (workspace == nullptr || !aligned_to(workspace, 16) ||
      workspace_bytes < many_mask_workspace(masks, m, n, d, largest))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  if (m == 0) return 0;
  return prepass(true, masks, m, n, row_indices, row_offsets, column_indices, workspace, stream);
}

int sputnik_hip_sparse_attention_many_mask_forward(
    int masks, int m, int n, int d, const int* nonzeros, int replicas, const int* row_indices,
    const int* row_offsets, const int* column_indices, const float* q, int64_t q_stride,
    const float* k, int64_t k_stride, const float* v, int64_t v_stride, float scale, float* out,
    int64_t out_stride, float* lse, int64_t lse_stride, void* workspace, size_t workspace_bytes,
    sputnik_hip_stream_t stream) {
  return forward(float_call(true, masks, nonzeros, m, n, d, replicas, row_indices, row_offsets,
                            column_indices, q, q_stride, k, k_stride, v, v_stride, scale, out,
                            out_stride, lse, lse_stride, workspace, workspace_bytes,
                            /*planned=*/false, stream));
}

int sputnik_hip_sparse_attention_many_mask_forward_planned(
    int masks, int m, int n, int d, const int* nonzeros, int replicas, const int* row_indices,
    const int* row_offsets, const int* column_indices, const float* q, int64_t q_stride,
    const float* k, int64_t k_stride, const float* v, int64_t v_stride, float scale, float* out,
    int64_t out_stride, float* lse, int64_t lse_stride, const void* workspace,
    size_t workspace_bytes, sputnik_hip_stream_t stream) {
  return forward(float_call(true, masks, nonzeros, m, n, d, replicas, row_indices, row_offsets,
                            column_indices, q, q_stride, k, k_stride, v, v_stride, scale, out,
                            out_stride, lse, lse_stride, workspace, workspace_bytes,
                            /*planned=*/true, stream));
}

int sputnik_hip_sparse_attention_many_mask_forward_dropout(
    int masks, int m, int n, int d, const int* nonzeros, int replicas, const int* row_indices,
    const int* row_offsets, const int* column_indices, const float* q, int64_t q_stride,
    const float* k, int64_t k_stride, const float* v, int64_t v_stride, float scale, float* out,
    int64_t out_stride, float* lse, int64_t lse_stride, double p, sputnik_hip_philox_state rng,
    int64_t* rng_state_out, void* workspace, size_t workspace_bytes, sputnik_hip_stream_t stream) {
  return forward_dropout(float_call(true, masks, nonzeros, m, n, d, replicas, row_indices, row_offsets,
                                    column_indices, q, q_stride, k, k_stride, v, v_stride, scale, out,
                                    out_stride, lse, lse_stride, workspace, workspace_bytes,
                                    /*planned=*/false, stream),
                         p, rng, rng_state_out);
}

int sputnik_hip_sparse_attention_many_mask_forward_planned_dropout(
    int masks, int m, int n, int d, const int* nonzeros, int replicas, const int* row_indices,
    const int* row_offsets, const int* column_indices, const float* q, int64_t q_stride,
    const float* k, int64_t k_stride, const float* v, int64_t v_stride, float scale, float* out,
    int64_t out_stride, float* lse, int64_t lse_stride, double p, sputnik_hip_philox_state rng,
    int64_t* rng_state_out, const void* workspace, size_t workspace_bytes,
    sputnik_hip_stream_t stream) {
  return forward_dropout(float_call(true, masks, nonzeros, m, n, d, replicas, row_indices, row_offsets,
                                    column_indices, q, q_stride, k, k_stride, v, v_stride, scale, out,
                                    out_stride, lse, lse_stride, workspace, workspace_bytes,
                                    /*planned=*/true, stream),
                         p, rng, rng_state_out);
}

int sputnik_hip_sparse_attention_heads_many_mask_forward(
    int masks, int m, int n, int d, const int* nonzeros, int batch, int heads,
    const int* row_indices, const int* row_offsets, const int* column_indices, int dtype,
    const void* q, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride,
    const void* k, int64_t k_batch_stride, int64_t k_head_stride, int64_t k_row_stride,
    const void* v, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride,
    float scale, void* out, int out_type, int64_t out_batch_stride, int64_t out_head_stride,
    int64_t out_row_stride, float* lse, int64_t lse_stride, void* workspace,
    size_t workspace_bytes, sputnik_hip_stream_t stream) {
  return forward(heads_call(true, masks, nonzeros, m, n, d, batch, heads, row_indices, row_offsets,
                            column_indices, dtype, q, q_batch_stride, q_head_stride, q_row_stride, k,
                            k_batch_stride, k_head_stride, k_row_stride, v, v_batch_stride, v_head_stride,
                            v_row_stride, scale, out, out_type, out_batch_stride, out_head_stride,
                            out_row_stride, lse, lse_stride, workspace, workspace_bytes,
                            /*planned=*/false, stream));
}

int sputnik_hip_sparse_attention_heads_many_mask_forward_planned(
    int masks, int m, int n, int d, const int* nonzeros, int batch, int heads,
    const int* row_indices, const int* row_offsets, const int* column_indices, int dtype,
    const void* q, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride,
    const void* k, int64_t k_batch_stride, int64_t k_head_stride, int64_t k_row_stride,
    const void* v, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride,
    float scale, void* out, int out_type, int64_t out_batch_stride, int64_t out_head_stride,
    int64_t out_row_stride, float* lse, int64_t lse_stride, const void* workspace,
    size_t workspace_bytes, sputnik_hip_stream_t stream) {
  return forward(heads_call(true, masks, nonzeros, m, n, d, batch, heads, row_indices, row_offsets,
                            column_indices, dtype, q, q_batch_stride, q_head_stride, q_row_stride, k,
                            k_batch_stride, k_head_stride, k_row_stride, v, v_batch_stride, v_head_stride,
                            v_row_stride, scale, out, out_type, out_batch_stride, out_head_stride,
                            out_row_stride, lse, lse_stride, workspace, workspace_bytes,
                            /*planned=*/true, stream));
}

int sputnik_hip_sparse_attention_heads_many_mask_forward_dropout(
    int masks, int m, int n, int d, const int* nonzeros, int batch, int heads,
    const int* row_indices, const int* row_offsets, const int* column_indices, int dtype,
    const void* q, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride,
    const void* k, int64_t k_batch_stride, int64_t k_head_stride, int64_t k_row_stride,
    const void* v, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride,
    float scale, void* out, int out_type, int64_t out_batch_stride, int64_t out_head_stride,
    int64_t out_row_stride, float* lse, int64_t lse_stride, double p, sputnik_hip_philox_state rng,
    int64_t* rng_state_out, void* workspace, size_t workspace_bytes, sputnik_hip_stream_t stream) {
  return forward_dropout(
      heads_call(true, masks, nonzeros, m, n, d, batch, heads, row_indices, row_offsets, column_indices,
                 dtype, q, q_batch_stride, q_head_stride, q_row_stride, k, k_batch_stride, k_head_stride,
                 k_row_stride, v, v_batch_stride, v_head_stride, v_row_stride, scale, out, out_type,
                 out_batch_stride, out_head_stride, out_row_stride, lse, lse_stride, workspace,
                 workspace_bytes, /*planned=*/false, stream),
      p, rng, rng_state_out);
}

int sputnik_hip_sparse_attention_heads_many_mask_forward_planned_dropout(
    int masks, int m, int n, int d, const int* nonzeros, int batch, int heads,
    const int* row_indices, const int* row_offsets, const int* column_indices, int dtype,
    const void* q, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride,
    const void* k, int64_t k_batch_stride, int64_t k_head_stride, int64_t k_row_stride,
    const void* v, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_row_stride,
    float scale, void* out, int out_type, int64_t out_batch_stride, int64_t out_head_stride,
    int64_t out_row_stride, float* lse, int64_t lse_stride, double p, sputnik_hip_philox_state rng,
    int64_t* rng_state_out, const void* workspace, size_t workspace_bytes,
    sputnik_hip_stream_t stream) {
  return forward_dropout(
      heads_call(true, masks, nonzeros, m, n, d, batch, heads, row_indices, row_offsets, column_indices,
                 dtype, q, q_batch_stride, q_head_stride, q_row_stride, k, k_batch_stride, k_head_stride,
                 k_row_stride, v, v_batch_stride, v_head_stride, v_row_stride, scale, out, out_type,
                 out_batch_stride, out_head_stride, out_row_stride, lse, lse_stride, workspace,
                 workspace_bytes, /*planned=*/true, stream),
      p, rng, rng_state_out);
}

}  // extern "C"
