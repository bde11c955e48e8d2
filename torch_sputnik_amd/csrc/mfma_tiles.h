// Shared pieces of the matrix-core kernels (sddmm_mfma.hip, spmm_mfma.hip): the
// 32 x 32 x 16 MFMA on float16 / bfloat16 fragments, tile geometry, the direct
// global->LDS copy.
#pragma once

#include "common.h"
#include "spmm_tiled_common.h"

namespace sputnik_hip {
namespace mfma_tiles {

using tiled::xcd_local_index32;
using f32x16 = float __attribute__((ext_vector_type(16)));

template <typename T>
struct Half8;
template <>
struct Half8<_Float16> {
  using type = _Float16 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ f32x16 mfma(type a, type b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Half8<__bf16> {
  using type = __bf16 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ f32x16 mfma(type a, type b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};

constexpr int kTile = 128;                       // rows and columns of an output tile
constexpr int kStep = 64;                        // k elements per step (128 bytes per row)
constexpr int kOperandBytes = kTile * kStep * 2; // 16 KiB: one operand's tile of a step
constexpr int kStageBytes = 2 * kOperandBytes;   // lhs tile, rhs tile
constexpr int kPitch = kTile + 4;                // floats per row of the epilogue's tile
constexpr int kTileBytes = kTile * kPitch * 4;   // 67 584
constexpr int kLdsBytes = kTileBytes + 4 * (kTile + 4);   // + the tile rows' CSR bounds
static_assert(kTileBytes >= 2 * kStageBytes, "the float tile reuses the stages");

constexpr float kLowPlaneScale = 2048.f;   // 2^11: the float16 split's low plane (see split_planes_kernel)

// The float16 split's range.  A float32 operand is scaled by 2^shift before it is split,
// shift = 14 - floor(log2(amax)) over its FINITE elements (0 when there are none), so that
// its largest magnitude lies in [2^14, 2^15); the tile kernel's epilogue multiplies by
// 2^-(shift_a + shift_b).  Both are exact (ldexp), so within the band where the unscaled
// split was already right the planes and the results keep their bits.  Every value keeps 22
// bits down to 2^-28 of the largest (the low plane leaves float16's subnormals there), the
// error stays below 2^-50 of the largest beneath that, over float32's whole range
// (subnormals included); without the shift only |v| in ~[1e-6, 65504) was covered.  The shift is found on the
// device by two launches -- range_kernel writes one maximum per block, the splitting kernel
// reduces them (every block the same way) -- and lives in a trailer behind the planes:
//   int shift, then (at byte 256) kRangeBlocks per-block maxima (bits of |v|).
// inf / NaN take no part in amax and come out of the split non-finite (inf - inf = NaN).
constexpr int kRangeBlocks = 512;
constexpr size_t kRangeBytes = 256 + 4 * kRangeBlocks;   // 2304: a multiple of 256
constexpr int kRangeTop = 14;                            // amax * 2^shift in [2^14, 2^15)

// shift from the bits of the largest finite |v| (the order of non-negative floats is that
// of their bits)
__device__ __forceinline__ int range_shift_of(unsigned amax_bits) {
  if (amax_bits == 0) return 0;
  const int e = static_cast<int>(amax_bits >> 23) - 127;   // (-127: a subnormal amax)
  return kRangeTop - e;
}

// The shift from range_kernel's maxima; every thread of a 256-thread block calls it.
__device__ __forceinline__ int range_shift(const unsigned* __restrict__ maxima) {
  __shared__ unsigned wave_max[4];
  unsigned v = max(maxima[threadIdx.x], maxima[threadIdx.x + 256]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, static_cast<unsigned>(__shfl_xor(static_cast<int>(v), o)));
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = v;
  __syncthreads();
  v = max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3]));
  return range_shift_of(v);
}
static_assert(kRangeBlocks == 512, "range_shift reads two maxima per thread of 256");

// ints of the plan's row_ok part (the table sits behind it)
__host__ __device__ inline int64_t plan_rows(int m) { return (static_cast<int64_t>(m) + 3) / 4 * 4; }

// A wave-uniform pointer that the compiler computed on the vector unit (an integer
// division ends there), back in scalar registers: the copies below take their base there.
template <typename T>
__device__ __forceinline__ const T* uniform_ptr(const T* p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
  return reinterpret_cast<const T*>((static_cast<uint64_t>(hi) << 32) | lo);
}

// direct global->LDS copy of 64 x 16 bytes: LDS destination M0 + lane * 16, per-lane source
__device__ __forceinline__ void copy_piece(const void* base /* wave-uniform */,
                                           unsigned lane_byte_offset, const char* lds_dst) {
  const unsigned lds_addr =
      static_cast<unsigned>(reinterpret_cast<uintptr_t>(AS_LDS(const_cast<char*>(lds_dst))));
  asm volatile(
      "s_mov_b32 m0, %0\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2"
      :
      : "s"(lds_addr), "v"(lane_byte_offset), "s"(base)
      : "memory", "m0");
}


}  // namespace mfma_tiles
}  // namespace sputnik_hip
