// What the row-group attention kernels share (attention_backward.hip, attention_rows.hip;
// DESIGN.md 3.9c): a 16-lane row group owns one row of D floats, D / 16 of them per lane as
// D / 64 float4 vectors -- vector c of lane i holds columns 64 c + 4 i .. + 3, so that every
// load instruction of a group covers 256 contiguous bytes -- and walks its list of entries in
// windows of 16, one dropout decision per lane and window.
#pragma once

#include "common.h"
#include "philox.h"
#include "wave_utils.h"

namespace sputnik_hip {
namespace rowgroup {

constexpr int kGroup = 16;         // lanes per row group
constexpr int kThreads = 256;      // 16 row groups per workgroup
constexpr int kRowsPerBlock = kThreads / kGroup;

__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
  float s = a.x * b.x;
  s = fmaf(a.y, b.y, s);
  s = fmaf(a.z, b.z, s);
  return fmaf(a.w, b.w, s);
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float s) {
  s = fmaf(a.x, b.x, s);
  s = fmaf(a.y, b.y, s);
  s = fmaf(a.z, b.z, s);
  return fmaf(a.w, b.w, s);
}

__device__ __forceinline__ void fma4(float4& acc, float a, const float4& b) {
  acc.x = fmaf(a, b.x, acc.x);
  acc.y = fmaf(a, b.y, acc.y);
  acc.z = fmaf(a, b.z, acc.z);
  acc.w = fmaf(a, b.w, acc.w);
}

__device__ __forceinline__ float4 load4(const float* __restrict__ base, unsigned offset) {
  return *reinterpret_cast<const float4*>(base + offset);
}

// A lane's share of one row of D floats.
template <int D>
struct Frag {
  static_assert(D % 64 == 0, "a row group moves 64 columns per load instruction");
  static constexpr int kVectors = D / 64;
  float4 v[kVectors];
};

template <int D>
__device__ __forceinline__ Frag<D> zero_frag() {
  Frag<D> f;
#pragma unroll
  for (int c = 0; c < Frag<D>::kVectors; ++c) f.v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  return f;
}

// `offset` = row * D + 4 * (lane of the group), in elements (32-bit: supported()).
template <int D>
__device__ __forceinline__ Frag<D> load_frag(const float* __restrict__ base, unsigned offset) {
  Frag<D> f;
#pragma unroll
  for (int c = 0; c < Frag<D>::kVectors; ++c) f.v[c] = load4(base, offset + 64 * c);
  return f;
}

template <int D>
__device__ __forceinline__ void store_frag(float* __restrict__ base, unsigned offset, const Frag<D>& f) {
#pragma unroll
  for (int c = 0; c < Frag<D>::kVectors; ++c) *reinterpret_cast<float4*>(base + offset + 64 * c) = f.v[c];
}

template <int D>
__device__ __forceinline__ Frag<D> scaled(const Frag<D>& a, float s) {
  Frag<D> f;
#pragma unroll
  for (int c = 0; c < Frag<D>::kVectors; ++c)
    f.v[c] = make_float4(a.v[c].x * s, a.v[c].y * s, a.v[c].z * s, a.v[c].w * s);
  return f;
}

// The lane's part of <a, b>: one chain of fused multiply-adds, vector 0 first.
template <int D>
__device__ __forceinline__ float dot(const Frag<D>& a, const Frag<D>& b) {
  float s = dot4(a.v[0], b.v[0]);
#pragma unroll
  for (int c = 1; c < Frag<D>::kVectors; ++c) s = dot4(a.v[c], b.v[c], s);
  return s;
}

template <int D>
__device__ __forceinline__ void fma(Frag<D>& acc, float a, const Frag<D>& b) {
#pragma unroll
  for (int c = 0; c < Frag<D>::kVectors; ++c) fma4(acc.v[c], a, b.v[c]);
}

// Dropout decisions of the entries [w, end) of a row group's list, end - w <= 16, entry
// w + u in bit u: lane u makes the one Philox call for list position w + u (original entry
// entry_of(w + u)) and a ballot hands the decisions to the whole group -- one call per lane
// and window instead of one per lane and entry.  Every lane of the group takes part.
template <typename EntryOf>
__device__ __forceinline__ unsigned keep_window(const PhiloxKey& key, const DropArgs& drop, int r,
                                                int w, int end, EntryOf entry_of) {
  const int i = threadIdx.x % kGroup;
  const bool kept = w + i < end && philox_keep(key, drop.threshold, r, entry_of(w + i));
  const int base = (threadIdx.x % kWave) & ~(kGroup - 1);
  return static_cast<unsigned>(__ballot(kept) >> base) & 0xffffu;
}

__device__ __forceinline__ DropArgs drop_of() { return DropArgs{}; }
__device__ __forceinline__ DropArgs drop_of(const DropArgs& d) { return d; }

inline bool operand_ok(const float* p, int64_t stride) {
  return p == nullptr || (aligned_to(p, 16) && stride % 4 == 0 && stride >= 0);
}

// m rows of d floats are addressed with 32-bit element offsets scaled to bytes.
inline bool rows_fit_32_bits(int rows, int d) {
  return static_cast<int64_t>(rows) * d * 4 < (int64_t{1} << 32);
}

}  // namespace rowgroup
}  // namespace sputnik_hip
