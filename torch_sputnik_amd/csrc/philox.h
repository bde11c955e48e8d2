// Attention dropout's random numbers (sputnik_hip.h, "dropout"): the keep decision of entry e
// of replica r is a pure function of (seed, offset, r, e), so that every route -- the fused
// kernels, sparse_dropout on an [R, width] values array, the backward's replay -- drops the
// same entries.  Philox4x32-10 with
//   key     = (seed lo, seed hi)
//   counter = (offset/4 lo, offset/4 hi, e >> 2, r),  output word e & 3
// which is ATen's Philox4_32(seed, subsequence = (r << 32) | (e >> 2), offset) for an offset
// that is a multiple of 4.  Entry (r, e) is kept iff word < threshold, and a kept value is
// multiplied by `scale`; both come from the host (drop_args).
#pragma once

#include <math.h>

#include "common.h"

namespace sputnik_hip {

struct DropArgs {
  sputnik_hip_philox_state rng;
  int64_t* rng_state_out;   // {seed, offset} as resolved, written by the first lane; may be NULL
  unsigned threshold;
  float scale;
  int replica0;             // replica index of the launch's first replica (chunked launches)
};

// p in [0, 1) -> threshold min(floor((1 - p) 2^32), 2^32 - 1) and scale float(1 / (1 - p)),
// both computed in double.  False for any other p (NaN included).
inline bool drop_args(double p, const sputnik_hip_philox_state& rng, int64_t* rng_state_out,
                      DropArgs* out) {
  if (!(p >= 0.0 && p < 1.0)) return false;
  const double t = floor((1.0 - p) * 4294967296.0);
  out->rng = rng;
  out->rng_state_out = rng_state_out;
  out->threshold = t >= 4294967295.0 ? 0xffffffffu : static_cast<unsigned>(t);
  out->scale = static_cast<float>(1.0 / (1.0 - p));
  out->replica0 = 0;
  return true;
}

struct PhiloxKey {
  unsigned k0, k1, c0, c1;   // key, and the offset half of the counter
};

// Resolve the state (the captured-graph form reads seed and offset from device memory) and
// publish it: the lane that passes `writer` stores {seed, offset} into rng_state_out with a
// plain vector store.
__device__ __forceinline__ PhiloxKey philox_key(const DropArgs& d, bool writer) {
  const uint64_t seed = d.rng.seed_ptr != nullptr ? static_cast<uint64_t>(*d.rng.seed_ptr) : d.rng.seed;
  const uint64_t offset = d.rng.offset_ptr != nullptr
                              ? static_cast<uint64_t>(*d.rng.offset_ptr) + d.rng.offset_intragraph
                              : d.rng.offset;
  if (writer && d.rng_state_out != nullptr) {
    d.rng_state_out[0] = static_cast<int64_t>(seed);
    d.rng_state_out[1] = static_cast<int64_t>(offset);
  }
  const uint64_t c = offset / 4;
  return PhiloxKey{static_cast<unsigned>(seed), static_cast<unsigned>(seed >> 32),
                   static_cast<unsigned>(c), static_cast<unsigned>(c >> 32)};
}

// The four words of counter (key.c0, key.c1, c2, c3).
__device__ __forceinline__ uint4 philox4x32_10(const PhiloxKey& key, unsigned c2, unsigned c3) {
  unsigned c0 = key.c0, c1 = key.c1, k0 = key.k0, k1 = key.k1;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
    const unsigned lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}

__device__ __forceinline__ unsigned uint4_word(const uint4& w, int i) {
  return i == 0 ? w.x : i == 1 ? w.y : i == 2 ? w.z : w.w;
}

// Keep decision of entry e of replica r.
__device__ __forceinline__ bool philox_keep(const PhiloxKey& key, unsigned threshold, int r, int e) {
  const uint4 w = philox4x32_10(key, static_cast<unsigned>(e) >> 2, static_cast<unsigned>(r));
  return uint4_word(w, e & 3) < threshold;
}

// Launches one lane that publishes the resolved state (dropout.hip): for the calls that have
// no stored entry to run a kernel over.  No-op when drop.rng_state_out is NULL.
int publish_rng_state(const DropArgs& drop, hipStream_t stream);

}  // namespace sputnik_hip
