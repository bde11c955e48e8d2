// sparse_dropout: out[r, e] = x[r, e] * keep(r, e) * scale over a values array [rows, width]
// (philox.h for the decision).  A bandwidth kernel: one thread owns 16 bytes of a row (4
// float32 or 8 half entries), i.e. one or two Philox calls of four words each, and reads and
// writes them with one 16-byte access where the row is aligned.  The same kernel serves the
// composed attention's forward and both replays of the backward (the weights and their
// gradient), so it takes its state from device memory as readily as from values.
#include "philox.h"

namespace sputnik_hip {
namespace {

constexpr int kDropThreads = 256;

template <typename T>
__device__ __forceinline__ float to_f32(T x) { return static_cast<float>(x); }

template <typename T, int V>
struct alignas(16) Pack {
  T v[V];
};

// VEC: every row base is 16-byte aligned (the host checks bases and strides); the last
// partial group of a row is handled entry by entry.
template <typename T, bool VEC>
__global__ __launch_bounds__(kDropThreads) void sparse_dropout_kernel(
    int rows, int width, const T* __restrict__ x, int64_t x_stride, T* __restrict__ out,
    int64_t out_stride, DropArgs drop) {
  constexpr int V = 16 / sizeof(T);   // entries per thread: 4 or 8
  const bool writer = blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0;
  const PhiloxKey key = philox_key(drop, writer);
  const int e0 = (blockIdx.x * kDropThreads + threadIdx.x) * V;
  if (e0 >= width) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) {
    const T* __restrict__ xr = x + r * x_stride;
    T* __restrict__ outr = out + r * out_stride;
    const unsigned replica = static_cast<unsigned>(drop.replica0 + r);
    uint4 words[V / 4];
#pragma unroll
    for (int j = 0; j < V / 4; ++j) words[j] = philox4x32_10(key, static_cast<unsigned>(e0 / 4 + j), replica);
    auto one = [&](int j, T xv) -> T {
      const bool keep = uint4_word(words[j / 4], j & 3) < drop.threshold;
      return static_cast<T>(keep ? to_f32(xv) * drop.scale : 0.f);
    };
    if (VEC && e0 + V <= width) {
      Pack<T, V> in = *reinterpret_cast<const Pack<T, V>*>(xr + e0), res;
#pragma unroll
      for (int j = 0; j < V; ++j) res.v[j] = one(j, in.v[j]);
      *reinterpret_cast<Pack<T, V>*>(outr + e0) = res;
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (e0 + j < width) outr[e0 + j] = one(j, xr[e0 + j]);
    }
  }
}

// Publishes the resolved state of a call that has nothing to drop (no stored entry).
__global__ void rng_state_kernel(DropArgs drop) { philox_key(drop, threadIdx.x == 0); }

template <typename T>
int launch_dropout(int rows, int width, const void* x, int64_t x_stride, void* out,
                   int64_t out_stride, const DropArgs& drop, hipStream_t stream) {
  const bool vec = aligned_to(x, 16) && aligned_to(out, 16) &&
                   (x_stride * static_cast<int64_t>(sizeof(T))) % 16 == 0 &&
                   (out_stride * static_cast<int64_t>(sizeof(T))) % 16 == 0;
  constexpr int V = 16 / sizeof(T);
  const dim3 grid(ceil_div(ceil_div(width, V), kDropThreads), min(rows, kMaxGridYZ));
  if (vec)
    hipLaunchKernelGGL((sparse_dropout_kernel<T, true>), grid, dim3(kDropThreads), 0, stream, rows,
                       width, static_cast<const T*>(x), x_stride, static_cast<T*>(out), out_stride, drop);
  else
    hipLaunchKernelGGL((sparse_dropout_kernel<T, false>), grid, dim3(kDropThreads), 0, stream, rows,
                       width, static_cast<const T*>(x), x_stride, static_cast<T*>(out), out_stride, drop);
  return launch_status();
}

}  // namespace

int publish_rng_state(const DropArgs& drop, hipStream_t stream) {
  if (drop.rng_state_out == nullptr) return 0;
  hipLaunchKernelGGL(rng_state_kernel, dim3(1), dim3(64), 0, stream, drop);
  return launch_status();
}

}  // namespace sputnik_hip

using namespace sputnik_hip;

extern "C" int sputnik_hip_sparse_dropout_typed(int rows, int width, int replica0, int dtype,
                                                const void* x, int64_t x_stride, void* out,
                                                int64_t out_stride, double p,
                                                sputnik_hip_philox_state rng,
                                                int64_t* rng_state_out,
                                                sputnik_hip_stream_t stream_in) {
  const hipStream_t stream = static_cast<hipStream_t>(stream_in);
  DropArgs drop;
  if (rows < 0 || width < 0 || replica0 < 0 || x_stride < width || out_stride < width ||
      !drop_args(p, rng, rng_state_out, &drop))
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  if (dtype != SPUTNIK_HIP_F32 && dtype != SPUTNIK_HIP_F16 && dtype != SPUTNIK_HIP_BF16)
    return SPUTNIK_HIP_INVALID_ARGUMENT;
  drop.replica0 = replica0;
  if (p == 0.0) {   // nothing is dropped and no state is touched: a copy
    if (rows == 0 || width == 0) return 0;
    const size_t elem = dtype == SPUTNIK_HIP_F32 ? 4 : 2;
    const hipError_t e = hipMemcpy2DAsync(out, out_stride * elem, x, x_stride * elem, width * elem, rows,
                                          hipMemcpyDeviceToDevice, stream);
    return static_cast<int>(e);
  }
  if (rows == 0 || width == 0) return publish_rng_state(drop, stream);
  if (dtype == SPUTNIK_HIP_F32)
    return launch_dropout<float>(rows, width, x, x_stride, out, out_stride, drop, stream);
  if (dtype == SPUTNIK_HIP_F16)
    return launch_dropout<_Float16>(rows, width, x, x_stride, out, out_stride, drop, stream);
  return launch_dropout<__bf16>(rows, width, x, x_stride, out, out_stride, drop, stream);
}
