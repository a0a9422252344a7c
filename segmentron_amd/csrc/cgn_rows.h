// What the kernels of csrc/cgnet.hip, csrc/espnetv2.hip and csrc/fpenet.hip share beyond the row
// geometry of rows.h (contiguous pixel chunks, at most CGN_MAX_CHUNKS per image): guarded
// per-channel parameter loads and the zero-padded tap of their depthwise passes.
#pragma once
#include "rows.h"

namespace seg {

constexpr int CGN_THREADS = ROWS_THREADS;
constexpr int CGN_MAX_CHUNKS = 256;
constexpr int CGN_JV = 4;  // channels per thread of the joint kernel (16 B of fp32, 8 B of bf16)

// `n` per-channel parameters from p[base + c0 ..]: 16-byte loads where the vector lies below C
// and is aligned, guarded element loads otherwise (never past p[base + C - 1]); `fill` beyond C
// and for a null table
template <int N>
__device__ __forceinline__ void cgn_params(const float* __restrict__ p, long base, int c0, int C,
                                           float fill, float* out) {
#pragma unroll
  for (int e = 0; e < N; ++e) out[e] = fill;
  if (p == nullptr) return;
  const float* q = p + base + c0;
  if (c0 + N <= C && (reinterpret_cast<uintptr_t>(q) & 15) == 0) {
    load_params<N>(q, 0, out);
    return;
  }
#pragma unroll
  for (int e = 0; e < N; ++e)
    if (c0 + e < C) out[e] = q[e];
}

// the channel vector at (hh, ww) of image `img`, zeros outside the image
template <typename T>
__device__ __forceinline__ void cgn_tap(const T* __restrict__ img, long ld, int H, int W, int hh,
                                        int ww, float* f) {
  const bool in = (unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W;
  const long p = in ? (long)hh * W + ww : 0;  // (always a valid address; masked below)
  HVec<T>::load(img + p * ld, f);
#pragma unroll
  for (int e = 0; e < CGN_JV; ++e) f[e] = in ? f[e] : 0.f;
}

static inline int cgn_round8(int C) { return (C + 7) / 8 * 8; }

}  // namespace seg

