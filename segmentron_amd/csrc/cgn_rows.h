// The launch geometry the kernels of csrc/cgnet.hip and csrc/espnetv2.hip share: grid (channel-vector
// blocks, pixel chunks, images); a chunk is a contiguous pixel range of one image, a thread keeps one
// channel vector of one image for its whole life, and a block sums its rows through LDS in row order
// into one fp32 partial row per (chunk, image).
#pragma once
#include "common.h"

namespace seg {

constexpr int CGN_THREADS = 256;
constexpr int CGN_MAX_CHUNKS = 256;
constexpr int CGN_JV = 4;  // channels per thread of the joint kernel (16 B of fp32, 8 B of bf16)

// lanes (channel vectors) per block row: the power of two <= 32 that wastes the fewest lanes,
// the widest among equals
static inline int cgn_pick_cvb_log2(int CV) {
  int best = 5;
  double bu = 0;
  for (int l = 5; l >= 0; --l) {
    const int b = 1 << l;
    const double u = (double)CV / (double)(((CV + b - 1) / b) * b);
    if (u > bu + 1e-9) { bu = u; best = l; }
  }
  return best;
}

// pixels of one chunk: HW / chunks rounded up to whole block rows
static inline long cgn_per(long HW, int chunks, int cvb_log2) {
  const long spb = CGN_THREADS >> cvb_log2;
  const long per = (HW + chunks - 1) / chunks;
  return (per + spb - 1) / spb * spb;
}

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

// Sum the K accumulator vectors of the block's rows in row order -> out[k][c] for the block's
// channels c < C.  smem: [K][rows][cvb * V]; ends with a barrier, so it can be called again.
template <int V, int K>
__device__ __forceinline__ void cgn_block_reduce(float* smem, const float (&acc)[K][V],
                                                 int cvb_log2, int C, float* out, long kstride) {
  const int tid = threadIdx.x;
  const int cvb = 1 << cvb_log2, spb = CGN_THREADS >> cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> cvb_log2;
  const int Wd = cvb * V;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float* mine = smem + ((long)k * spb + sy) * Wd + cx * V;
#pragma unroll
    for (int e = 0; e < V; ++e) mine[e] = acc[k][e];
  }
  __syncthreads();
  for (int i = tid; i < K * Wd; i += CGN_THREADS) {
    const int k = i / Wd, e = i - k * Wd;
    float tot = 0.f;
    for (int rr = 0; rr < spb; ++rr) tot += smem[((long)k * spb + rr) * Wd + e];
    const int c = blockIdx.x * Wd + e;
    if (c < C) out[(long)k * kstride + c] = tot;
  }
  __syncthreads();
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

static inline dim3 cgn_grid(int CV, int cvb_log2, int chunks, int N) {
  const int cvb = 1 << cvb_log2;
  return dim3((CV + cvb - 1) / cvb, chunks, N);
}

}  // namespace seg

#define CGN_LAUNCH(kernel, a, chunks, stream)                                                 \
  do {                                                                                        \
    const dim3 grid = cgn_grid(a.CV, a.cvb_log2, chunks, a.N);                                \
    if (dtype == DT_BF16)                                                                     \
      hipLaunchKernelGGL((kernel<bf16_t>), grid, dim3(CGN_THREADS), 0, (hipStream_t)stream, a); \
    else                                                                                      \
      hipLaunchKernelGGL((kernel<float>), grid, dim3(CGN_THREADS), 0, (hipStream_t)stream, a);  \
  } while (0)
