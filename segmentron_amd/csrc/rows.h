// The row geometry of the bandwidth-bound kernels, stated once: a thread keeps ONE channel vector
// for its whole life, a block holds cvb = 2^cvb_log2 vector lanes and THREADS / cvb pixel rows, and
// a reducing block sums its rows through LDS in row order into one fp32 partial row.  No atomics:
// the same inputs give the same bits.  The host queries that size the partial buffers and the
// launchers take cvb_log2, the chunk count and the grid from the functions below, so the two agree
// by construction.
//
// Which pixel a block row visits is the KERNEL's choice and decides which pixel lands in which
// partial row: the kernels of chan_gate.hip and pool.hip walk STRIDED chunks (q = chunk * spb +
// row, q += chunks * spb), those of cgnet.hip, espnetv2.hip and fpenet.hip a CONTIGUOUS range of
// rows_per() pixels per chunk.  Both keep their walk; only the geometry around it is shared.
#pragma once
#include "common.h"

namespace seg {

constexpr int ROWS_THREADS = 256;

// Lanes per block row by UTILISATION: the power of two in [2^min_log2, 32] that wastes the fewest
// lanes, the widest among equals (a whole wave on contiguous channels where CV allows it).
//   min_log2 = 0: chan_gate.hip, cgnet.hip, espnetv2.hip, fpenet.hip (stages, meu_bwd_high)
//   min_log2 = 3: pool.hip (adaptive average), dwconv.hip (strip), bn.hip (row tiles <= 32 lanes)
static inline int rows_pick_cvb_log2(int CV, int min_log2) {
  int best = 5;
  double bu = 0;
  for (int l = 5; l >= min_log2; --l) {
    const int b = 1 << l;
    const double u = (double)CV / (double)(((CV + b - 1) / b) * b);
    if (u > bu + 1e-9) { bu = u; best = l; }
  }
  return best;
}

// Lanes per block row by FIT: the smallest power of two that holds CV, 2^max_log2 at the most.
//   max_log2 = 5:  unet.hip (skip_pool_bwd: more channel blocks beyond 32 lanes)
//   max_log2 = 30: fpenet.hip (the MEU low kernels keep ALL of a pixel's channels in one block row)
static inline int rows_fit_cvb_log2(int CV, int max_log2) {
  int l = 0;
  while ((1 << l) < CV && l < max_log2) ++l;
  return l;
}

// Pixel chunks per image: about target_blocks blocks over N images of gx channel blocks, at least
// min_pixels pixels per chunk, 1 .. max_chunks
static inline int rows_chunks(int N, long gx, long HW, long min_pixels, long target_blocks,
                              int max_chunks) {
  long c = (target_blocks + (long)N * gx - 1) / ((long)N * gx);
  const long cap = (HW + min_pixels - 1) / min_pixels;
  if (c > cap) c = cap;
  if (c > max_chunks) c = max_chunks;
  if (c < 1) c = 1;
  return (int)c;
}

// channel blocks of a launch
static inline int rows_gx(int CV, int cvb_log2) { return (CV + (1 << cvb_log2) - 1) >> cvb_log2; }

// pixels of one contiguous chunk: HW / chunks rounded up to whole block rows
static inline long rows_per(long HW, int chunks, int cvb_log2) {
  const long spb = ROWS_THREADS >> cvb_log2;
  const long per = (HW + chunks - 1) / chunks;
  return (per + spb - 1) / spb * spb;
}

// grid (channel-vector blocks, pixel chunks, images)
static inline dim3 rows_grid(int CV, int cvb_log2, int chunks, int N) {
  return dim3(rows_gx(CV, cvb_log2), chunks, N);
}

// ceil(total / threads) clamped to [1, cap]: the grid of a grid-stride kernel
static inline int grid_1d(long total, int threads, long cap) {
  long g = (total + threads - 1) / threads;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// Sum the K accumulator vectors of the block's rows in row order -> out[k * kstride + c] for the
// channels c < C of channel block `cblk`.  smem: K * THREADS * V floats, laid out
// [K][rows][cvb * V]; ends with a barrier, so it can be called again on the same smem.
template <int V, int K, int THREADS = ROWS_THREADS>
__device__ __forceinline__ void rows_block_reduce(float* smem, const float (&acc)[K][V],
                                                  int cvb_log2, int cblk, int C, float* out,
                                                  long kstride) {
  const int tid = threadIdx.x;
  const int cvb = 1 << cvb_log2, spb = THREADS >> cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> cvb_log2;
  const int Wd = cvb * V;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float* mine = smem + ((long)k * spb + sy) * Wd + cx * V;
#pragma unroll
    for (int e = 0; e < V; ++e) mine[e] = acc[k][e];
  }
  __syncthreads();
  for (int i = tid; i < K * Wd; i += THREADS) {
    const int k = i / Wd, e = i - k * Wd;
    float tot = 0.f;
    for (int rr = 0; rr < spb; ++rr) tot += smem[((long)k * spb + rr) * Wd + e];
    const int c = cblk * Wd + e;
    if (c < C) out[(long)k * kstride + c] = tot;
  }
  __syncthreads();
}

// The launcher contract the rows kernels share: dtype, 1 <= N <= 65535 (grid z), HW >= 1, C a
// positive multiple of c_multiple, every pitch a multiple of ld_multiple that holds need[i]
// (need null: C) channels, 1 <= chunks <= max_chunks, N * C below 2^31.
static inline int rows_require(const char* what, int dtype, int N, long HW, int C, int c_multiple,
                               int ld_multiple, const long* lds, const int* need, int nld,
                               int chunks, int max_chunks) {
  SEG_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "%s: bad dtype %d", what, dtype);
  SEG_REQUIRE(N >= 1 && N <= 65535 && HW >= 1 && C >= c_multiple && C % c_multiple == 0,
              "%s: bad shape N=%d HW=%ld C=%d (C a multiple of %d)", what, N, HW, C, c_multiple);
  for (int i = 0; i < nld; ++i)
    SEG_REQUIRE(lds[i] % ld_multiple == 0 && lds[i] >= (need != nullptr ? need[i] : C),
                "%s: row pitch %ld not a multiple of %d / < %d", what, lds[i], ld_multiple,
                need != nullptr ? need[i] : C);
  SEG_REQUIRE(chunks >= 1 && chunks <= max_chunks, "%s: chunks %d out of [1, %d]", what, chunks,
              max_chunks);
  SEG_REQUIRE((long)N * C < (1L << 31), "%s: too large", what);
  return 0;
}

}  // namespace seg
