// PointRend point head (segmentron/models/pointrend.py:32-195): point sampling, its deterministic
// backward, the uncertainty measures, a device top-k, point coordinates, the scatter back into
// the logits, the resizes of the subdivision loop and the point-level cross-entropy.
//
// Maps are addressed through strides: element (n, pixel p = h*W + w, channel c) lives at
// base + n*sn + p*sp + c*sc, so one kernel reads the NHWC activations of the network
// (sn = H*W*ld, sp = ld, sc = 1) and the NCHW float32 maps of the subdivision loop
// (sn = C*H*W, sp = 1, sc = H*W).  Points are fp32 [N][P][2] in (width, height) order, in [0, 1].
// Point rows (the sampled features, the MLP logits) are [N*P][ld] in `dtype`.
//
// The source coordinate of a point follows ATen's grid_sample (align_corners=False,
// padding_mode='zeros'): g = 2p - 1, then ((g + 1) * W - 1) / 2, each step rounded to fp32
// (csrc is built with -ffp-contract=off).  No float atomics anywhere: the sampling backward
// buckets points by the cell of their top-left tap and lets every pixel gather its points in a
// fixed order, the top-k is an integer radix select, the loss reduction a fixed tree.
#include "common.h"

namespace seg {

constexpr int PR_THREADS = 256;

__device__ __forceinline__ float pr_load(const void* x, int dtype, long off) {
  return dtype == DT_BF16 ? bf16_to_f32(((const bf16_t*)x)[off]) : ((const float*)x)[off];
}
__device__ __forceinline__ void pr_put(void* y, int dtype, long off, float v) {
  if (dtype == DT_BF16)
    ((bf16_t*)y)[off] = f32_to_bf16(v);
  else
    ((float*)y)[off] = v;
}

// ATen grid_sampler_compute_source_index, align_corners=False, zeros padding (no clipping)
__device__ __forceinline__ float pr_source(float p, int size) {
  const float g = 2.0f * p - 1.0f;
  return ((g + 1.f) * (float)size - 1.f) / 2.f;
}

struct Taps {  // the four bilinear taps of one point: nw, ne, sw, se
  int x0, y0;  // nw tap (-1 .. W-1 / H-1: the taps outside the map are skipped)
  float w[4];
  bool valid;  // false: no tap can be inside the map (also NaN / huge coordinates)
};

__device__ __forceinline__ Taps pr_taps(float px, float py, int H, int W) {
  Taps t;
  const float ix = pr_source(px, W), iy = pr_source(py, H);
  t.x0 = t.y0 = 0;
  t.w[0] = t.w[1] = t.w[2] = t.w[3] = 0.f;
  t.valid = ix > -2.f && ix < (float)W && iy > -2.f && iy < (float)H;
  if (!t.valid) return t;
  const float fx = floorf(ix), fy = floorf(iy);
  t.x0 = (int)fx;
  t.y0 = (int)fy;
  const float x1 = fx + 1.f, y1 = fy + 1.f;
  t.w[0] = (x1 - ix) * (y1 - iy);  // nw
  t.w[1] = (ix - fx) * (y1 - iy);  // ne
  t.w[2] = (x1 - ix) * (iy - fy);  // sw
  t.w[3] = (ix - fx) * (iy - fy);  // se
  t.valid = t.x0 >= -1 && t.x0 <= W - 1 && t.y0 >= -1 && t.y0 <= H - 1;
  return t;
}

__device__ __forceinline__ bool pr_in(int y, int x, int H, int W) {
  return y >= 0 && y < H && x >= 0 && x < W;
}

// ---------------------------------------------------------------- sampling (forward)
// one thread per (point row, channel)
__global__ void __launch_bounds__(PR_THREADS)
point_sample_kernel(int dtype_x, const void* __restrict__ x, long sn, long sp, long sc, int N,
                    int H, int W, int C, const float* __restrict__ pts, int P, int nearest,
                    int dtype_y, void* __restrict__ y, long ldy, int col) {
  const long i = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (i >= (long)N * P * C) return;
  const int c = (int)(i % C);
  const long row = i / C;
  const long n = row / P;
  const float px = pts[2 * row], py = pts[2 * row + 1];
  const long base = n * sn + (long)c * sc;
  float v = 0.f;
  if (nearest) {  // ATen: std::nearbyint (half to even)
    const float rx = rintf(pr_source(px, W)), ry = rintf(pr_source(py, H));
    if (rx >= 0.f && rx < (float)W && ry >= 0.f && ry < (float)H)
      v = pr_load(x, dtype_x, base + ((long)ry * W + (long)rx) * sp);
  } else {
    const Taps t = pr_taps(px, py, H, W);
    if (t.valid) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int yy = t.y0 + (k >> 1), xx = t.x0 + (k & 1);
        if (pr_in(yy, xx, H, W))
          v = v + pr_load(x, dtype_x, base + ((long)yy * W + xx) * sp) * t.w[k];
      }
    }
  }
  pr_put(y, dtype_y, row * ldy + col + c, v);
}

// ---------------------------------------------------------------- sampling (backward)
// workspace (ints): off[N*cells + 1] | cursor[N*cells] | cell_of[N*P] | list[N*P],
// cells = (H+1)*(W+1): cell (y0+1, x0+1) holds the points whose nw tap is (y0, x0)
__global__ void pr_zero_ints(int* p, long n) {
  const long i = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (i < n) p[i] = 0;
}

__global__ void __launch_bounds__(PR_THREADS)
pr_bucket_count(const float* __restrict__ pts, int N, int P, int H, int W, int* cnt,
                int* cell_of) {
  const long r = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (r >= (long)N * P) return;
  const long n = r / P;
  const Taps t = pr_taps(pts[2 * r], pts[2 * r + 1], H, W);
  int cell = -1;
  if (t.valid) {
    cell = (t.y0 + 1) * (W + 1) + (t.x0 + 1);
    atomicAdd(&cnt[n * (H + 1) * (W + 1) + cell], 1);  // integer: the count is order-free
  }
  cell_of[r] = cell;
}

// exclusive scan of off[0..total) in place, off[total] = sum, cursor = copy: one block
__global__ void __launch_bounds__(1024) pr_scan(int* off, int* cursor, long total) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const long chunk = (total + 1023) / 1024;
  const long b = (long)t * chunk, e = min(total, b + chunk);
  int s = 0;
  for (long i = b; i < e; ++i) s += off[i];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;
  for (long i = b; i < e; ++i) {
    const int v = off[i];
    off[i] = run;
    cursor[i] = run;
    run += v;
  }
  if (t == 1023) off[total] = part[1023];
}

__global__ void __launch_bounds__(PR_THREADS)
pr_bucket_fill(int N, int P, int H, int W, const int* __restrict__ cell_of, int* cursor,
               int* list) {
  const long r = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (r >= (long)N * P) return;
  const int cell = cell_of[r];
  if (cell < 0) return;
  const long n = r / P;
  const int slot = atomicAdd(&cursor[n * (H + 1) * (W + 1) + cell], 1);
  list[slot] = (int)r;
}

// the fill order inside a cell depends on scheduling: sort each cell's points by index
__global__ void __launch_bounds__(PR_THREADS)
pr_bucket_sort(const int* __restrict__ off, long total, int* list) {
  const long c = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (c >= total) return;
  const int b = off[c], e = off[c + 1];
  for (int i = b + 1; i < e; ++i) {
    const int v = list[i];
    int j = i - 1;
    while (j >= b && list[j] > v) {
      list[j + 1] = list[j];
      --j;
    }
    list[j + 1] = v;
  }
}

// one thread per (pixel, channel): dx = sum over the points of the 4 cells whose taps include
// the pixel, cells in a fixed order, points in index order
__global__ void __launch_bounds__(PR_THREADS)
pr_sample_bwd_gather(int dtype_g, const void* __restrict__ g, long ldg, int col,
                     const float* __restrict__ pts, int N, int H, int W, int C,
                     const int* __restrict__ off, const int* __restrict__ list, int dtype_x,
                     void* __restrict__ dx, long lddx) {
  const long i = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (i >= (long)N * H * W * C) return;
  const int c = (int)(i % C);
  const long pix = i / C;
  const int w = (int)(pix % W);
  const int h = (int)((pix / W) % H);
  const long n = pix / ((long)H * W);
  const long cbase = n * (H + 1) * (W + 1);
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // cell (h + k/2, w + k%2) holds the points whose nw tap is (h + k/2 - 1, w + k%2 - 1): this
    // pixel is their tap 3 - k (se, sw, ne, nw)
    const long cell = cbase + (long)(h + (k >> 1)) * (W + 1) + (w + (k & 1));
    const int b = off[cell], e = off[cell + 1];
    for (int j = b; j < e; ++j) {
      const int r = list[j];
      const Taps t = pr_taps(pts[2 * (long)r], pts[2 * (long)r + 1], H, W);
      acc = acc + pr_load(g, dtype_g, (long)r * ldg + col + c) * t.w[3 - k];
    }
  }
  pr_put(dx, dtype_x, pix * lddx + c, acc);
}

// ---------------------------------------------------------------- uncertainty
// the two largest of the C channels (torch.sort(descending)[0], [1])
__device__ __forceinline__ void pr_top2(const void* x, int dtype, long base, long sc, int C,
                                        float& t1, float& t2) {
  t1 = pr_load(x, dtype, base);
  t2 = -INFINITY;
  for (int c = 1; c < C; ++c) {
    const float v = pr_load(x, dtype, base + (long)c * sc);
    if (v > t1) {
      t2 = t1;
      t1 = v;
    } else if (v > t2) {
      t2 = v;
    }
  }
}

// grid: u[n][p] = -(top1 - top2) over the C channels of pixel p
__global__ void __launch_bounds__(PR_THREADS)
pr_uncertainty_grid(int dtype, const void* __restrict__ x, long sn, long sp, long sc, int N,
                    long HW, int C, float* __restrict__ u) {
  const long i = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (i >= (long)N * HW) return;
  const long n = i / HW, p = i % HW;
  float t1, t2;
  pr_top2(x, dtype, n * sn + p * sp, sc, C, t1, t2);
  u[i] = -(t1 - t2);
}

// at points: the rank-0 and rank-1 planes of the channel-sorted map, each interpolated (zeros
// padding), then -(s0 - s1)  (pointrend.py:162,184-186)
__global__ void __launch_bounds__(PR_THREADS)
pr_uncertainty_points(int dtype, const void* __restrict__ x, long sn, long sp, long sc, int N,
                      int H, int W, int C, const float* __restrict__ pts, int P,
                      float* __restrict__ u) {
  const long r = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (r >= (long)N * P) return;
  const long n = r / P;
  const Taps t = pr_taps(pts[2 * r], pts[2 * r + 1], H, W);
  float s0 = 0.f, s1 = 0.f;
  if (t.valid) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int yy = t.y0 + (k >> 1), xx = t.x0 + (k & 1);
      if (!pr_in(yy, xx, H, W)) continue;
      float t1, t2;
      pr_top2(x, dtype, n * sn + ((long)yy * W + xx) * sp, sc, C, t1, t2);
      s0 = s0 + t1 * t.w[k];
      s1 = s1 + t2 * t.w[k];
    }
  }
  u[r] = -(s0 - s1);
}

// ---------------------------------------------------------------- top-k (radix select)
// order-preserving uint32 image of an fp32 key (-0 and +0 are one key, as they compare equal)
__device__ __forceinline__ uint32_t pr_key(float f) {
  const uint32_t v = f == 0.f ? 0u : __float_as_uint(f);
  return (v & 0x80000000u) ? ~v : (v | 0x80000000u);
}

constexpr int TK_CHUNK = 4096;  // keys per block of the histogram / count / write passes

// state[n] = {prefix, mask, remaining k, unused}; hist[n][256]
__global__ void pr_topk_init(int K, uint32_t* state, int* hist) {
  const int n = blockIdx.x, t = threadIdx.x;
  hist[n * 256 + t] = 0;
  if (t == 0) {
    state[4 * n] = 0u;
    state[4 * n + 1] = 0u;
    state[4 * n + 2] = (uint32_t)K;
    state[4 * n + 3] = 0u;
  }
}

__global__ void __launch_bounds__(256)
pr_topk_hist(const float* __restrict__ keys, long L, int shift, const uint32_t* __restrict__ state,
             int* hist) {
  __shared__ int h[256];
  const int n = blockIdx.y, t = threadIdx.x;
  h[t] = 0;
  __syncthreads();
  const uint32_t prefix = state[4 * n], mask = state[4 * n + 1];
  const long b = (long)blockIdx.x * TK_CHUNK, e = min(L, b + TK_CHUNK);
  const float* kn = keys + (long)n * L;
  for (long i = b + t; i < e; i += 256) {
    const uint32_t k = pr_key(kn[i]);
    if ((k & mask) == prefix) atomicAdd(&h[(k >> shift) & 255u], 1);
  }
  __syncthreads();
  if (h[t]) atomicAdd(&hist[n * 256 + t], h[t]);
}

// one block per image: the digit bucket that holds the k-th largest key; re-zeroes the histogram
__global__ void pr_topk_pick(int shift, uint32_t* state, int* hist) {
  __shared__ int h[256];
  const int n = blockIdx.x, t = threadIdx.x;
  h[t] = hist[n * 256 + t];
  hist[n * 256 + t] = 0;
  __syncthreads();
  if (t == 0) {
    int kr = (int)state[4 * n + 2];
    int d = 255;
    for (; d > 0; --d) {
      if (kr <= h[d]) break;
      kr -= h[d];
    }
    state[4 * n] |= (uint32_t)d << shift;
    state[4 * n + 1] |= 255u << shift;
    state[4 * n + 2] = (uint32_t)kr;
  }
}

__device__ __forceinline__ int pr_block_count(int v, int* red) {  // 256 threads = 4 waves
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int t = threadIdx.x;
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// cnt[n][block] = (#keys > T, #keys == T) of the block's chunk; T = the k-th largest key
__global__ void __launch_bounds__(256)
pr_topk_count(const float* __restrict__ keys, long L, const uint32_t* __restrict__ state,
              int* cnt) {
  __shared__ int red[4];
  const int n = blockIdx.y, t = threadIdx.x;
  const uint32_t T = state[4 * n];
  const long b = (long)blockIdx.x * TK_CHUNK, e = min(L, b + TK_CHUNK);
  const float* kn = keys + (long)n * L;
  int gt = 0, eq = 0;
  for (long i = b + t; i < e; i += 256) {
    const uint32_t k = pr_key(kn[i]);
    gt += k > T;
    eq += k == T;
  }
  gt = pr_block_count(gt, red);
  eq = pr_block_count(eq, red);
  if (t == 0) {
    cnt[2 * ((long)n * gridDim.x + blockIdx.x)] = gt;
    cnt[2 * ((long)n * gridDim.x + blockIdx.x) + 1] = eq;
  }
}

// selected: key > T, or key == T among the first `remaining k` such keys in index order.
// Output position = #(key > T before i) + #(key == T before i): ascending indices.
__global__ void __launch_bounds__(256)
pr_topk_write(const float* __restrict__ keys, long L, int K, const uint32_t* __restrict__ state,
              const int* __restrict__ cnt, long* __restrict__ idx) {
  __shared__ int base[2];
  __shared__ int wgt[4], weq[4];
  const int n = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t T = state[4 * n];
  const int keq = (int)state[4 * n + 2];
  if (t < 2) {
    int s = 0;
    for (int j = 0; j < (int)blockIdx.x; ++j) s += cnt[2 * ((long)n * gridDim.x + j) + t];
    base[t] = s;
  }
  __syncthreads();
  int run_gt = base[0], run_eq = base[1];
  const long b = (long)blockIdx.x * TK_CHUNK, e = min(L, b + TK_CHUNK);
  const float* kn = keys + (long)n * L;
  long* out = idx + (long)n * K;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (long i0 = b; i0 < e; i0 += 256) {  // block-uniform trip count
    const long i = i0 + t;
    const uint32_t k = i < e ? pr_key(kn[i]) : 0u;
    const bool g = i < e && k > T, q = i < e && k == T;
    const unsigned long long mg = __ballot(g), mq = __ballot(q);
    __syncthreads();
    if (lane == 0) {
      wgt[wv] = __popcll(mg);
      weq[wv] = __popcll(mq);
    }
    __syncthreads();
    int bg = run_gt, bq = run_eq;
    for (int j = 0; j < wv; ++j) {
      bg += wgt[j];
      bq += weq[j];
    }
    bg += __popcll(mg & below);
    bq += __popcll(mq & below);
    if (g || (q && bq < keq)) {
      const int pos = bg + min(bq, keq);
      if (pos < K) out[pos] = i;
    }
    run_gt += wgt[0] + wgt[1] + wgt[2] + wgt[3];
    run_eq += weq[0] + weq[1] + weq[2] + weq[3];
  }
}

// ---------------------------------------------------------------- coordinates, scatter
// train: importance points over[n][idx[n][j]] (j < K), then the coverage draws
__global__ void __launch_bounds__(PR_THREADS)
pr_coords_train(const float* __restrict__ over, const long* __restrict__ idx, int N, int L, int K,
                const float* __restrict__ cover, int P, float* __restrict__ pts) {
  const long i = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (i >= (long)N * P) return;
  const long n = i / P;
  const int j = (int)(i % P);
  const float* src;
  if (j < K) {
    const long s = idx[n * K + j];
    src = over + 2 * (n * L + s);
  } else {
    src = cover + 2 * (n * (P - K) + (j - K));
  }
  pts[2 * i] = src[0];
  pts[2 * i + 1] = src[1];
}

// eval: pixel centres as pointrend.py:170-172 computes them in fp32: W_step / 2 + (idx % W) * W_step
__global__ void __launch_bounds__(PR_THREADS)
pr_coords_grid(const long* __restrict__ idx, int N, int K, int H, int W, float* __restrict__ pts) {
  const long i = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (i >= (long)N * K) return;
  const long s = idx[i];
  const float ws = (float)(1.0 / W), hs = (float)(1.0 / H);
  const float ws2 = (float)(1.0 / W / 2.0), hs2 = (float)(1.0 / H / 2.0);
  pts[2 * i] = ws2 + (float)(s % W) * ws;
  pts[2 * i + 1] = hs2 + (float)(s / W) * hs;
}

__global__ void __launch_bounds__(PR_THREADS)
pr_scatter(int dtype_r, const void* __restrict__ rend, long ldr, const long* __restrict__ idx,
           int N, int P, int C, float* __restrict__ y, long sn, long sp, long sc) {
  const long i = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (i >= (long)N * P * C) return;
  const int c = (int)(i % C);
  const long row = i / C;
  const long n = row / P;
  y[n * sn + idx[row] * sp + (long)c * sc] = pr_load(rend, dtype_r, row * ldr + c);
}

// ---------------------------------------------------------------- bilinear resize
// ATen upsample_bilinear2d (area_pixel_compute_source_index) of a strided map of `dtype` into a
// float32 NCHW [N][C][Ho][Wo] map
__device__ __forceinline__ void pr_src(int dst, float scale, int in, int align, int& i0, int& i1,
                                       float& l0, float& l1) {
  float s = align ? scale * (float)dst : scale * ((float)dst + 0.5f) - 0.5f;
  if (!align && s < 0.f) s = 0.f;
  i0 = min((int)s, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}

__global__ void __launch_bounds__(PR_THREADS)
pr_resize(int dtype, const void* __restrict__ x, long sn, long sp, long sc, int N, int Hi, int Wi,
          int C, float* __restrict__ y, int Ho, int Wo, float rh, float rw, int align) {
  const long i = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (i >= (long)N * C * Ho * Wo) return;
  const int wo = (int)(i % Wo);
  const int ho = (int)((i / Wo) % Ho);
  const long nc = i / ((long)Ho * Wo);
  const int c = (int)(nc % C);
  const long n = nc / C;
  int h0, h1, w0, w1;
  float a0, a1, b0, b1;
  pr_src(ho, rh, Hi, align, h0, h1, a0, a1);
  pr_src(wo, rw, Wi, align, w0, w1, b0, b1);
  const long base = n * sn + (long)c * sc;
  const float x00 = pr_load(x, dtype, base + ((long)h0 * Wi + w0) * sp);
  const float x01 = pr_load(x, dtype, base + ((long)h0 * Wi + w1) * sp);
  const float x10 = pr_load(x, dtype, base + ((long)h1 * Wi + w0) * sp);
  const float x11 = pr_load(x, dtype, base + ((long)h1 * Wi + w1) * sp);
  y[i] = a0 * (b0 * x00 + b1 * x01) + a1 * (b0 * x10 + b1 * x11);
}

// ---------------------------------------------------------------- point cross-entropy
__device__ __forceinline__ void pr_row_lse(const void* x, int dtype, long off, int C, float& mx,
                                           float& lse) {
  mx = -INFINITY;
  for (int c = 0; c < C; ++c) mx = fmaxf(mx, pr_load(x, dtype, off + c));
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += expf(pr_load(x, dtype, off + c) - mx);
  lse = logf(s);
}

__device__ __forceinline__ double pr_block_sum_d(double v, double* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int o = PR_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ bool pr_valid(long tg, long ignore, int C) {
  return tg != ignore && tg >= 0 && tg < C;
}

// ws[2*block] = (sum of -log p[target], valid rows) of the block's 256 rows
__global__ void __launch_bounds__(PR_THREADS)
pr_ce_partial(int dtype, const void* __restrict__ x, long ldx, long R, int C,
              const long* __restrict__ target, long ignore, double* __restrict__ ws) {
  __shared__ double red[PR_THREADS];
  const long r = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  double l = 0.0, v = 0.0;
  if (r < R && pr_valid(target[r], ignore, C)) {
    float mx, lse;
    pr_row_lse(x, dtype, r * ldx, C, mx, lse);
    l = (double)(lse - (pr_load(x, dtype, r * ldx + target[r]) - mx));
    v = 1.0;
  }
  l = pr_block_sum_d(l, red);
  v = pr_block_sum_d(v, red);
  if (threadIdx.x == 0) {
    ws[2 * blockIdx.x] = l;
    ws[2 * blockIdx.x + 1] = v;
  }
}

__global__ void __launch_bounds__(PR_THREADS)
pr_ce_final(const double* __restrict__ ws, int blocks, float* __restrict__ loss_out) {
  __shared__ double red[PR_THREADS];
  double l = 0.0, v = 0.0;
  for (int b = threadIdx.x; b < blocks; b += PR_THREADS) {
    l += ws[2 * b];
    v += ws[2 * b + 1];
  }
  l = pr_block_sum_d(l, red);
  v = pr_block_sum_d(v, red);
  if (threadIdx.x == 0) {
    loss_out[0] = (float)(l / v);  // no valid row: 0/0 = NaN, as torch
    loss_out[1] = (float)(1.0 / v);
  }
}

__global__ void __launch_bounds__(PR_THREADS)
pr_ce_bwd(int dtype, const void* __restrict__ x, long ldx, long R, int C,
          const long* __restrict__ target, long ignore, const float* __restrict__ loss_out,
          const float* __restrict__ grad_out, void* __restrict__ dx, long lddx) {
  const long r = (long)blockIdx.x * PR_THREADS + threadIdx.x;
  if (r >= R) return;
  const long tg = target[r];
  if (pr_valid(tg, ignore, C)) {
    float mx, lse;
    pr_row_lse(x, dtype, r * ldx, C, mx, lse);
    const float s = grad_out[0] * loss_out[1];
    for (int c = 0; c < C; ++c) {
      const float p = expf(pr_load(x, dtype, r * ldx + c) - mx - lse);
      pr_put(dx, dtype, r * lddx + c, s * (p - (c == tg ? 1.f : 0.f)));
    }
  } else {
    for (int c = 0; c < C; ++c) pr_put(dx, dtype, r * lddx + c, 0.f);
  }
}

inline unsigned pr_grid(long n) { return (unsigned)((n + PR_THREADS - 1) / PR_THREADS); }

inline bool pr_dt(int d) { return d == DT_F32 || d == DT_BF16; }

inline long pr_bwd_ws_ints(int N, int H, int W, int P) {
  return 2 * (long)N * (H + 1) * (W + 1) + 1 + 2 * (long)N * P;
}

}  // namespace seg

using namespace seg;

extern "C" {

int seg_point_sample(int dtype_x, const void* x, long sn, long sp, long sc, int N, int H, int W,
                     int C, const float* pts, int P, int nearest, int dtype_y, void* y, long ldy,
                     int col, void* stream) {
  SEG_REQUIRE(x && pts && y && pr_dt(dtype_x) && pr_dt(dtype_y), "point_sample: bad arguments");
  SEG_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 1 && P >= 0 && col >= 0 && ldy >= col + C,
              "point_sample: bad geometry N=%d H=%d W=%d C=%d P=%d col=%d ldy=%ld", N, H, W, C, P,
              col, ldy);
  const long total = (long)N * P * C;
  if (total == 0) return 0;
  hipLaunchKernelGGL(point_sample_kernel, dim3(pr_grid(total)), dim3(PR_THREADS), 0,
                     (hipStream_t)stream, dtype_x, x, sn, sp, sc, N, H, W, C, pts, P, nearest,
                     dtype_y, y, ldy, col);
  return check_launch("point_sample");
}

int seg_point_sample_bwd_ws(int N, int H, int W, int P) {
  const long n = pr_bwd_ws_ints(N, H, W, P);
  return n < (1L << 31) ? (int)n : -1;
}

int seg_point_sample_bwd(int dtype_g, const void* g, long ldg, int col, const float* pts, int N,
                         int P, int H, int W, int C, int dtype_x, void* dx, long lddx, int* ws,
                         void* stream) {
  SEG_REQUIRE(g && pts && dx && ws && pr_dt(dtype_g) && pr_dt(dtype_x),
              "point_sample_bwd: bad arguments");
  SEG_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 1 && P >= 0 && lddx >= C && ldg >= col + C &&
                  pr_bwd_ws_ints(N, H, W, P) < (1L << 31),
              "point_sample_bwd: bad geometry N=%d H=%d W=%d C=%d P=%d", N, H, W, C, P);
  hipStream_t s = (hipStream_t)stream;
  const long cells = (long)N * (H + 1) * (W + 1);
  const long rows = (long)N * P;
  int* off = ws;
  int* cursor = off + cells + 1;
  int* cell_of = cursor + cells;
  int* list = cell_of + rows;
  hipLaunchKernelGGL(pr_zero_ints, dim3(pr_grid(cells + 1)), dim3(PR_THREADS), 0, s, off,
                     cells + 1);
  if (rows > 0)
    hipLaunchKernelGGL(pr_bucket_count, dim3(pr_grid(rows)), dim3(PR_THREADS), 0, s, pts, N, P, H,
                       W, off, cell_of);
  hipLaunchKernelGGL(pr_scan, dim3(1), dim3(1024), 0, s, off, cursor, cells);
  if (rows > 0) {
    hipLaunchKernelGGL(pr_bucket_fill, dim3(pr_grid(rows)), dim3(PR_THREADS), 0, s, N, P, H, W,
                       cell_of, cursor, list);
    hipLaunchKernelGGL(pr_bucket_sort, dim3(pr_grid(cells)), dim3(PR_THREADS), 0, s, off, cells,
                       list);
  }
  const long total = (long)N * H * W * C;
  hipLaunchKernelGGL(pr_sample_bwd_gather, dim3(pr_grid(total)), dim3(PR_THREADS), 0, s, dtype_g,
                     g, ldg, col, pts, N, H, W, C, off, list, dtype_x, dx, lddx);
  return check_launch("point_sample_bwd");
}

int seg_point_uncertainty(int dtype, const void* x, long sn, long sp, long sc, int N, int H, int W,
                          int C, const float* pts, int P, float* u, void* stream) {
  SEG_REQUIRE(x && u && pr_dt(dtype) && N >= 1 && H >= 1 && W >= 1 && C >= 2 && P >= 0,
              "point_uncertainty: bad arguments (C=%d must be >= 2)", C);
  if (pts == nullptr) {
    const long total = (long)N * H * W;
    hipLaunchKernelGGL(pr_uncertainty_grid, dim3(pr_grid(total)), dim3(PR_THREADS), 0,
                       (hipStream_t)stream, dtype, x, sn, sp, sc, N, (long)H * W, C, u);
  } else {
    const long total = (long)N * P;
    if (total == 0) return 0;
    hipLaunchKernelGGL(pr_uncertainty_points, dim3(pr_grid(total)), dim3(PR_THREADS), 0,
                       (hipStream_t)stream, dtype, x, sn, sp, sc, N, H, W, C, pts, P, u);
  }
  return check_launch("point_uncertainty");
}

int seg_point_topk_ws(int N, long L) {
  const long blocks = (L + TK_CHUNK - 1) / TK_CHUNK;
  return (int)(4L * N + 256L * N + 2L * N * blocks);  // 32-bit words
}

int seg_point_topk(const float* keys, int N, long L, int K, long* idx, int* ws, void* stream) {
  SEG_REQUIRE(keys && idx && ws && N >= 1 && L >= 1 && K >= 1 && K <= L && L < (1L << 30),
              "point_topk: bad arguments N=%d L=%ld K=%d", N, L, K);
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((L + TK_CHUNK - 1) / TK_CHUNK);
  uint32_t* state = (uint32_t*)ws;
  int* hist = ws + 4 * N;
  int* cnt = hist + 256 * N;
  hipLaunchKernelGGL(pr_topk_init, dim3(N), dim3(256), 0, s, K, state, hist);
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(pr_topk_hist, dim3(blocks, N), dim3(256), 0, s, keys, L, shift, state,
                       hist);
    hipLaunchKernelGGL(pr_topk_pick, dim3(N), dim3(256), 0, s, shift, state, hist);
  }
  hipLaunchKernelGGL(pr_topk_count, dim3(blocks, N), dim3(256), 0, s, keys, L, state, cnt);
  hipLaunchKernelGGL(pr_topk_write, dim3(blocks, N), dim3(256), 0, s, keys, L, K, state, cnt, idx);
  return check_launch("point_topk");
}

int seg_point_coords(const float* over, const long* idx, int N, int L, int K, const float* cover,
                     int P, int H, int W, float* pts, void* stream) {
  SEG_REQUIRE(idx && pts && N >= 1 && K >= 1, "point_coords: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  if (over != nullptr) {
    SEG_REQUIRE(P >= K && K <= L && (cover != nullptr || P == K),
                "point_coords: P=%d K=%d L=%d", P, K, L);
    hipLaunchKernelGGL(pr_coords_train, dim3(pr_grid((long)N * P)), dim3(PR_THREADS), 0, s, over,
                       idx, N, L, K, cover, P, pts);
  } else {
    SEG_REQUIRE(H >= 1 && W >= 1 && K <= (long)H * W, "point_coords: H=%d W=%d K=%d", H, W, K);
    hipLaunchKernelGGL(pr_coords_grid, dim3(pr_grid((long)N * K)), dim3(PR_THREADS), 0, s, idx, N,
                       K, H, W, pts);
  }
  return check_launch("point_coords");
}

int seg_point_scatter(int dtype_r, const void* rend, long ldr, const long* idx, int N, int P,
                      int C, float* y, long sn, long sp, long sc, void* stream) {
  SEG_REQUIRE(rend && idx && y && pr_dt(dtype_r) && N >= 1 && P >= 0 && C >= 1 && ldr >= C,
              "point_scatter: bad arguments");
  const long total = (long)N * P * C;
  if (total == 0) return 0;
  hipLaunchKernelGGL(pr_scatter, dim3(pr_grid(total)), dim3(PR_THREADS), 0, (hipStream_t)stream,
                     dtype_r, rend, ldr, idx, N, P, C, y, sn, sp, sc);
  return check_launch("point_scatter");
}

int seg_point_resize(int dtype, const void* x, long sn, long sp, long sc, int N, int Hi, int Wi,
                     int C, float* y, int Ho, int Wo, int align_corners, void* stream) {
  SEG_REQUIRE(x && y && pr_dt(dtype) && N >= 1 && Hi >= 1 && Wi >= 1 && C >= 1 && Ho >= 1 &&
                  Wo >= 1,
              "point_resize: bad arguments");
  float rh, rw;
  if (align_corners) {
    rh = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f;
    rw = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
  } else {
    rh = (float)Hi / (float)Ho;
    rw = (float)Wi / (float)Wo;
  }
  const long total = (long)N * C * Ho * Wo;
  hipLaunchKernelGGL(pr_resize, dim3(pr_grid(total)), dim3(PR_THREADS), 0, (hipStream_t)stream,
                     dtype, x, sn, sp, sc, N, Hi, Wi, C, y, Ho, Wo, rh, rw, align_corners);
  return check_launch("point_resize");
}

int seg_point_ce_blocks(long R) { return (int)((R + PR_THREADS - 1) / PR_THREADS); }

int seg_point_ce_fwd(int dtype, const void* x, long ldx, long R, int C, const long* target,
                     long ignore_index, double* ws, float* loss_out, void* stream) {
  SEG_REQUIRE(x && target && ws && loss_out && pr_dt(dtype) && R >= 1 && C >= 1 && ldx >= C,
              "point_ce_fwd: bad arguments");
  const int blocks = seg_point_ce_blocks(R);
  hipLaunchKernelGGL(pr_ce_partial, dim3(blocks), dim3(PR_THREADS), 0, (hipStream_t)stream, dtype,
                     x, ldx, R, C, target, ignore_index, ws);
  hipLaunchKernelGGL(pr_ce_final, dim3(1), dim3(PR_THREADS), 0, (hipStream_t)stream, ws, blocks,
                     loss_out);
  return check_launch("point_ce_fwd");
}

int seg_point_ce_bwd(int dtype, const void* x, long ldx, long R, int C, const long* target,
                     long ignore_index, const float* loss_out, const float* grad_out, void* dx,
                     long lddx, void* stream) {
  SEG_REQUIRE(x && target && loss_out && grad_out && dx && pr_dt(dtype) && R >= 1 && C >= 1 &&
                  ldx >= C && lddx >= C,
              "point_ce_bwd: bad arguments");
  hipLaunchKernelGGL(pr_ce_bwd, dim3(pr_grid(R)), dim3(PR_THREADS), 0, (hipStream_t)stream, dtype,
                     x, ldx, R, C, target, ignore_index, loss_out, grad_out, dx, lddx);
  return check_launch("point_ce_bwd");
}

}  // extern "C"
