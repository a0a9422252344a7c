// Fused  bilinear upsample (align_corners) -> log-softmax -> NLL(ignore_index), forward and
// backward, on the LOW-resolution NHWC logits.  Replaces, for the train step of
// tools/train.py:135-146, the chain
//     F.interpolate(head(x), size, mode='bilinear', align_corners=True)    deeplabv3_plus.py:44
//     F.cross_entropy(pred, target, ignore_index=-1)                       solver/loss.py:16-46
// whose intermediate [N, nclass, H, W] float32 logits (319 MB at 2 x 19 x 1025 x 2049) are
// written once and read three times by five ATen kernels.  Here they are never
// materialised: the forward interpolates, soft-maxes and reduces per output pixel; the backward
// recomputes the soft-max once per output pixel and gathers the gradient into the low-resolution
// tensor in two separable passes — along w into an fp32 workspace [N, H, Wi, C] (80 MB for the
// tensor above), then along h.
//
// Numerics follow ATen: interpolation in float32 with the tap arithmetic of resize_taps.h and
// the same association  h0l*(w0l*x00 + w1l*x01) + h1l*(w0l*x10 + w1l*x11); log-softmax as
// z - max - log(sum exp(z - max)); loss = sum over valid pixels / number of valid pixels
// (reduction='mean').  Sums are taken in float64 in a fixed order: bitwise deterministic.
#include "common.h"
#include "resize_taps.h"

namespace seg {

constexpr int CE_THREADS = 256;

struct CeArgs {
  const void* lo;        // [N, Hi, Wi, ld] logits, element type T
  const long* target;    // [N, H, W] int64
  long ld;
  int N, Hi, Wi, H, W, C;
  long ignore;
  float sh, sw;
  int align;
};

// NC channels of one pixel; vectors beyond the row pitch (narrow class counts: the buffer is
// padded to a vector multiple of C, not to NC) are not touched
template <typename T, int NC>
__device__ __forceinline__ void ce_load_pixel(const T* __restrict__ p, long ld, float (&f)[NC]) {
  constexpr int VEC = Vec<T>::N;
#pragma unroll
  for (int v = 0; v < NC / VEC; ++v) {
    if (v * VEC < ld) {
      Vec<T>::unpack(ldg16(p + v * VEC), &f[v * VEC]);
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) f[v * VEC + k] = 0.f;
    }
  }
}

// z[c] of output pixel (n, h, w): NC >= C channels are loaded (the buffer is channel-padded)
template <typename T, int NC>
__device__ __forceinline__ void ce_logits(const CeArgs& a, int n, int h, int w, float (&z)[NC]) {
  const T* __restrict__ X = reinterpret_cast<const T*>(a.lo);
  int h0, h1, w0, w1; float lh, lw;
  taps(a.sh, h, a.Hi, a.align, h0, h1, lh);
  taps(a.sw, w, a.Wi, a.align, w0, w1, lw);
  const long base = (long)n * a.Hi * a.Wi;
  // the four taps stay PACKED until they are combined, one channel vector at a time: 4 * NC
  // unpacked floats alive at once (96 registers for 24 classes) cost the backward kernel its
  // occupancy; all loads are still issued before the first use
  constexpr int VEC = Vec<T>::N, NV = NC / VEC;
  const T* __restrict__ p00 = X + (base + (long)h0 * a.Wi + w0) * a.ld;
  const T* __restrict__ p01 = X + (base + (long)h0 * a.Wi + w1) * a.ld;
  const T* __restrict__ p10 = X + (base + (long)h1 * a.Wi + w0) * a.ld;
  const T* __restrict__ p11 = X + (base + (long)h1 * a.Wi + w1) * a.ld;
  const float h0l = 1.f - lh, w0l = 1.f - lw;
  // one vector ahead: the next vector's four loads are in flight while this one is combined
  uint4 q00 = ldg16(p00), q01 = ldg16(p01), q10 = ldg16(p10), q11 = ldg16(p11);
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const uint4 c00 = q00, c01 = q01, c10 = q10, c11 = q11;
    if (v + 1 < NV) {
      const int off = ((v + 1) * VEC < a.ld) ? (v + 1) * VEC : 0;  // beyond the pitch: masked below
      q00 = ldg16(p00 + off); q01 = ldg16(p01 + off);
      q10 = ldg16(p10 + off); q11 = ldg16(p11 + off);
    }
    const bool in = v * VEC < a.ld;
    if constexpr (sizeof(T) == 2) {
      // bf16: two channels per dword, combined pair by pair (8 temporaries instead of 32)
      const unsigned d00[4] = {c00.x, c00.y, c00.z, c00.w}, d01[4] = {c01.x, c01.y, c01.z, c01.w};
      const unsigned d10[4] = {c10.x, c10.y, c10.z, c10.w}, d11[4] = {c11.x, c11.y, c11.z, c11.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float a0 = __uint_as_float(d00[k] << 16), a1 = __uint_as_float(d00[k] & 0xFFFF0000u);
        const float b0 = __uint_as_float(d01[k] << 16), b1 = __uint_as_float(d01[k] & 0xFFFF0000u);
        const float e0 = __uint_as_float(d10[k] << 16), e1 = __uint_as_float(d10[k] & 0xFFFF0000u);
        const float g0 = __uint_as_float(d11[k] << 16), g1 = __uint_as_float(d11[k] & 0xFFFF0000u);
        const float t0 = h0l * (w0l * a0 + lw * b0) + lh * (w0l * e0 + lw * g0);
        const float t1 = h0l * (w0l * a1 + lw * b1) + lh * (w0l * e1 + lw * g1);
        z[v * VEC + 2 * k] = in ? t0 : 0.f;
        z[v * VEC + 2 * k + 1] = in ? t1 : 0.f;
      }
    } else {
      float f00[VEC], f01[VEC], f10[VEC], f11[VEC];
      Vec<T>::unpack(c00, f00); Vec<T>::unpack(c01, f01);
      Vec<T>::unpack(c10, f10); Vec<T>::unpack(c11, f11);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float t = h0l * (w0l * f00[k] + lw * f01[k]) + lh * (w0l * f10[k] + lw * f11[k]);
        z[v * VEC + k] = in ? t : 0.f;
      }
    }
  }
}

// forward: partial[block] = (sum of -log p_target over the block's valid pixels, valid count)
template <typename T, int NC>
__global__ __launch_bounds__(CE_THREADS) void ce_fwd_kernel(const CeArgs a, double* partial) {
  __shared__ double red[2][CE_THREADS / 64];
  const long total = (long)a.N * a.H * a.W;
  double lsum = 0.0, lcnt = 0.0;
  for (long i = (long)blockIdx.x * CE_THREADS + threadIdx.x; i < total;
       i += (long)gridDim.x * CE_THREADS) {
    const long t = a.target[i];
    // targets outside [0, C) that are not ignore_index (torch raises a device assert for them)
    // are left out of the sum AND the count, like ignored pixels — never counted with z_t = 0.
    // (No branch on the target: its load and the logit taps go out together.)
    const bool valid = !(t == a.ignore || t < 0 || t >= a.C);
    const int w = (int)(i % a.W);
    const long q = i / a.W;
    const int h = (int)(q % a.H), n = (int)(q / a.H);
    float z[NC];
    ce_logits<T, NC>(a, n, h, w, z);
    float m = z[0];
#pragma unroll
    for (int c = 1; c < NC; ++c) m = (c < a.C) ? fmaxf(m, z[c]) : m;
    float s = 0.f, zt = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < a.C) s += expf(z[c] - m);
      if (c == (int)t) zt = z[c];
    }
    if (valid) {
      lsum += (double)(logf(s) + m - zt);
      lcnt += 1.0;
    }
  }
  // block reduction in a fixed order (wave butterfly, then the waves in index order)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lsum += __shfl_xor(lsum, o, 64);
    lcnt += __shfl_xor(lcnt, o, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wave] = lsum; red[1][wave] = lcnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0, c = 0.0;
    for (int k = 0; k < CE_THREADS / 64; ++k) { s += red[0][k]; c += red[1][k]; }
    partial[2 * blockIdx.x] = s;
    partial[2 * blockIdx.x + 1] = c;
  }
}

// out[0] = loss (mean over valid pixels), out[1] = 1 / valid count (0 if none), both float32
__global__ void ce_finalize_kernel(const double* partial, int nblocks, float* out) {
  __shared__ double red[2][256];
  double s = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) { s += partial[2 * i]; c += partial[2 * i + 1]; }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double cnt = red[1][0];
    out[0] = cnt > 0.0 ? (float)(red[0][0] / cnt) : nanf("");  // torch: mean over nothing = nan
    out[1] = cnt > 0.0 ? (float)(1.0 / cnt) : 0.f;
  }
}

// backward: the gather  dlo[n][i][j][c] = sum_h wh(h -> i) * sum_w ww(w -> j) * dz[n][h][w][c]  is
// separable, so it runs as two passes with an fp32 workspace tmp[N][H][Wi][C] between them.
//   row pass     block = (image, output row h, segment of SJ low-resolution columns).  A thread owns
//                one output pixel of the segment's footprint: dz = g * (softmax - onehot) into LDS
//                as [c][w]; then (column j, class c) items reduce along w, ascending over
//                cand_range(j) with fmaf, and the segment's tmp[n][h][j0 ..][:] — one contiguous run
//                of the workspace — leaves through LDS as coalesced dword stores.  Only the few
//                halo pixels a segment shares with its neighbours are computed twice.
//   column pass  per (n, i, j, c): ascending over cand_range(i) with fmaf from 0, rounded once to
//                the storage type; channels >= C are written as zero up to the pitch.
// Every output pixel's softmax is computed once per segment that touches it (the tiled kernel this
// replaces computed it ~1.27 times at x4 and spent two thirds of its time in three barrier-separated
// phases per 12-row chunk).  The order of every sum is that of a whole-footprint gather, rows
// outside columns inside; zero-weight candidates are skipped (fmaf(0, finite, v) == v).  No atomics.
constexpr int CE_ROW_THREADS = 256;           // the most output pixels a segment's footprint may hold
constexpr int CE_ROW_PITCH = CE_ROW_THREADS + 1;  // dz row pitch: == 1 (mod 32 banks)
constexpr int CE_ROW_TPJ = 4;                 // threads that share one column j of the row reduction
constexpr int CE_ROW_MAX_SJ = 128;            // bounds the LDS of the store staging
constexpr float CE_MAX_SCALE = 16.1f;         // output-stride-4, -8 and -16 heads

template <typename T, int NC>
__global__ __launch_bounds__(CE_ROW_THREADS) void ce_bwd_row_kernel(const CeArgs a, const float* gscale,
                                                                    const float* gout,
                                                                    float* __restrict__ ws, int SJ) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_ce[];
  float* dz = reinterpret_cast<float*>(smem_ce);     // [C][CE_ROW_PITCH]
  float* stage = dz + (long)a.C * CE_ROW_PITCH;      // [SJ][C]
  const int h = blockIdx.y, n = blockIdx.z;
  const int j0 = blockIdx.x * SJ, j1 = min(a.Wi, j0 + SJ) - 1, nj = j1 - j0 + 1;
  // output columns touching [j0, j1]: nw <= CE_ROW_THREADS (checked on the host, column by column)
  int wlo, whi, t0, t1;
  cand_range(a.sw, j0, a.W, a.align, wlo, t1);
  cand_range(a.sw, j1, a.W, a.align, t0, whi);
  const int nw = whi - wlo + 1;
  const float g = gout[0] * gscale[1];  // dLoss * (1 / valid count)
  if ((int)threadIdx.x < nw) {
    const int w = wlo + threadIdx.x;
    // the target and the four logit taps are requested together (the softmax of an ignored
    // pixel — 5 % of Cityscapes-like labels — is computed and discarded: a branch on the
    // target would put a second, dependent memory round trip behind the first)
    const long t = a.target[((long)n * a.H + h) * a.W + w];
    float z[NC];
    ce_logits<T, NC>(a, n, h, w, z);
    const bool valid = t != a.ignore && t >= 0 && t < a.C;
    float m = z[0];
#pragma unroll
    for (int c = 1; c < NC; ++c) m = (c < a.C) ? fmaxf(m, z[c]) : m;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      z[c] = (c < a.C) ? expf(z[c] - m) : 0.f;
      s += z[c];
    }
    const float inv = valid ? g / s : 0.f, hot = valid ? g : 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) z[c] = z[c] * inv - (c == (int)t ? hot : 0.f);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < a.C) dz[c * CE_ROW_PITCH + threadIdx.x] = z[c];
  }
  __syncthreads();
  // ---- along w: CE_ROW_TPJ threads share a column and split its classes, so a tap weight is
  // derived once per (column, candidate) and not once per class
  const int cg = threadIdx.x % CE_ROW_TPJ;
  for (int jj = threadIdx.x / CE_ROW_TPJ; jj < nj; jj += CE_ROW_THREADS / CE_ROW_TPJ) {
    int clo, chi;
    cand_range(a.sw, j0 + jj, a.W, a.align, clo, chi);
    float v[NC / CE_ROW_TPJ];
#pragma unroll
    for (int k = 0; k < NC / CE_ROW_TPJ; ++k) v[k] = 0.f;
    for (int w = clo; w <= chi; ++w) {
      const float wt = tap_weight(a.sw, w, a.Wi, a.align, j0 + jj);
      if (wt == 0.f) continue;
      const float* col = dz + (w - wlo);
#pragma unroll
      for (int k = 0; k < NC / CE_ROW_TPJ; ++k) {
        const int c = cg + k * CE_ROW_TPJ;
        if (c < a.C) v[k] = fmaf(wt, col[c * CE_ROW_PITCH], v[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < NC / CE_ROW_TPJ; ++k) {
      const int c = cg + k * CE_ROW_TPJ;
      if (c < a.C) stage[jj * a.C + c] = v[k];
    }
  }
  __syncthreads();
  float* __restrict__ out = ws + (((long)n * a.H + h) * a.Wi + j0) * a.C;
  for (int p = threadIdx.x; p < nj * a.C; p += CE_ROW_THREADS) out[p] = stage[p];
}

constexpr int CE_COL_THREADS = 256;
constexpr int CE_COL_BATCH = 8;  // workspace rows requested together
template <typename T>
__global__ __launch_bounds__(CE_COL_THREADS) void ce_bwd_col_kernel(const float* __restrict__ ws,
                                                                    T* __restrict__ dlo, int ld,
                                                                    int Hi, int Wi, int H, int C,
                                                                    float sh, int align) {
  // the rows of cand_range(i) that carry weight, ascending, 64 candidates at a time
  __shared__ float s_wt[64];
  __shared__ int s_row[64];
  __shared__ int s_cnt;
  const int i = blockIdx.y, n = blockIdx.z;
  const int q = blockIdx.x * CE_COL_THREADS + threadIdx.x;  // (j, c) of the padded row
  const int j = q / ld, c = q - j * ld;
  const bool live = j < Wi && c < C;
  const float* __restrict__ src = ws + ((long)n * H * Wi + (live ? j : 0)) * C + (live ? c : 0);
  const long pitch = (long)Wi * C;
  int hlo, hhi;
  cand_range(sh, i, H, align, hlo, hhi);
  float acc = 0.f;
  for (int hb = hlo; hb <= hhi; hb += 64) {
    if (threadIdx.x < 64) {
      const int h = hb + threadIdx.x;
      const float wt = h <= hhi ? tap_weight(sh, h, Hi, align, i) : 0.f;
      const unsigned long long mask = __ballot(wt != 0.f);
      const int pos = __popcll(mask & ((1ull << threadIdx.x) - 1ull));
      if (wt != 0.f) { s_wt[pos] = wt; s_row[pos] = h; }
      if (threadIdx.x == 0) s_cnt = __popcll(mask);
    }
    __syncthreads();
    const int cnt = s_cnt;
    if (live) {
      // CE_COL_BATCH loads in flight at a time (slots past the end of the list repeat its last
      // load and are not added)
      for (int k0 = 0; k0 < cnt; k0 += CE_COL_BATCH) {
        float v[CE_COL_BATCH];
#pragma unroll
        for (int u = 0; u < CE_COL_BATCH; ++u) v[u] = src[s_row[min(k0 + u, cnt - 1)] * pitch];
#pragma unroll
        for (int u = 0; u < CE_COL_BATCH; ++u)
          if (k0 + u < cnt) acc = fmaf(s_wt[k0 + u], v[u], acc);
      }
    }
    __syncthreads();
  }
  if (j < Wi) Vec<T>::store1(dlo + (((long)n * Hi + i) * Wi + j) * ld + c, acc);
}

}  // namespace seg

// loss_out: float32[2] = (mean loss, 1 / valid count); ws: >= 2 * seg_upsample_ce_blocks doubles
extern "C" int seg_upsample_ce_blocks(int N, int H, int W) {
  const long total = (long)N * H * W;
  long b = (total + seg::CE_THREADS - 1) / seg::CE_THREADS;
  return (int)(b > 4096 ? 4096 : b);
}

extern "C" int seg_upsample_ce_fwd(int dtype, const void* lo, long ld, int N, int Hi, int Wi, int C,
                                   const long* target, int H, int W, long ignore_index,
                                   int align_corners, double* ws, float* loss_out, void* stream) {
  using namespace seg;
  SEG_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "upsample_ce_fwd: bad dtype %d", dtype);
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(C >= 1 && C <= 32 && ld % vec == 0 && ld >= (C + vec - 1) / vec * vec,
              "upsample_ce_fwd: C=%d must be <= 32 and the pitch %ld a padded multiple of %d", C,
              ld, vec);
  SEG_REQUIRE(N > 0 && Hi > 0 && Wi > 0 && H > 0 && W > 0, "upsample_ce_fwd: empty problem");
  CeArgs a;
  a.lo = lo; a.target = target; a.ld = ld; a.N = N; a.Hi = Hi; a.Wi = Wi; a.H = H; a.W = W;
  a.C = C; a.ignore = ignore_index; a.align = align_corners;
  a.sh = host_scale(Hi, H, align_corners); a.sw = host_scale(Wi, W, align_corners);
  const int blocks = seg_upsample_ce_blocks(N, H, W);
  hipStream_t st = (hipStream_t)stream;
  const int nc = C <= 24 ? 24 : 32;
  if (dtype == DT_BF16) {
    if (nc == 24) hipLaunchKernelGGL((ce_fwd_kernel<bf16_t, 24>), dim3(blocks), dim3(CE_THREADS), 0, st, a, ws);
    else hipLaunchKernelGGL((ce_fwd_kernel<bf16_t, 32>), dim3(blocks), dim3(CE_THREADS), 0, st, a, ws);
  } else {
    if (nc == 24) hipLaunchKernelGGL((ce_fwd_kernel<float, 24>), dim3(blocks), dim3(CE_THREADS), 0, st, a, ws);
    else hipLaunchKernelGGL((ce_fwd_kernel<float, 32>), dim3(blocks), dim3(CE_THREADS), 0, st, a, ws);
  }
  hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, st, ws, blocks, loss_out);
  return check_launch("upsample_ce_fwd");
}

// Segment width of the row pass: the most low-resolution columns whose footprint of output columns,
// (SJ + 1.5) / scale + 5 at the outside, still fits one block, spread evenly over the segments
static int ce_bwd_seg_width(int Wi, float sw) {
  int sj = 1;
  if (sw > 0.f) {
    sj = (int)floorf((float)(seg::CE_ROW_THREADS - 5) * sw - 1.5f);
    sj = sj < 1 ? 1 : (sj > seg::CE_ROW_MAX_SJ ? seg::CE_ROW_MAX_SJ : sj);
  }
  const int nseg = (Wi + sj - 1) / sj;
  return (Wi + nseg - 1) / nseg;
}

// bytes of the fp32 workspace [N][H][Wi][C] between the two passes of seg_upsample_ce_bwd
// (-1: more than an int holds)
extern "C" int seg_upsample_ce_bwd_ws_bytes(int N, int H, int Wi, int C) {
  if (N <= 0 || H <= 0 || Wi <= 0 || C <= 0) return 0;
  const long b = (long)N * H * Wi * C * (long)sizeof(float);
  return b > 0x7fffffffL ? -1 : (int)b;
}

extern "C" int seg_upsample_ce_bwd(int dtype, const void* lo, long ld, int N, int Hi, int Wi, int C,
                                   const long* target, int H, int W, long ignore_index,
                                   int align_corners, const float* loss_out, const float* grad_out,
                                   void* dlo, long lddlo, float* ws, long ws_bytes, void* stream) {
  using namespace seg;
  SEG_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "upsample_ce_bwd: bad dtype %d", dtype);
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(C >= 1 && C <= 32 && ld % vec == 0 && lddlo >= C && lddlo <= 32,
              "upsample_ce_bwd: bad C / pitch (1 <= C <= lddlo <= 32)");
  SEG_REQUIRE(N > 0 && Hi > 0 && Wi > 0 && H > 0 && W > 0, "upsample_ce_bwd: empty problem");
  SEG_REQUIRE(H >= Hi && W >= Wi, "upsample_ce_bwd: the fused loss is for UP-sampling heads");
  const float sh = host_scale(Hi, H, align_corners), sw = host_scale(Wi, W, align_corners);
  const float smin = fminf(sh > 0.f ? sh : 1.f, sw > 0.f ? sw : 1.f);
  SEG_REQUIRE(1.f / smin <= CE_MAX_SCALE,
              "upsample_ce_bwd: scale factor %.2f too large for the fused backward", 1.f / smin);
  SEG_REQUIRE(N <= 65535 && H <= 65535, "upsample_ce_bwd: N=%d / H=%d beyond the launch grid", N, H);
  SEG_REQUIRE(ws && ws_bytes >= (long)N * H * Wi * C * (long)sizeof(float),
              "upsample_ce_bwd: workspace of %ld bytes, seg_upsample_ce_bwd_ws_bytes asks for more",
              ws_bytes);
  // every column's candidate range must lie inside the footprint of the segment that owns it, and
  // the footprint inside the block: the kernel's own float formulas, column by column
  const int SJ = ce_bwd_seg_width(Wi, sw), nseg = (Wi + SJ - 1) / SJ;
  for (int s = 0; s < nseg; ++s) {
    const int j0 = s * SJ, j1 = (j0 + SJ < Wi ? j0 + SJ : Wi) - 1;
    int wlo, whi, t0, t1;
    cand_range(sw, j0, W, align_corners, wlo, t1);
    cand_range(sw, j1, W, align_corners, t0, whi);
    SEG_REQUIRE(whi - wlo + 1 <= CE_ROW_THREADS,
                "upsample_ce_bwd: columns %d..%d touch %d output columns, a block holds %d", j0, j1,
                whi - wlo + 1, CE_ROW_THREADS);
    for (int j = j0; j <= j1; ++j) {
      int clo, chi;
      cand_range(sw, j, W, align_corners, clo, chi);
      SEG_REQUIRE(clo >= wlo && chi <= whi && clo <= chi,
                  "upsample_ce_bwd: column %d gathers outside its segment", j);
    }
  }
  CeArgs a;
  a.lo = lo; a.target = target; a.ld = ld; a.N = N; a.Hi = Hi; a.Wi = Wi; a.H = H; a.W = W;
  a.C = C; a.ignore = ignore_index; a.align = align_corners; a.sh = sh; a.sw = sw;
  hipStream_t st = (hipStream_t)stream;
  const int nc = C <= 24 ? 24 : 32;
  const size_t lds = ((size_t)C * CE_ROW_PITCH + (size_t)SJ * C) * sizeof(float);  // <= 49 KiB
  const dim3 rgrid(nseg, H, N);
  if (dtype == DT_BF16) {
    if (nc == 24) hipLaunchKernelGGL((ce_bwd_row_kernel<bf16_t, 24>), rgrid, dim3(CE_ROW_THREADS), lds, st, a, loss_out, grad_out, ws, SJ);
    else hipLaunchKernelGGL((ce_bwd_row_kernel<bf16_t, 32>), rgrid, dim3(CE_ROW_THREADS), lds, st, a, loss_out, grad_out, ws, SJ);
  } else {
    if (nc == 24) hipLaunchKernelGGL((ce_bwd_row_kernel<float, 24>), rgrid, dim3(CE_ROW_THREADS), lds, st, a, loss_out, grad_out, ws, SJ);
    else hipLaunchKernelGGL((ce_bwd_row_kernel<float, 32>), rgrid, dim3(CE_ROW_THREADS), lds, st, a, loss_out, grad_out, ws, SJ);
  }
  const dim3 cgrid((unsigned)(((long)Wi * lddlo + CE_COL_THREADS - 1) / CE_COL_THREADS), Hi, N);
  if (dtype == DT_BF16)
    hipLaunchKernelGGL((ce_bwd_col_kernel<bf16_t>), cgrid, dim3(CE_COL_THREADS), 0, st, ws,
                       reinterpret_cast<bf16_t*>(dlo), (int)lddlo, Hi, Wi, H, C, sh, align_corners);
  else
    hipLaunchKernelGGL((ce_bwd_col_kernel<float>), cgrid, dim3(CE_COL_THREADS), 0, st, ws,
                       reinterpret_cast<float*>(dlo), (int)lddlo, Hi, Wi, H, C, sh, align_corners);
  return check_launch("upsample_ce_bwd");
}
