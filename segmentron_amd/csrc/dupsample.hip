// DUpsampling ("Decoders Matter", segmentron/models/dunet.py:90-117) on the LOW-resolution NHWC
// output of its 1x1 convolution.  The reference rearranges conv_w(x) [N, s*s*C, h, w] into the
// full-resolution logits [N, C, h*s, w*s] with three permute / contiguous / view rounds:
//     out[n, k, hh*s + a, ww*s + b] = conv_w(x)[n, (a*s + b)*C + k, hh, ww]
// In NHWC the C logits of every full-resolution pixel are therefore C CONSECUTIVE elements of
// the low-resolution row lo[n, hh, ww, :], and
//     F.cross_entropy(DUpsampling(x), target, ignore_index)               solver/loss.py:16-46
// is a row cross-entropy over R = N*h*w*s*s rows whose target sits at a permuted address.  The
// full-resolution tensor (90 MB in bf16 at 4 x 96 x 96 x 1216, 180 MB as the float32 the loss
// reads) is never written in any other order; the gradient comes out in the layout the 1x1
// convolution's backward reads.
//
// One block owns TW consecutive low-resolution pixels of one image row: their values are one
// contiguous run of global memory, fetched with 16-byte loads into LDS as float32; one thread
// then owns one full-resolution pixel and walks its C values in LDS (lane stride C dwords:
// conflict-free for the odd class counts 19 and 21; an even C pays bank conflicts, not
// correctness).  The s target rows a block touches are runs of TW*s labels each.  The backward
// recomputes the softmax from the staged row, overwrites it in LDS with the gradient and stores
// the run with 16-byte stores.
//
// Numerics are those of the row cross-entropy in csrc/pointrend.hip, operation for operation:
// lse = log(sum_c exp(z_c - max)) summed in class order, loss = lse - (z_t - max),
// d z_c = g * (exp(z_c - max - lse) - [c == t]) with g = grad_out / valid count; labels outside
// [0, C) are left out of sum and count like ignore_index.  Partial sums are float64, reduced in a
// fixed order: bitwise deterministic, no atomics.
#include <math.h>

#include "common.h"

namespace seg {

constexpr int DUP_THREADS = 256;
constexpr int DUP_LDS_BYTES = 48 * 1024;  // staged rows + the block reduction's 64 bytes

struct DupArgs {
  const void* lo;  // [N, h, w, ld], element type T (unused by the NCHW -> NHWC direction)
  long ld;
  int N, h, w, s, C;
  int TW;       // low-resolution pixels per block
  int tiles_w;  // blocks per image row
  int rowv;     // 16-byte vectors that hold the s*s*C values of one pixel
};

struct DupTile {
  int n, hh, w0, npix;
};

__device__ __forceinline__ DupTile dup_tile(const DupArgs& a) {
  DupTile t;
  const int tw = blockIdx.x % a.tiles_w;
  const int q = blockIdx.x / a.tiles_w;
  t.hh = q % a.h;
  t.n = q / a.h;
  t.w0 = tw * a.TW;
  t.npix = min(a.TW, a.w - t.w0);
  return t;
}

// the tile's values -> sm[p * KP + e] as float32 (KP = rowv * VEC; e < s*s*C are the logits)
template <typename T>
__device__ __forceinline__ void dup_stage(const DupArgs& a, const DupTile& t, float* sm) {
  constexpr int VEC = Vec<T>::N;
  const T* __restrict__ src =
      reinterpret_cast<const T*>(a.lo) + (((long)t.n * a.h + t.hh) * a.w + t.w0) * a.ld;
  const int nvec = t.npix * a.rowv;
  for (int v = threadIdx.x; v < nvec; v += DUP_THREADS) {
    const int p = v / a.rowv, j = v - p * a.rowv;
    float f[VEC];
    Vec<T>::unpack(ldg16(src + (long)p * a.ld + j * VEC), f);
    float4* d = reinterpret_cast<float4*>(sm + (long)v * VEC);
#pragma unroll
    for (int i = 0; i < VEC / 4; ++i)
      d[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
  }
}

// sm -> dst[N, h, w, ldd] (element type T) with 16-byte stores; elements >= s*s*C of every pixel
// are written as zeros up to the pitch
template <typename T>
__device__ __forceinline__ void dup_store(const DupArgs& a, const DupTile& t, const float* sm,
                                          T* __restrict__ dst, long ldd) {
  constexpr int VEC = Vec<T>::N;
  const int K = a.s * a.s * a.C, KP = a.rowv * VEC;
  const int outv = (int)(ldd / VEC), nvec = t.npix * outv;
  T* __restrict__ out = dst + (((long)t.n * a.h + t.hh) * a.w + t.w0) * ldd;
  for (int v = threadIdx.x; v < nvec; v += DUP_THREADS) {
    const int p = v / outv, j = v - p * outv;
    float f[VEC];
    if (j < a.rowv) {
      const float4* src = reinterpret_cast<const float4*>(sm + (long)p * KP + j * VEC);
#pragma unroll
      for (int i = 0; i < VEC / 4; ++i) {
        const float4 q = src[i];
        f[4 * i] = q.x; f[4 * i + 1] = q.y; f[4 * i + 2] = q.z; f[4 * i + 3] = q.w;
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i)
        if (j * VEC + i >= K) f[i] = 0.f;
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) f[i] = 0.f;
    }
    stg16(out + (long)p * ldd + j * VEC, Vec<T>::pack(f));
  }
}

// row r of the tile = (pixel p, sub-row aa, sub-column b): its offset in sm and its label's index
__device__ __forceinline__ long dup_row(const DupArgs& a, const DupTile& t, int r, int KP,
                                        int& off) {
  const int ss = a.s * a.s;
  const int p = r / ss, q = r - p * ss;
  const int aa = q / a.s, b = q - aa * a.s;
  off = p * KP + q * a.C;
  const long H = (long)a.h * a.s, W = (long)a.w * a.s;
  return ((long)t.n * H + (long)t.hh * a.s + aa) * W + (long)(t.w0 + p) * a.s + b;
}

__device__ __forceinline__ bool dup_valid(long tg, long ignore, int C) {
  return tg != ignore && tg >= 0 && tg < C;
}

// partial[block] = (sum of -log p_target over the block's valid pixels, valid count)
template <typename T>
__global__ __launch_bounds__(DUP_THREADS) void dup_ce_fwd_kernel(const DupArgs a,
                                                                 const long* __restrict__ target,
                                                                 long ignore,
                                                                 double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_dup[];
  float* sm = reinterpret_cast<float*>(smem_dup);
  const int KP = a.rowv * Vec<T>::N;
  double* red = reinterpret_cast<double*>(sm + (long)a.TW * KP);  // [2][DUP_THREADS / 64]
  const DupTile t = dup_tile(a);
  const int rows = t.npix * a.s * a.s;
  // the first label is requested together with the logits
  int r = threadIdx.x, off = 0;
  long tg = ignore;
  if (r < rows) tg = target[dup_row(a, t, r, KP, off)];
  dup_stage<T>(a, t, sm);
  __syncthreads();
  double lsum = 0.0, lcnt = 0.0;
  while (r < rows) {
    const float* z = sm + off;
    float mx = -INFINITY;
    for (int c = 0; c < a.C; ++c) mx = fmaxf(mx, z[c]);
    float sum = 0.f;
    for (int c = 0; c < a.C; ++c) sum += expf(z[c] - mx);
    if (dup_valid(tg, ignore, a.C)) {
      lsum += (double)(logf(sum) - (z[tg] - mx));
      lcnt += 1.0;
    }
    r += DUP_THREADS;
    if (r < rows) tg = target[dup_row(a, t, r, KP, off)];
  }
  // block reduction in a fixed order (wave butterfly, then the waves in index order)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lsum += __shfl_xor(lsum, o, 64);
    lcnt += __shfl_xor(lcnt, o, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[wave] = lsum; red[DUP_THREADS / 64 + wave] = lcnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0, c = 0.0;
    for (int k = 0; k < DUP_THREADS / 64; ++k) { s += red[k]; c += red[DUP_THREADS / 64 + k]; }
    partial[2 * (long)blockIdx.x] = s;
    partial[2 * (long)blockIdx.x + 1] = c;
  }
}

// out[0] = loss (mean over valid pixels), out[1] = 1 / valid count (0 if none), both float32:
// the finalize of csrc/loss.hip, statement for statement
__global__ void dup_ce_finalize_kernel(const double* partial, int nblocks, float* out) {
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

// dlo = grad_out * loss_out[1] * (softmax - onehot); rows of invalid pixels and the pad are zeros
template <typename T>
__global__ __launch_bounds__(DUP_THREADS) void dup_ce_bwd_kernel(const DupArgs a,
                                                                 const long* __restrict__ target,
                                                                 long ignore,
                                                                 const float* __restrict__ loss_out,
                                                                 const float* __restrict__ gout,
                                                                 T* __restrict__ dlo, long lddlo) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_dup[];
  float* sm = reinterpret_cast<float*>(smem_dup);
  const int KP = a.rowv * Vec<T>::N;
  const DupTile t = dup_tile(a);
  const int rows = t.npix * a.s * a.s;
  int r = threadIdx.x, off = 0;
  long tg = ignore;
  if (r < rows) tg = target[dup_row(a, t, r, KP, off)];
  const float g = gout[0] * loss_out[1];  // dLoss * (1 / valid count)
  dup_stage<T>(a, t, sm);
  __syncthreads();
  // every row is read and rewritten by its own thread only
  while (r < rows) {
    float* z = sm + off;
    if (dup_valid(tg, ignore, a.C)) {
      float mx = -INFINITY;
      for (int c = 0; c < a.C; ++c) mx = fmaxf(mx, z[c]);
      float sum = 0.f;
      for (int c = 0; c < a.C; ++c) sum += expf(z[c] - mx);
      const float lse = logf(sum);
      for (int c = 0; c < a.C; ++c) {
        const float p = expf(z[c] - mx - lse);
        z[c] = g * (p - (c == (int)tg ? 1.f : 0.f));
      }
    } else {
      for (int c = 0; c < a.C; ++c) z[c] = 0.f;
    }
    r += DUP_THREADS;
    if (r < rows) tg = target[dup_row(a, t, r, KP, off)];
  }
  __syncthreads();
  dup_store<T>(a, t, sm, dlo, lddlo);
}

// the materialised float32 [N, C, h*s, w*s]: per (class, sub-row) one run of npix*s outputs
template <typename T>
__global__ __launch_bounds__(DUP_THREADS) void dup_to_nchw_kernel(const DupArgs a,
                                                                  float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_dup[];
  float* sm = reinterpret_cast<float*>(smem_dup);
  const int KP = a.rowv * Vec<T>::N;
  const DupTile t = dup_tile(a);
  dup_stage<T>(a, t, sm);
  __syncthreads();
  const int runw = t.npix * a.s, items = a.C * a.s * runw;
  const long H = (long)a.h * a.s, W = (long)a.w * a.s;
  for (int i = threadIdx.x; i < items; i += DUP_THREADS) {
    const int x = i % runw, m = i / runw;
    const int aa = m % a.s, k = m / a.s;
    const int p = x / a.s, b = x - p * a.s;
    out[(((long)t.n * a.C + k) * H + (long)t.hh * a.s + aa) * W + (long)t.w0 * a.s + x] =
        sm[p * KP + (aa * a.s + b) * a.C + k];
  }
}

// its inverse: float32 NCHW gradient -> NHWC in T (pad written as zeros)
template <typename T>
__global__ __launch_bounds__(DUP_THREADS) void dup_to_nchw_bwd_kernel(const DupArgs a,
                                                                      const float* __restrict__ gy,
                                                                      T* __restrict__ gx,
                                                                      long ldgx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_dup[];
  float* sm = reinterpret_cast<float*>(smem_dup);
  const int KP = a.rowv * Vec<T>::N;
  const DupTile t = dup_tile(a);
  const int runw = t.npix * a.s, items = a.C * a.s * runw;
  const long H = (long)a.h * a.s, W = (long)a.w * a.s;
  for (int i = threadIdx.x; i < items; i += DUP_THREADS) {
    const int x = i % runw, m = i / runw;
    const int aa = m % a.s, k = m / a.s;
    const int p = x / a.s, b = x - p * a.s;
    sm[p * KP + (aa * a.s + b) * a.C + k] =
        gy[(((long)t.n * a.C + k) * H + (long)t.hh * a.s + aa) * W + (long)t.w0 * a.s + x];
  }
  __syncthreads();
  dup_store<T>(a, t, sm, gx, ldgx);
}

// Geometry of one launch: TW pixels per block so that a block has about DUP_THREADS rows and its
// staged values fit DUP_LDS_BYTES.  -> 0, or 1 with the error set.
static int dup_plan(const char* what, int dtype, long ld, int N, int h, int w, int s, int C,
                    DupArgs& a, size_t& lds, long& blocks) {
  SEG_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "%s: bad dtype %d", what, dtype);
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(N > 0 && h > 0 && w > 0, "%s: empty problem", what);
  SEG_REQUIRE(C >= 1 && C <= 32 && s >= 1 && s <= 1024, "%s: C=%d must be in [1, 32], s=%d >= 1",
              what, C, s);
  const long K = (long)s * s * C;
  const long rowv = (K + vec - 1) / vec;
  const long row_bytes = rowv * vec * (long)sizeof(float);
  SEG_REQUIRE(row_bytes <= DUP_LDS_BYTES - 64,
              "%s: the %ld values of one pixel (s=%d, C=%d) do not fit the staging buffer", what,
              K, s, C);
  SEG_REQUIRE(ld % vec == 0 && ld >= K, "%s: pitch %ld must be a multiple of %d and >= s*s*C = %ld",
              what, ld, vec, K);
  SEG_REQUIRE((long)h * s <= 0x7fffffffL && (long)w * s <= 0x7fffffffL, "%s: output too large",
              what);
  const long ss = (long)s * s;
  long tw = (DUP_THREADS + ss - 1) / ss;
  const long fit = (DUP_LDS_BYTES - 64) / row_bytes;
  if (tw > fit) tw = fit;
  if (tw > w) tw = w;
  if (tw < 1) tw = 1;
  a.lo = nullptr; a.ld = ld; a.N = N; a.h = h; a.w = w; a.s = s; a.C = C;
  a.TW = (int)tw;
  a.tiles_w = (int)((w + tw - 1) / tw);
  a.rowv = (int)rowv;
  blocks = (long)N * h * a.tiles_w;
  SEG_REQUIRE(blocks <= 0x7fffffffL, "%s: %ld blocks beyond the launch grid", what, blocks);
  lds = (size_t)(tw * row_bytes + 64);
  return 0;
}

static inline bool dup_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace seg

using namespace seg;

extern "C" int seg_dup_ce_blocks(int dtype, long ld, int N, int h, int w, int s, int C) {
  DupArgs a; size_t lds; long blocks;
  if (dup_plan("dup_ce_blocks", dtype, ld, N, h, w, s, C, a, lds, blocks)) return -1;
  return (int)blocks;
}

extern "C" int seg_dup_ce_fwd(int dtype, const void* lo, long ld, int N, int h, int w, int s, int C,
                              const long* target, long ignore_index, double* ws, float* loss_out,
                              void* stream) {
  DupArgs a; size_t lds; long blocks;
  if (dup_plan("dup_ce_fwd", dtype, ld, N, h, w, s, C, a, lds, blocks)) return 1;
  SEG_REQUIRE(lo && target && ws && loss_out && dup_aligned(lo),
              "dup_ce_fwd: null or misaligned pointer");
  a.lo = lo;
  hipStream_t st = (hipStream_t)stream;
  SEG_LAUNCH_T(dup_ce_fwd_kernel, dim3((unsigned)blocks), dim3(DUP_THREADS), lds, st, a, target,
               ignore_index, ws);
  hipLaunchKernelGGL(dup_ce_finalize_kernel, dim3(1), dim3(256), 0, st, ws, (int)blocks, loss_out);
  return check_launch("dup_ce_fwd");
}

extern "C" int seg_dup_ce_bwd(int dtype, const void* lo, long ld, int N, int h, int w, int s, int C,
                              const long* target, long ignore_index, const float* loss_out,
                              const float* grad_out, void* dlo, long lddlo, void* stream) {
  DupArgs a; size_t lds; long blocks;
  if (dup_plan("dup_ce_bwd", dtype, ld, N, h, w, s, C, a, lds, blocks)) return 1;
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(lddlo % vec == 0 && lddlo >= (long)s * s * C,
              "dup_ce_bwd: gradient pitch %ld must be a multiple of %d and >= s*s*C", lddlo, vec);
  SEG_REQUIRE(lo && target && loss_out && grad_out && dlo && dup_aligned(lo) && dup_aligned(dlo),
              "dup_ce_bwd: null or misaligned pointer");
  a.lo = lo;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DT_BF16)
    hipLaunchKernelGGL((dup_ce_bwd_kernel<bf16_t>), dim3((unsigned)blocks), dim3(DUP_THREADS), lds,
                       st, a, target, ignore_index, loss_out, grad_out,
                       reinterpret_cast<bf16_t*>(dlo), lddlo);
  else
    hipLaunchKernelGGL((dup_ce_bwd_kernel<float>), dim3((unsigned)blocks), dim3(DUP_THREADS), lds,
                       st, a, target, ignore_index, loss_out, grad_out,
                       reinterpret_cast<float*>(dlo), lddlo);
  return check_launch("dup_ce_bwd");
}

extern "C" int seg_dup_to_nchw(int dtype, const void* lo, long ld, int N, int h, int w, int s, int C,
                               float* out, void* stream) {
  DupArgs a; size_t lds; long blocks;
  if (dup_plan("dup_to_nchw", dtype, ld, N, h, w, s, C, a, lds, blocks)) return 1;
  SEG_REQUIRE(lo && out && dup_aligned(lo), "dup_to_nchw: null or misaligned pointer");
  a.lo = lo;
  hipStream_t st = (hipStream_t)stream;
  SEG_LAUNCH_T(dup_to_nchw_kernel, dim3((unsigned)blocks), dim3(DUP_THREADS), lds, st, a, out);
  return check_launch("dup_to_nchw");
}

extern "C" int seg_dup_to_nchw_bwd(int dtype, void* gx, long ldgx, int N, int h, int w, int s, int C,
                                   const float* gy, void* stream) {
  DupArgs a; size_t lds; long blocks;
  if (dup_plan("dup_to_nchw_bwd", dtype, ldgx, N, h, w, s, C, a, lds, blocks)) return 1;
  SEG_REQUIRE(gx && gy && dup_aligned(gx), "dup_to_nchw_bwd: null or misaligned pointer");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DT_BF16)
    hipLaunchKernelGGL((dup_to_nchw_bwd_kernel<bf16_t>), dim3((unsigned)blocks), dim3(DUP_THREADS),
                       lds, st, a, gy, reinterpret_cast<bf16_t*>(gx), ldgx);
  else
    hipLaunchKernelGGL((dup_to_nchw_bwd_kernel<float>), dim3((unsigned)blocks), dim3(DUP_THREADS),
                       lds, st, a, gy, reinterpret_cast<float*>(gx), ldgx);
  return check_launch("dup_to_nchw_bwd");
}
