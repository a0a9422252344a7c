// Depthwise 3x3 convolution (groups == C), NHWC, any stride / dilation, pad = dil.
// Reference call sites: segmentron/modules/basic.py:38-40 (SeparableConv2d.depthwise),
// :152-153 (InvertedResidual dw).  68 instances in DeepLabv3+/xception65: 1.5 % of
// the MACs but as much HBM traffic as all 1x1 convs -> purely bandwidth-bound, so the kernel is
// built around 16-byte channel vectors (8 bf16 / 4 f32 per lane, consecutive lanes = consecutive
// channel vectors = fully coalesced NHWC rows) with the producer's BatchNorm(+ReLU) fused into
// the load path and the consumer BatchNorm's sum / sum-of-squares fused into the store path.
//
//   MODE_FWD   : y[n,ho,wo,c] = sum_{kh,kw} act(x[n, ho*s-p+kh*d, wo*s-p+kw*d, c]) * w[kh,kw,c]
//   MODE_DGRAD : dx[n,h,w,c]  = sum_{kh,kw} dy[n,(h+p-kh*d)/s,(w+p-kw*d)/s,c] * w[kh,kw,c]
//                (terms kept only when the division is exact and in range)
//   wgrad      : dw[kh,kw,c]  = sum_{n,ho,wo} dy[n,ho,wo,c] * act(x[n, ho*s-p+kh*d, ...,c])
//
// Thread layout: block = CVB channel-vectors (8/16/32, chosen by the host to fit C) x 256/CVB
// pixel strips; a strip is TW=4 consecutive output pixels of one row.  blockIdx.x tiles the
// channel vectors, blockIdx.y the strips (grid-stride), one row of statistics partials per
// blockIdx.y (deterministic: LDS tree over the strips of a block, fp64 finish in bn_finalize).
#include "rows.h"
#include "dwconv.h"
#include <cstdlib>
#include <type_traits>

namespace seg {

constexpr int DW_TW = 4;
constexpr int DW_THREADS = 256;
enum { MODE_FWD = 0, MODE_DGRAD = 1 };

struct DwArgs {
  const void* x;      // fwd: input; dgrad: dy
  const float* w;     // [9][C] fp32, tap-major
  void* y;            // fwd: output; dgrad: dx
  const float* pro_scale;
  const float* pro_shift;
  float* stat_partial;  // [gridDim.y][2][C] or null (fwd only)
  long ldx, ldy;
  int N, Hi, Wi, C;   // geometry of the tensor being READ
  int Ho, Wo;         // geometry of the tensor being WRITTEN
  int stride, pad, dil;
  int pro_mode;
  int cvb_log2;       // log2(CVB)
  int CV;             // C / VEC
  long strips;        // N * Ho * ceil(Wo / TW)
};

// (the per-strip index decode divides with fast_div — common.h states its contract, the launchers
// below enforce it on the strip count)

template <int VEC>
__device__ __forceinline__ void dw_act(float* f, int mode, const float* sc, const float* sh) {
  if (mode & PRO_AFFINE) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) f[i] = fmaf(f[i], sc[i], sh[i]);
  }
  if (mode & PRO_RELU) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) f[i] = fmaxf(f[i], 0.f);
  }
  if (mode & PRO_CLAMP6) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) f[i] = fminf(f[i], 6.f);
  }
}

// Strip kernels: the fallback of dw_route (below) — strided data gradients, strides and dilations no
// other family takes (stride 2 with dilation, stride 3, dilation > 64); the networks' stride-1
// layers run on the sliding (dil 1), LDS-tiled (dil 2) and row-chain (dil 6/12/18/...) kernels.
template <typename T, int MODE>
__global__ __launch_bounds__(DW_THREADS, 2) void dwconv_kernel(const DwArgs a) {
  using V = Vec<T>;
  constexpr int VEC = V::N;
  extern __shared__ __attribute__((aligned(16))) float dw_smem[];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int spb = DW_THREADS >> a.cvb_log2;  // strips per block iteration
  const int cv = blockIdx.x * cvb + cx;
  const bool cok = cv < a.CV;
  const int c0 = cok ? cv * VEC : 0;
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  T* __restrict__ Y = reinterpret_cast<T*>(a.y);
  const int WQ = (a.Wo + DW_TW - 1) / DW_TW;
  const float inv_wq = 1.0f / (float)WQ, inv_ho = 1.0f / (float)a.Ho;

  float sc[VEC], sh[VEC];
  if (a.pro_mode & PRO_AFFINE) {
    load_params<VEC>(a.pro_scale, c0, sc);
    load_params<VEC>(a.pro_shift, c0, sh);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) { sc[i] = 1.f; sh[i] = 0.f; }
  }
  float ssum[VEC], ssq[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) ssum[i] = ssq[i] = 0.f;

  const int nstrips = (int)a.strips;
  for (int s = blockIdx.y * spb + sy; s < nstrips; s += gridDim.y * spb) {
    if (!cok) continue;
    const int t = fast_div(s, WQ, inv_wq);
    const int wq = s - t * WQ;
    const int n = fast_div(t, a.Ho, inv_ho);
    const int ho = t - n * a.Ho;
    const int w0 = wq * DW_TW;
    float acc[DW_TW][VEC];
#pragma unroll
    for (int j = 0; j < DW_TW; ++j)
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[j][i] = 0.f;

#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      int hi;
      if (MODE == MODE_FWD) {
        hi = ho * a.stride - a.pad + kh * a.dil;
      } else {
        const int hn = ho + a.pad - kh * a.dil;
        if (hn < 0 || (hn % a.stride) != 0) continue;
        hi = hn / a.stride;
      }
      if (hi < 0 || hi >= a.Hi) continue;
      const long rowbase = ((long)n * a.Hi + hi) * a.Wi;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        float wv[VEC];
        load_params<VEC>(a.w + (kh * 3 + kw) * a.C, c0, wv);
#pragma unroll
        for (int j = 0; j < DW_TW; ++j) {
          const int wo = w0 + j;
          int wi;
          bool ok = wo < a.Wo;
          if (MODE == MODE_FWD) {
            wi = wo * a.stride - a.pad + kw * a.dil;
          } else {
            const int wn = wo + a.pad - kw * a.dil;
            ok = ok && wn >= 0 && (wn % a.stride) == 0;
            wi = wn / a.stride;
          }
          ok = ok && wi >= 0 && wi < a.Wi;
          if (ok) {
            float f[VEC];
            V::unpack_raw(V::load_raw(X + (rowbase + wi) * a.ldx + c0), f);
            dw_act<VEC>(f, a.pro_mode, sc, sh);
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[j][i] = fmaf(f[i], wv[i], acc[j][i]);
          }
        }
      }
    }
    const long orow = ((long)n * a.Ho + ho) * a.Wo;
#pragma unroll
    for (int j = 0; j < DW_TW; ++j) {
      if (w0 + j < a.Wo) {
        V::store(Y + (orow + w0 + j) * a.ldy + c0, acc[j]);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          ssum[i] += acc[j][i];
          ssq[i] += acc[j][i] * acc[j][i];
        }
      }
    }
  }

  if (a.stat_partial != nullptr) {
    // dw_smem: [spb][cvb][2*VEC]
    float* mine = dw_smem + ((long)sy * cvb + cx) * 2 * VEC;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      mine[i] = ssum[i];
      mine[VEC + i] = ssq[i];
    }
    __syncthreads();
    for (int e = tid; e < cvb * 2 * VEC; e += DW_THREADS) {
      float tot = 0.f;
      for (int r = 0; r < spb; ++r) tot += dw_smem[(long)r * cvb * 2 * VEC + e];
      const int lcx = e / (2 * VEC), k = e % (2 * VEC);
      const int which = k / VEC, ci = k % VEC;
      const int c = (blockIdx.x * cvb + lcx) * VEC + ci;
      if (c < a.C) a.stat_partial[((long)blockIdx.y * 2 + which) * a.C + c] = tot;
    }
  }
}

// ---- weight gradient: partial[blockIdx.y][9][C]
struct DwWgradArgs {
  const void* x;   // forward input (pre-activation raw tensor + prologue)
  const void* dy;  // grad wrt dw output
  float* partial;  // [gridDim.y][9][C]
  const float* pro_scale;
  const float* pro_shift;
  long ldx, lddy;
  int N, Hi, Wi, C, Ho, Wo;
  int stride, pad, dil;
  int pro_mode;
  int cvb_log2, CV;
  long strips;
};

template <typename T>
__global__ __launch_bounds__(DW_THREADS) void dwconv_wgrad_kernel(const DwWgradArgs a) {
  constexpr int VEC = Vec<T>::N;
  extern __shared__ __attribute__((aligned(16))) float dw_smem[];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int spb = DW_THREADS >> a.cvb_log2;
  const int cv = blockIdx.x * cvb + cx;
  const bool cok = cv < a.CV;
  const int c0 = cok ? cv * VEC : 0;
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ DY = reinterpret_cast<const T*>(a.dy);
  const int WQ = (a.Wo + DW_TW - 1) / DW_TW;
  const float inv_wq = 1.0f / (float)WQ, inv_ho = 1.0f / (float)a.Ho;

  float sc[VEC], sh[VEC];
  if (a.pro_mode & PRO_AFFINE) {
    load_params<VEC>(a.pro_scale, c0, sc);
    load_params<VEC>(a.pro_shift, c0, sh);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) { sc[i] = 1.f; sh[i] = 0.f; }
  }
  float acc[9][VEC];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[k][i] = 0.f;

  const int nstrips = (int)a.strips;
  for (int s = blockIdx.y * spb + sy; s < nstrips; s += gridDim.y * spb) {
    if (!cok) continue;
    const int t = fast_div(s, WQ, inv_wq);
    const int wq = s - t * WQ;
    const int n = fast_div(t, a.Ho, inv_ho);
    const int ho = t - n * a.Ho;
    const int w0 = wq * DW_TW;
    const long orow = ((long)n * a.Ho + ho) * a.Wo;
    float g[DW_TW][VEC];
#pragma unroll
    for (int j = 0; j < DW_TW; ++j) {
      const int wc = min(w0 + j, a.Wo - 1);
      Vec<T>::unpack(ldg16(DY + (orow + wc) * a.lddy + c0), g[j]);
      const float keep = (w0 + j < a.Wo) ? 1.f : 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) g[j][i] *= keep;
    }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int hi = ho * a.stride - a.pad + kh * a.dil;
      if (hi < 0 || hi >= a.Hi) continue;
      const long rowbase = ((long)n * a.Hi + hi) * a.Wi;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
#pragma unroll
        for (int j = 0; j < DW_TW; ++j) {
          const int wi = (w0 + j) * a.stride - a.pad + kw * a.dil;
          if (w0 + j < a.Wo && wi >= 0 && wi < a.Wi) {
            float f[VEC];
            Vec<T>::unpack(ldg16(X + (rowbase + wi) * a.ldx + c0), f);
            dw_act<VEC>(f, a.pro_mode, sc, sh);
#pragma unroll
            for (int i = 0; i < VEC; ++i)
              acc[kh * 3 + kw][i] = fmaf(f[i], g[j][i], acc[kh * 3 + kw][i]);
          }
        }
      }
    }
  }
  // block reduction over the strips, three taps at a time (LDS: [spb][cvb][3*VEC])
#pragma unroll
  for (int k3 = 0; k3 < 3; ++k3) {
    float* mine = dw_smem + ((long)sy * cvb + cx) * 3 * VEC;
#pragma unroll
    for (int kk = 0; kk < 3; ++kk)
#pragma unroll
      for (int i = 0; i < VEC; ++i) mine[kk * VEC + i] = acc[k3 * 3 + kk][i];
    __syncthreads();
    for (int e = tid; e < cvb * 3 * VEC; e += DW_THREADS) {
      float tot = 0.f;
      for (int r = 0; r < spb; ++r) tot += dw_smem[(long)r * cvb * 3 * VEC + e];
      const int lcx = e / (3 * VEC), k = e % (3 * VEC);
      const int kk = k / VEC, ci = k % VEC;
      const int c = (blockIdx.x * cvb + lcx) * VEC + ci;
      if (c < a.C) a.partial[((long)blockIdx.y * 9 + k3 * 3 + kk) * a.C + c] = tot;
    }
    __syncthreads();
  }
}

// ---- fused backward (stride 1):  one pass over (dy, x) produces
//   g'[p]      = relu_mask(x[p]) * sum_k dy[p - dk] * w[k]          (data gradient wrt act(x))
//   dW[k]     += dy[p - dk] * act(x[p])                              (the SAME shifted dy values)
//   (sum g', sum g'*x)                                               (BatchNorm-backward sums)
// replacing three kernels (dgrad, wgrad, bn_bwd_reduce) that each re-read dy / x.
struct DwBwdArgs {
  const void* dy; const void* x; void* g;
  const float* w;  // [9][C]
  const float* pro_scale; const float* pro_shift;
  float* partial_w;   // [gridDim.y][9][C]
  float* partial_bn;  // [gridDim.y][2][C] or null
  long lddy, ldx, ldg;
  int N, H, W, C, dil, pro_mode, cvb_log2, CV;
  long strips;
};

template <typename T>
__global__ __launch_bounds__(DW_THREADS) void dwconv_bwd_fused_kernel(const DwBwdArgs a) {
  constexpr int VEC = HVec<T>::N;  // 4 channels per thread (8-byte bf16 vectors): this kernel
                                   // carries 9 tap accumulators per channel
  extern __shared__ __attribute__((aligned(16))) float dw_smem[];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int spb = DW_THREADS >> a.cvb_log2;
  const int cv = blockIdx.x * cvb + cx;
  const bool cok = cv < a.CV;
  const int c0 = cok ? cv * VEC : 0;
  const T* __restrict__ DY = reinterpret_cast<const T*>(a.dy);
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  T* __restrict__ G = reinterpret_cast<T*>(a.g);
  const int WQ = (a.W + DW_TW - 1) / DW_TW;
  const float inv_wq = 1.0f / (float)WQ, inv_h = 1.0f / (float)a.H;
  const int d = a.dil;

  float sc[VEC], sh[VEC];
  if (a.pro_mode & PRO_AFFINE) {
    load_params<VEC>(a.pro_scale, c0, sc);
    load_params<VEC>(a.pro_shift, c0, sh);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) { sc[i] = 1.f; sh[i] = 0.f; }
  }
  float accw[9][VEC], s1[VEC], s2[VEC];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int i = 0; i < VEC; ++i) accw[k][i] = 0.f;
#pragma unroll
  for (int i = 0; i < VEC; ++i) s1[i] = s2[i] = 0.f;

  const int nstrips = (int)a.strips;
  for (int s = blockIdx.y * spb + sy; s < nstrips; s += gridDim.y * spb) {
    if (!cok) continue;
    const int t = fast_div(s, WQ, inv_wq);
    const int wq = s - t * WQ;
    const int n = fast_div(t, a.H, inv_h);
    const int h = t - n * a.H;
    const int w0 = wq * DW_TW;
    const long prow = ((long)n * a.H + h) * a.W;
    // centre pixels: raw x (for mask / BN sums) and activated x (for the weight gradient)
    float xr[DW_TW][VEC], xa[DW_TW][VEC], g[DW_TW][VEC];
#pragma unroll
    for (int j = 0; j < DW_TW; ++j) {
      const int wc = min(w0 + j, a.W - 1);
      HVec<T>::load(X + (prow + wc) * a.ldx + c0, xr[j]);
      const float keep = (w0 + j < a.W) ? 1.f : 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        xa[j][i] = xr[j][i];
        g[j][i] = 0.f;
      }
      dw_act<VEC>(xa[j], a.pro_mode, sc, sh);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        xa[j][i] *= keep;
        xr[j][i] *= keep;
      }
    }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int r = h + (1 - kh) * d;
      if (r < 0 || r >= a.H) continue;
      const long rowbase = ((long)n * a.H + r) * a.W;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        float wv[VEC];
        load_params<VEC>(a.w + (kh * 3 + kw) * a.C, c0, wv);
#pragma unroll
        for (int j = 0; j < DW_TW; ++j) {
          const int c = w0 + j + (1 - kw) * d;
          if (w0 + j < a.W && c >= 0 && c < a.W) {
            float dyv[VEC];
            HVec<T>::load(DY + (rowbase + c) * a.lddy + c0, dyv);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
              g[j][i] = fmaf(dyv[i], wv[i], g[j][i]);
              accw[kh * 3 + kw][i] = fmaf(dyv[i], xa[j][i], accw[kh * 3 + kw][i]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < DW_TW; ++j) {
      if (w0 + j < a.W) {
        if (a.pro_mode & PRO_RELU) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const bool on = xa[j][i] > 0.f && (!(a.pro_mode & PRO_CLAMP6) || xa[j][i] < 6.f);
            g[j][i] = on ? g[j][i] : 0.f;
          }
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          s1[i] += g[j][i];
          s2[i] = fmaf(g[j][i], xr[j][i], s2[i]);
        }
        HVec<T>::store(G + (prow + w0 + j) * a.ldg + c0, g[j]);
      }
    }
  }
  // block reductions (LDS: [spb][cvb][3*VEC] reused): 9 taps in three rounds, then BN sums
#pragma unroll
  for (int k3 = 0; k3 < 4; ++k3) {
    if (k3 == 3 && a.partial_bn == nullptr) break;
    float* mine = dw_smem + ((long)sy * cvb + cx) * 3 * VEC;
#pragma unroll
    for (int kk = 0; kk < 3; ++kk)
#pragma unroll
      for (int i = 0; i < VEC; ++i)
        mine[kk * VEC + i] = k3 < 3 ? accw[(k3 < 3 ? k3 : 0) * 3 + kk][i]
                                    : (kk == 0 ? s1[i] : (kk == 1 ? s2[i] : 0.f));
    __syncthreads();
    const int ncol = (k3 < 3 ? 3 : 2) * VEC;
    for (int e = tid; e < cvb * 3 * VEC; e += DW_THREADS) {
      const int lcx = e / (3 * VEC), k = e % (3 * VEC);
      if (k >= ncol) continue;
      float tot = 0.f;
      for (int r = 0; r < spb; ++r) tot += dw_smem[(long)r * cvb * 3 * VEC + e];
      const int kk = k / VEC, ci = k % VEC;
      const int c = (blockIdx.x * cvb + lcx) * VEC + ci;
      if (c < a.C) {
        if (k3 < 3) a.partial_w[((long)blockIdx.y * 9 + k3 * 3 + kk) * a.C + c] = tot;
        else a.partial_bn[((long)blockIdx.y * 2 + kk) * a.C + c] = tot;
      }
    }
    __syncthreads();
  }
}

// strip launches: blocks along the channel vectors
static int strip_gx(int CV, int& cvb_log2) {
  cvb_log2 = rows_pick_cvb_log2(CV, 3);  // 32 / 16 / 8 channel vectors per block
  return rows_gx(CV, cvb_log2);
}

// The kernel family of a depthwise 3x3 launch: the ONLY statement of that policy in the library
// (the grid query and every launch entry switch on its result).  v = 8 channels bf16 / 4 fp32.
//
//   op                     stride  dil     family      C, pitches % ..   taps
//   forward (and stride-1  1       1       sliding     v                 torch [C,1,3,3] or [9][C]
//     data gradient:       1       2       tiled       v                 torch or [9][C]
//     reversed taps)       2       1       tiled s2    v                 torch or [9][C]
//                          1       3..64   row-chain   v                 [9][C]
//                          other           strip       v                 [9][C]
//   strided data gradient  any     any     strip       v                 [9][C]
//   fused backward         1       1       sliding     4                 torch or [9][C]
//                          1       2       tiled       v                 torch or [9][C]
//                          1       3..64   row-chain   v (C, lddy), 4    [9][C]
//                          1       > 64    strip       4                 [9][C]
//   ... with residual      1       1       sliding     v (ldr: 4)        torch or [9][C]
//       (sliding only, no other family adds one: with one rounding, or with the arithmetic of the
//       2-ary sum it replaces)
//   weight gradient        1       1, 2    tiled       v                 -
//                          other           strip       v                 -
//
// The sliding and row-chain families need C % 4 == 0; a launch without it falls to the strip row of
// its op and is refused by the entry's C % vec check (4 divides every vec) before anything runs.
// The tiled launchers refuse any dilation but 2 themselves.  (The stride-2 fused backward has its
// own entry point and kernel, dwconv_s2.hip: C and pitches % 4, torch taps.)
DwRoute dw_route(DwOp op, int dtype, int C, int stride, int dil) {
  const int v = dtype == DT_BF16 ? 8 : 4;
  const bool s1 = stride == 1 && op != DW_OP_DGRAD;
  DwFamily f = DW_STRIP;
  if (s1 && dil == 1 && C % 4 == 0 && op != DW_OP_WGRAD) f = DW_SLIDE;
  else if (s1 && (dil == 2 || (dil == 1 && op == DW_OP_WGRAD))) f = DW_TILED;
  else if (op == DW_OP_FWD && stride == 2 && dil == 1) f = DW_TILED_S2;
  else if (s1 && dil > 2 && dil <= 64 && C % 4 == 0 && op != DW_OP_WGRAD) f = DW_ROW;
  const bool narrow = op == DW_OP_BWD && (f == DW_SLIDE || f == DW_STRIP);  // HVec: 4 channels
  return {f, narrow ? 4 : v, f == DW_SLIDE || f == DW_TILED || f == DW_TILED_S2};
}

int dw_route_grid_y(DwRoute r, DwOp op, int dtype, int C, int N, int Ho, int Wo, int dil) {
  const int v = dtype == DT_BF16 ? 8 : 4;
  const bool fused = op == DW_OP_BWD || op == DW_OP_BWD_ADD;
  // the channel vector the family's geometry counts in
  const int gvec = (fused || r.family == DW_SLIDE || r.family == DW_ROW) ? 4 : v;
  if (N < 1 || Ho < 1 || Wo < 1 || C < gvec || C % gvec != 0) return -1;
  switch (r.family) {
    case DW_SLIDE: return dw_slide_rows(C, N, Ho, Wo);
    case DW_TILED:
      return dw_tiled_grid_y(dtype, C, N, Ho, Wo, fused ? 1 : op == DW_OP_WGRAD ? 2 : 0);
    case DW_TILED_S2: return dw_tiled_s2_grid_y(dtype, C, N, Ho, Wo);
    case DW_ROW: return dw_row_grid_y(dtype, C, N, Ho, Wo, dil);  // stride 1: the input size too
    case DW_STRIP: break;
  }
  if (C < v) return -1;  // (the strip geometry counts whole v-channel vectors for every op)
  int l;
  const int gx = strip_gx(C / v, l);
  const int spb = DW_THREADS >> l;
  const long strips = (long)N * Ho * ((Wo + DW_TW - 1) / DW_TW);
  long gy = (strips + spb - 1) / spb;
  long cap = 1536 / gx;  // ~6 blocks per CU; bounds the number of partial rows
  if (cap < 1) cap = 1;
  if (gy > cap) gy = cap;
  return (int)gy;
}

}  // namespace seg

// Number of partial rows / persistent blocks per channel block for one depthwise launch, or -1
// where there is no such launch (non-positive sizes, C not made of the family's channel vectors).
// kind: 0 forward / data gradient, 1 fused backward, 2 weight gradient.
extern "C" int seg_dwconv_grid_y(int dtype, int C, int N, int Ho, int Wo, int stride, int dil,
                                 int kind) {
  using namespace seg;
  static const DwOp ops[3] = {DW_OP_FWD, DW_OP_BWD, DW_OP_WGRAD};
  if ((dtype != DT_F32 && dtype != DT_BF16) || kind < 0 || kind > 2 || stride < 1 || dil < 1)
    return -1;
  return dw_route_grid_y(dw_route(ops[kind], dtype, C, stride, dil), ops[kind], dtype, C, N, Ho, Wo,
                         dil);
}

extern "C" int seg_dwconv3x3(int dtype, int mode, const void* x, long ldx, int N, int Hi, int Wi,
                             int C, const float* w9c, int w_layout, int stride, int dil, int pro_mode,
                             const float* pro_scale, const float* pro_shift, void* y, long ldy,
                             int Ho, int Wo, float* stat_partial, int grid_y, void* stream) {
  using namespace seg;
  SEG_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "dwconv3x3: bad dtype %d", dtype);
  const DwRoute r = dw_route(mode == MODE_FWD ? DW_OP_FWD : DW_OP_DGRAD, dtype, C, stride, dil);
  const int vec = r.vec;
  SEG_REQUIRE(C % vec == 0 && ldx % vec == 0 && ldy % vec == 0,
              "dwconv3x3: C/ldx/ldy must be multiples of %d", vec);
  SEG_REQUIRE(((pro_mode & PRO_AFFINE) == 0) || (pro_scale && pro_shift),
              "dwconv3x3: affine prologue without scale/shift");
  SEG_REQUIRE(mode == MODE_FWD || stat_partial == nullptr, "dwconv3x3: stats only in forward");
  SEG_REQUIRE(grid_y >= 1, "dwconv3x3: grid_y must be >= 1");
  SEG_REQUIRE(r.torch_taps || w_layout == 0,
              "dwconv3x3: the row-chain and strip kernels take tap-major [9][C] weights");
  hipStream_t st = (hipStream_t)stream;
  switch (r.family) {
    case DW_SLIDE:
    case DW_TILED:  // incl. the stride-1 data gradient (reversed taps)
    case DW_ROW:
      SEG_REQUIRE(Ho == Hi && Wo == Wi, "dwconv3x3: stride 1 keeps the size");
      if (r.family == DW_SLIDE)
        return launch_dw_slide_fwd(dtype, x, ldx, N, Hi, Wi, C, w9c, w_layout, pro_mode, pro_scale,
                                   pro_shift, y, ldy, stat_partial, grid_y, st);
      if (r.family == DW_TILED)
        return launch_dw_tiled(dtype, x, ldx, N, Hi, Wi, C, w9c, w_layout, dil, pro_mode, pro_scale,
                               pro_shift, y, ldy, stat_partial, grid_y, st);
      return launch_dw_row_fwd(dtype, x, ldx, N, Hi, Wi, C, w9c, dil, pro_mode, pro_scale, pro_shift,
                               y, ldy, stat_partial, grid_y, st);
    case DW_TILED_S2:
      SEG_REQUIRE(Ho == (Hi + 1) / 2 && Wo == (Wi + 1) / 2, "dwconv3x3: stride-2 output size");
      SEG_REQUIRE((long)N * Hi * Wi < (1L << 31), "dwconv3x3: tensor exceeds 32-bit pixel offsets");
      return launch_dw_tiled_s2(dtype, x, ldx, N, Hi, Wi, C, w9c, w_layout, pro_mode, pro_scale,
                                pro_shift, y, ldy, stat_partial, grid_y, st);
    case DW_STRIP: break;
  }
  DwArgs a;
  a.x = x; a.w = w9c; a.y = y; a.pro_scale = pro_scale; a.pro_shift = pro_shift;
  a.stat_partial = stat_partial; a.ldx = ldx; a.ldy = ldy;
  a.N = N; a.Hi = Hi; a.Wi = Wi; a.C = C; a.Ho = Ho; a.Wo = Wo;
  a.stride = stride; a.pad = dil; a.dil = dil; a.pro_mode = pro_mode;
  a.CV = C / vec;  // vec channels per thread
  a.strips = (long)N * Ho * ((Wo + DW_TW - 1) / DW_TW);
  const dim3 grid(strip_gx(a.CV, a.cvb_log2), grid_y);
  const size_t lds = stat_partial ? (size_t)DW_THREADS * 2 * vec * sizeof(float) : 0;
  SEG_REQUIRE_FAST_DIV("dwconv3x3", (long)N * Ho, (Wo + DW_TW - 1) / DW_TW);
  SEG_REQUIRE((long)N * Hi * Wi * ldx < (1L << 31), "dwconv3x3: tensor exceeds 32-bit offsets");
#define SEG_DW_LAUNCH(TT, MM) \
  hipLaunchKernelGGL((dwconv_kernel<TT, MM>), grid, dim3(DW_THREADS), lds, st, a)
  if (dtype == DT_BF16) {
    if (mode == MODE_FWD) SEG_DW_LAUNCH(bf16_t, MODE_FWD); else SEG_DW_LAUNCH(bf16_t, MODE_DGRAD);
  } else {
    if (mode == MODE_FWD) SEG_DW_LAUNCH(float, MODE_FWD); else SEG_DW_LAUNCH(float, MODE_DGRAD);
  }
#undef SEG_DW_LAUNCH
  return check_launch("dwconv3x3");
}

extern "C" int seg_dwconv3x3_wgrad(int dtype, const void* x, long ldx, int N, int Hi, int Wi,
                                   int C, const void* dy, long lddy, int Ho, int Wo, int stride,
                                   int dil, int pro_mode, const float* pro_scale,
                                   const float* pro_shift, float* partial, int grid_y,
                                   void* stream) {
  using namespace seg;
  SEG_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "dwconv3x3_wgrad: bad dtype %d", dtype);
  const DwRoute r = dw_route(DW_OP_WGRAD, dtype, C, stride, dil);
  const int vec = r.vec;
  SEG_REQUIRE(C % vec == 0 && ldx % vec == 0 && lddy % vec == 0,
              "dwconv3x3_wgrad: C/ldx/lddy must be multiples of %d", vec);
  SEG_REQUIRE(grid_y >= 1, "dwconv3x3_wgrad: grid_y must be >= 1");
  hipStream_t st = (hipStream_t)stream;
  if (r.family == DW_TILED) {
    SEG_REQUIRE(Ho == Hi && Wo == Wi, "dwconv3x3_wgrad: stride 1 keeps the size");
    return launch_dw_wgrad_tiled(dtype, x, ldx, N, Hi, Wi, C, dy, lddy, dil, pro_mode, pro_scale,
                                 pro_shift, partial, grid_y, st);
  }
  DwWgradArgs a;
  a.x = x; a.dy = dy; a.partial = partial; a.pro_scale = pro_scale; a.pro_shift = pro_shift;
  a.ldx = ldx; a.lddy = lddy; a.N = N; a.Hi = Hi; a.Wi = Wi; a.C = C; a.Ho = Ho; a.Wo = Wo;
  a.stride = stride; a.pad = dil; a.dil = dil; a.pro_mode = pro_mode;
  a.CV = C / vec;
  a.strips = (long)N * Ho * ((Wo + DW_TW - 1) / DW_TW);
  const dim3 grid(strip_gx(a.CV, a.cvb_log2), grid_y);
  const size_t lds = (size_t)DW_THREADS * 3 * vec * sizeof(float);
  SEG_REQUIRE_FAST_DIV("dwconv3x3_wgrad", (long)N * Ho, (Wo + DW_TW - 1) / DW_TW);
  SEG_LAUNCH_T(dwconv_wgrad_kernel, grid, dim3(DW_THREADS), lds, st, a);
  return check_launch("dwconv3x3_wgrad");
}

// Fused stride-1 backward: g = relu_mask(x) * dgrad(dy), partial_w [grid_y][9][C],
// partial_bn [grid_y][2][C] = (sum g, sum g*x_raw) (nullable).  x is the forward input (raw tensor
// + prologue), w9c the forward taps (not reversed).
// With `res` ([N,H,W,C], pitch ldr, element type of g; the _add entry): that tensor is added to the
// masked data gradient in the store path, g = relu_mask(x) * dgrad + res.  Dilation 1 only — the
// caller does a separate add otherwise (seg_dwconv3x3_bwd_fused_add_ok).
// res_mode 2 (the _sum entry): the masked data gradient is rounded to the storage type before
// `res` joins — the stored g of the launch without `res` followed by seg_sum_n, in one pass.
// Sliding family only (seg_dwconv3x3_bwd_fused_sum_ok).
namespace seg {
static int dw_bwd_fused(const char* name, int dtype, const void* dy, long lddy, const void* x,
                        long ldx, int N, int H, int W, int C, const float* w9c, int w_layout,
                        int dil, int pro_mode, const float* pro_scale, const float* pro_shift,
                        const void* res, long ldr, void* g, long ldg, float* partial_w,
                        float* partial_bn, int grid_y, hipStream_t st, int res_mode = 1) {
  const int vec = 4;  // HVec: 4 channels per thread in both element types
  SEG_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "%s: bad dtype %d", name, dtype);
  const DwRoute r = dw_route(res ? DW_OP_BWD_ADD : DW_OP_BWD, dtype, C, 1, dil);
  SEG_REQUIRE(C % vec == 0 && ldx % vec == 0 && lddy % vec == 0 && ldg % vec == 0 && ldr % vec == 0,
              "%s: C/ld must be multiples of %d", name, vec);
  SEG_REQUIRE(((pro_mode & PRO_AFFINE) == 0) || (pro_scale && pro_shift),
              "%s: affine prologue without scale/shift", name);
  SEG_REQUIRE(grid_y >= 1 && partial_w != nullptr, "%s: bad grid/partials", name);
  SEG_REQUIRE(r.torch_taps || w_layout == 0,
              "%s: the row-chain and strip kernels take tap-major [9][C] weights", name);
  // the row-chain kernel stages dy with 16-byte vectors (8 bf16 channels): a bf16 C = 4 (mod 8)
  // would read four channels past C (past the tensor on the last pixel), at 8-byte alignment;
  // its x and g move as 4-channel vectors: the common check above is all their pitches need
  SEG_REQUIRE(C % r.vec == 0 && lddy % r.vec == 0 &&
                  (r.family == DW_ROW || (ldx % r.vec == 0 && ldg % r.vec == 0)),
              "%s: C/ld must be multiples of %d", name, r.vec);
  SEG_REQUIRE(res_mode == 1 || r.family == DW_SLIDE,
              "%s: only the sliding kernels take residual mode %d", name, res_mode);
  switch (r.family) {
    case DW_SLIDE:
      return launch_dw_slide_bwd(dtype, dy, lddy, x, ldx, N, H, W, C, w9c, w_layout, pro_mode,
                                 pro_scale, pro_shift, g, ldg, partial_w, partial_bn, grid_y, st,
                                 res, ldr, res_mode);
    case DW_TILED:
      return launch_dw_bwd_tiled(dtype, dy, lddy, x, ldx, N, H, W, C, w9c, w_layout, dil, pro_mode,
                                 pro_scale, pro_shift, g, ldg, partial_w, partial_bn, grid_y, st);
    case DW_ROW:
      return launch_dw_row_bwd(dtype, dy, lddy, x, ldx, N, H, W, C, w9c, dil, pro_mode, pro_scale,
                               pro_shift, g, ldg, partial_w, partial_bn, grid_y, st);
    default: break;
  }
  DwBwdArgs a;
  a.dy = dy; a.x = x; a.g = g; a.w = w9c; a.pro_scale = pro_scale; a.pro_shift = pro_shift;
  a.partial_w = partial_w; a.partial_bn = partial_bn;
  a.lddy = lddy; a.ldx = ldx; a.ldg = ldg; a.N = N; a.H = H; a.W = W; a.C = C; a.dil = dil;
  a.pro_mode = pro_mode; a.CV = C / vec;
  a.strips = (long)N * H * ((W + DW_TW - 1) / DW_TW);
  SEG_REQUIRE_FAST_DIV(name, (long)N * H, (W + DW_TW - 1) / DW_TW);
  SEG_REQUIRE((long)N * H * W * lddy < (1L << 31), "%s: 32-bit offsets", name);
  const dim3 grid(strip_gx(a.CV, a.cvb_log2), grid_y);
  const size_t lds = (size_t)DW_THREADS * 3 * vec * sizeof(float);
  SEG_LAUNCH_T(dwconv_bwd_fused_kernel, grid, dim3(DW_THREADS), lds, st, a);
  return check_launch(name);
}
}  // namespace seg

extern "C" int seg_dwconv3x3_bwd_fused_add_ok(int dil) { return dil == 1 ? 1 : 0; }

extern "C" int seg_dwconv3x3_bwd_fused_add(int dtype, const void* dy, long lddy, const void* x,
                                           long ldx, int N, int H, int W, int C, const float* w9c,
                                           int w_layout, int pro_mode, const float* pro_scale,
                                           const float* pro_shift, const void* res, long ldr,
                                           void* g, long ldg, float* partial_w, float* partial_bn,
                                           int grid_y, void* stream) {
  SEG_REQUIRE(res != nullptr, "dwconv3x3_bwd_fused_add: C/ld must be multiples of %d, res non-null",
              dtype == seg::DT_BF16 ? 8 : 4);
  return seg::dw_bwd_fused("dwconv3x3_bwd_fused_add", dtype, dy, lddy, x, ldx, N, H, W, C, w9c,
                           w_layout, 1, pro_mode, pro_scale, pro_shift, res, ldr, g, ldg, partial_w,
                           partial_bn, grid_y, (hipStream_t)stream);
}

// Does a fused backward with a residual of C channels of `dtype` run on the sliding family — the
// one seg_dwconv3x3_bwd_fused_sum needs?  Pure host.
extern "C" int seg_dwconv3x3_bwd_fused_sum_ok(int dtype, int C, int dil) {
  using namespace seg;
  if ((dtype != DT_F32 && dtype != DT_BF16) || C < 1 || dil < 1) return 0;
  const DwRoute r = dw_route(DW_OP_BWD_ADD, dtype, C, 1, dil);
  return r.family == DW_SLIDE && C % r.vec == 0 ? 1 : 0;
}

// seg_dwconv3x3_bwd_fused_add with the masked gradient rounded to `dtype` before res joins: bit for
// bit seg_sum_n over the stored g of seg_dwconv3x3_bwd_fused and res, in one pass (fp32: the same
// values as the _add entry).
extern "C" int seg_dwconv3x3_bwd_fused_sum(int dtype, const void* dy, long lddy, const void* x,
                                           long ldx, int N, int H, int W, int C, const float* w9c,
                                           int w_layout, int pro_mode, const float* pro_scale,
                                           const float* pro_shift, const void* res, long ldr,
                                           void* g, long ldg, float* partial_w, float* partial_bn,
                                           int grid_y, void* stream) {
  SEG_REQUIRE(res != nullptr, "dwconv3x3_bwd_fused_sum: res must be non-null");
  return seg::dw_bwd_fused("dwconv3x3_bwd_fused_sum", dtype, dy, lddy, x, ldx, N, H, W, C, w9c,
                           w_layout, 1, pro_mode, pro_scale, pro_shift, res, ldr, g, ldg, partial_w,
                           partial_bn, grid_y, (hipStream_t)stream, 2);
}

extern "C" int seg_dwconv3x3_bwd_fused(int dtype, const void* dy, long lddy, const void* x,
                                       long ldx, int N, int H, int W, int C, const float* w9c,
                                       int w_layout, int dil, int pro_mode, const float* pro_scale,
                                       const float* pro_shift, void* g, long ldg,
                                       float* partial_w, float* partial_bn, int grid_y,
                                       void* stream) {
  return seg::dw_bwd_fused("dwconv3x3_bwd_fused", dtype, dy, lddy, x, ldx, N, H, W, C, w9c, w_layout,
                           dil, pro_mode, pro_scale, pro_shift, nullptr, 0, g, ldg, partial_w,
                           partial_bn, grid_y, (hipStream_t)stream);
}

// dW [C][9] (= torch [C,1,3,3]) from the weight-gradient partials [R][9][C]
extern "C" int seg_dwconv3x3_wgrad_finalize(const float* partial, int R, int C, float* dw_c9,
                                            void* stream) {
  using namespace seg;
  SEG_REQUIRE(R >= 1 && C >= 1, "dwconv3x3_wgrad_finalize: bad R/C");
  return launch_dw_wgrad_finalize(partial, R, C, dw_c9, (hipStream_t)stream);
}
