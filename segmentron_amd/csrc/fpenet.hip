// FPENet's FPE block and MEU module (segmentron/models/fpenet.py:150-247) on NHWC tensors: the
// operators the conv / BatchNorm machinery lacks.
//   seg_fpe_stage_fwd   one stage of the FPE pyramid: the depthwise 3x3 (pad = dilation = 1..8) of
//                       in = relu(sa*a + ta) + relu(sb*b + tb) on an n-channel slice, n a multiple of
//                       4: `a` is the stage's slice of conv1's raw output under bn1, `b` the previous
//                       stage's raw output under its own BatchNorm.  The sum is fp32 and never
//                       stored; the activated b at the centre tap goes out as a side output (the
//                       previous stage's slice of the concat conv3 reads) and the BatchNorm
//                       statistic rows of the fp32 outputs come from the same pass.
//   seg_fpe_act_fwd     relu(sb*b + tb) alone on such a slice: the last stage's slice of the concat
//                       (seg_bn_apply needs 8-channel vectors in bf16).
//   seg_fpe_stage_bwd   one pass over (dy, a, b, res): both masked data gradients, the weight-gradient
//                       rows and the BatchNorm-backward rows of bn1 (its column slice) and of the
//                       previous stage's BatchNorm.  dy null: the last stage's slice, where only
//                       gb = mask(b) * res and its rows exist.
//   seg_fpe_bn_bwd_apply dx = scale*g - c0 - c1*x on such a slice (the affine part of the BatchNorm
//                       backward; seg_bn_bwd_apply needs 8-channel vectors in bf16).
//   seg_meu_fwd         out = a[n][c]*(sl*L + tl) + sa[p]*(sh*bilinear(Hraw) + th) with
//                       sa[p] = sigmoid(w_sa * mean_c(sl*L + tl)), align_corners bilinear.
//   seg_meu_bwd_low     the gradient at bn_low's output and the rows of da, d w_sa and bn_low.
//   seg_meu_bwd_high    the gradient at bn_high's output, a gather, and bn_high's rows.
// All use the launch geometry of rows.h with 4-channel vectors (16 B of fp32, 8 B of bf16): no
// atomics, fp32 partial rows per (chunk, image) summed in index order, the same bits on every launch,
// and an image never reaches another image's outputs or partial rows.
#include "cgn_rows.h"
#include "resize_taps.h"

namespace seg {

constexpr int FPE_V = 4;
constexpr int FPE_MAX_N = 64;
constexpr int FPE_MAX_DIL = 8;
constexpr int MEU_MAX_C = 128;

// ------------------------------------------------------------------------------- stage forward
struct FpeFwdArgs {
  const void* a; const void* b; void* y; void* b_act;
  const float* w;  // [n][9]: the [n,1,3,3] parameter as it is
  const float* sa; const float* ta; const float* sb; const float* tb;
  float* partial;
  long lda, ldb, ldy, ldo, per;
  int N, H, W, n, CV, cvb_log2, dil;
};

template <typename T, bool HAS_B>
__global__ __launch_bounds__(CGN_THREADS) void fpe_stage_fwd_kernel(const FpeFwdArgs a) {
  constexpr int V = FPE_V;
  __shared__ __attribute__((aligned(16))) float smem[2 * CGN_THREADS * V];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2, spb = CGN_THREADS >> a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int cv = blockIdx.x * cvb + cx;
  const int img = blockIdx.z;
  float acc[2][V];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int e = 0; e < V; ++e) acc[k][e] = 0.f;
  if (cv < a.CV) {
    const int c0 = cv * V;
    float wk[9][V], sa[V], ta[V], sb[V], tb[V];
#pragma unroll
    for (int e = 0; e < V; ++e)
#pragma unroll
      for (int k = 0; k < 9; ++k) wk[k][e] = a.w[(long)(c0 + e) * 9 + k];
    cgn_params<V>(a.sa, 0, c0, a.n, 1.f, sa);
    cgn_params<V>(a.ta, 0, c0, a.n, 0.f, ta);
    cgn_params<V>(a.sb, 0, c0, a.n, 1.f, sb);
    cgn_params<V>(a.tb, 0, c0, a.n, 0.f, tb);
    const long HW = (long)a.H * a.W;
    const T* __restrict__ A = reinterpret_cast<const T*>(a.a) + (long)img * HW * a.lda + c0;
    const T* __restrict__ B =
        HAS_B ? reinterpret_cast<const T*>(a.b) + (long)img * HW * a.ldb + c0 : nullptr;
    T* __restrict__ Y = reinterpret_cast<T*>(a.y) + (long)img * HW * a.ldy + c0;
    T* __restrict__ O = (HAS_B && a.b_act != nullptr)
                            ? reinterpret_cast<T*>(a.b_act) + (long)img * HW * a.ldo + c0
                            : nullptr;
    const long q0 = (long)blockIdx.y * a.per;
    const long q1 = q0 + a.per < HW ? q0 + a.per : HW;
    for (long q = q0 + sy; q < q1; q += spb) {
      const int h = (int)(q / a.W), w = (int)(q - (long)h * a.W);
      float o[V];
#pragma unroll
      for (int e = 0; e < V; ++e) o[e] = 0.f;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int hh = h + (kh - 1) * a.dil, ww = w + (kw - 1) * a.dil;
          const bool in = (unsigned)hh < (unsigned)a.H && (unsigned)ww < (unsigned)a.W;
          const long p = in ? (long)hh * a.W + ww : q;  // (always a valid address; masked below)
          float fa[V], v[V];
          HVec<T>::load(A + p * a.lda, fa);
#pragma unroll
          for (int e = 0; e < V; ++e) v[e] = fmaxf(fmaf(fa[e], sa[e], ta[e]), 0.f);
          if (HAS_B) {
            float fb[V];
            HVec<T>::load(B + p * a.ldb, fb);
#pragma unroll
            for (int e = 0; e < V; ++e) fb[e] = fmaxf(fmaf(fb[e], sb[e], tb[e]), 0.f);
            if (kh == 1 && kw == 1 && O != nullptr) HVec<T>::store(O + q * a.ldo, fb);
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] += fb[e];
          }
#pragma unroll
          for (int e = 0; e < V; ++e) o[e] = fmaf(wk[kh * 3 + kw][e], in ? v[e] : 0.f, o[e]);
        }
      HVec<T>::store(Y + q * a.ldy, o);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        acc[0][e] += o[e];
        acc[1][e] = fmaf(o[e], o[e], acc[1][e]);
      }
    }
  }
  if (a.partial != nullptr)
    rows_block_reduce<V, 2>(smem, acc, a.cvb_log2, blockIdx.x, a.n,
                            a.partial + ((long)blockIdx.y * a.N + img) * 2 * a.n, a.n);
}

// ------------------------------------------------------------------------------- flat slice passes
struct FpeFlatArgs {
  const void* x; const void* g; void* y;
  const float* s; const float* t; const float* c0; const float* c1;
  long ldx, ldg, ldy, total;
  int n, CV;
};

// BWD false: y = relu(s*x + t);  BWD true: y = s*g - c0 - c1*x (c0 / c1 null: y = s*g)
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void fpe_flat_kernel(const FpeFlatArgs a) {
  constexpr int V = FPE_V;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  const long row = i / a.CV;
  const int c0 = (int)(i - row * a.CV) * V;
  float s[V], t[V], k0[V], k1[V], fx[V], fg[V];
  cgn_params<V>(a.s, 0, c0, a.n, 1.f, s);
  cgn_params<V>(a.t, 0, c0, a.n, 0.f, t);
  HVec<T>::load(reinterpret_cast<const T*>(a.x) + row * a.ldx + c0, fx);
  if (BWD) {
    cgn_params<V>(a.c0, 0, c0, a.n, 0.f, k0);
    cgn_params<V>(a.c1, 0, c0, a.n, 0.f, k1);
    HVec<T>::load(reinterpret_cast<const T*>(a.g) + row * a.ldg + c0, fg);
#pragma unroll
    for (int e = 0; e < V; ++e) fx[e] = s[e] * fg[e] - k0[e] - k1[e] * fx[e];
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) fx[e] = fmaxf(fmaf(fx[e], s[e], t[e]), 0.f);
  }
  HVec<T>::store(reinterpret_cast<T*>(a.y) + row * a.ldy + c0, fx);
}

// ------------------------------------------------------------------------------- stage backward
struct FpeBwdArgs {
  const void* dy; const void* a; const void* b; const void* res; void* ga; void* gb;
  const float* w; const float* sa; const float* ta; const float* sb; const float* tb;
  float* pw; float* pa; float* pb;
  long lddy, lda, ldb, ldres, ldga, ldgb, per, pa_pitch;
  int N, H, W, n, CV, cvb_log2, dil, pa_col;
};

// MODE 0: stage 0 (no b);  1: a stage with b;  2: the last stage's slice (b and res only)
template <typename T, int MODE>
__global__ __launch_bounds__(CGN_THREADS) void fpe_stage_bwd_kernel(const FpeBwdArgs a) {
  constexpr int V = FPE_V;
  constexpr int KW = MODE == 2 ? 2 : 9;
  __shared__ __attribute__((aligned(16))) float smem[KW * CGN_THREADS * V];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2, spb = CGN_THREADS >> a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int cv = blockIdx.x * cvb + cx;
  const int img = blockIdx.z;
  float aw[9][V], apa[2][V], apb[2][V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
#pragma unroll
    for (int k = 0; k < 9; ++k) aw[k][e] = 0.f;
    apa[0][e] = apa[1][e] = apb[0][e] = apb[1][e] = 0.f;
  }
  if (cv < a.CV) {
    const int c0 = cv * V;
    float wk[9][V], sa[V], ta[V], sb[V], tb[V];
    if (MODE != 2) {
#pragma unroll
      for (int e = 0; e < V; ++e)
#pragma unroll
        for (int k = 0; k < 9; ++k) wk[k][e] = a.w[(long)(c0 + e) * 9 + k];
    }
    cgn_params<V>(a.sa, 0, c0, a.n, 1.f, sa);
    cgn_params<V>(a.ta, 0, c0, a.n, 0.f, ta);
    cgn_params<V>(a.sb, 0, c0, a.n, 1.f, sb);
    cgn_params<V>(a.tb, 0, c0, a.n, 0.f, tb);
    const long HW = (long)a.H * a.W;
    const long base = (long)img * HW;
    const T* __restrict__ DY =
        MODE != 2 ? reinterpret_cast<const T*>(a.dy) + base * a.lddy + c0 : nullptr;
    const T* __restrict__ A =
        MODE != 2 ? reinterpret_cast<const T*>(a.a) + base * a.lda + c0 : nullptr;
    T* __restrict__ GA = MODE != 2 ? reinterpret_cast<T*>(a.ga) + base * a.ldga + c0 : nullptr;
    const T* __restrict__ B =
        MODE != 0 ? reinterpret_cast<const T*>(a.b) + base * a.ldb + c0 : nullptr;
    const T* __restrict__ R =
        MODE != 0 ? reinterpret_cast<const T*>(a.res) + base * a.ldres + c0 : nullptr;
    T* __restrict__ GB = MODE != 0 ? reinterpret_cast<T*>(a.gb) + base * a.ldgb + c0 : nullptr;
    const long q0 = (long)blockIdx.y * a.per;
    const long q1 = q0 + a.per < HW ? q0 + a.per : HW;
    for (long q = q0 + sy; q < q1; q += spb) {
      const int h = (int)(q / a.W), w = (int)(q - (long)h * a.W);
      float fa[V], za[V], fb[V], zb[V], in[V], dg[V];
#pragma unroll
      for (int e = 0; e < V; ++e) in[e] = dg[e] = 0.f;
      if (MODE != 2) {
        HVec<T>::load(A + q * a.lda, fa);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          za[e] = fmaf(fa[e], sa[e], ta[e]);
          in[e] = fmaxf(za[e], 0.f);
        }
      }
      if (MODE != 0) {
        HVec<T>::load(B + q * a.ldb, fb);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          zb[e] = fmaf(fb[e], sb[e], tb[e]);
          in[e] += fmaxf(zb[e], 0.f);
        }
      }
      if (MODE != 2) {
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            // t_k = dy[p - d_k]: the output pixel that read `in` at p through tap k
            float t[V];
            cgn_tap<T>(DY, a.lddy, a.H, a.W, h - (kh - 1) * a.dil, w - (kw - 1) * a.dil, t);
#pragma unroll
            for (int e = 0; e < V; ++e) {
              dg[e] = fmaf(t[e], wk[kh * 3 + kw][e], dg[e]);
              aw[kh * 3 + kw][e] = fmaf(t[e], in[e], aw[kh * 3 + kw][e]);
            }
          }
        float g[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          g[e] = za[e] > 0.f ? dg[e] : 0.f;
          apa[0][e] += g[e];
          apa[1][e] = fmaf(g[e], fa[e], apa[1][e]);
        }
        HVec<T>::store(GA + q * a.ldga, g);
      }
      if (MODE != 0) {
        float r[V], g[V];
        HVec<T>::load(R + q * a.ldres, r);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          g[e] = zb[e] > 0.f ? dg[e] + r[e] : 0.f;
          apb[0][e] += g[e];
          apb[1][e] = fmaf(g[e], fb[e], apb[1][e]);
        }
        HVec<T>::store(GB + q * a.ldgb, g);
      }
    }
  }
  const long row = (long)blockIdx.y * a.N + img;
  if (MODE != 2) {
    rows_block_reduce<V, 9>(smem, aw, a.cvb_log2, blockIdx.x, a.n, a.pw + row * 9 * a.n, a.n);
    rows_block_reduce<V, 2>(smem, apa, a.cvb_log2, blockIdx.x, a.n,
                            a.pa + row * 2 * a.pa_pitch + a.pa_col, a.pa_pitch);
  }
  if (MODE != 0) rows_block_reduce<V, 2>(smem, apb, a.cvb_log2, blockIdx.x, a.n,
                                         a.pb + row * 2 * a.n, a.n);
}

// ------------------------------------------------------------------------------- MEU
struct MeuArgs {
  const void* L; const void* Hr; const void* g; void* out;
  const float* a; const float* sl; const float* tl; const float* sh; const float* th;
  const float* wsa; const float* dpool;
  float* sa;
  float* p1; float* p2;
  long ldl, ldh, ldg, ldo, per;
  float scale_h, scale_w, inv_c, inv_hw2;
  int N, h, w, h2, w2, C, CV, cvb_log2;
};

// sum over the 2^l lanes that share a pixel (an aligned lane group of the wave): every lane of the
// group ends with the same value
__device__ __forceinline__ float meu_group_sum(float v, int l) {
  for (int o = (1 << l) >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sh * bilinear(Hraw) + th at output pixel (ho, wo): the affine commutes with the interpolation
template <typename T>
__device__ __forceinline__ void meu_high_up(const T* __restrict__ Himg, const MeuArgs& a, int ho,
                                            int wo, const float* sh, const float* th, float* up) {
  constexpr int V = FPE_V;
  int i0, i1, j0, j1;
  float lh, lw;
  taps(a.scale_h, ho, a.h2, 1, i0, i1, lh);
  taps(a.scale_w, wo, a.w2, 1, j0, j1, lw);
  float f00[V], f01[V], f10[V], f11[V];
  HVec<T>::load(Himg + ((long)i0 * a.w2 + j0) * a.ldh, f00);
  HVec<T>::load(Himg + ((long)i0 * a.w2 + j1) * a.ldh, f01);
  HVec<T>::load(Himg + ((long)i1 * a.w2 + j0) * a.ldh, f10);
  HVec<T>::load(Himg + ((long)i1 * a.w2 + j1) * a.ldh, f11);
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const float top = (1.f - lw) * f00[e] + lw * f01[e];
    const float bot = (1.f - lw) * f10[e] + lw * f11[e];
    up[e] = fmaf((1.f - lh) * top + lh * bot, sh[e], th[e]);
  }
}

// grid (1, chunks, N): the 2^cvb_log2 >= C/4 lanes of a block row hold ONE pixel's channels
// BWD false: out and sa;  BWD true: out = dL (at bn_low's output), p1 = rows (sum g*Lbn | d w_sa in
// column 0), p2 = rows (sum dL | sum dL*L)
template <typename T, bool BWD>
__global__ __launch_bounds__(CGN_THREADS) void meu_low_kernel(const MeuArgs a) {
  constexpr int V = FPE_V;
  __shared__ __attribute__((aligned(16))) float smem[2 * CGN_THREADS * V];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2, spb = CGN_THREADS >> a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int img = blockIdx.z;
  const bool live = cx < a.CV;
  const int c0 = live ? cx * V : 0;
  float sl[V], tl[V], sh[V], th[V], av[V];
  cgn_params<V>(a.sl, 0, c0, a.C, 1.f, sl);
  cgn_params<V>(a.tl, 0, c0, a.C, 0.f, tl);
  cgn_params<V>(a.sh, 0, c0, a.C, 1.f, sh);
  cgn_params<V>(a.th, 0, c0, a.C, 0.f, th);
  cgn_params<V>(a.a, (long)img * a.C, c0, a.C, 0.f, av);
  const float wsa = a.wsa[0];
  const long hw = (long)a.h * a.w;
  const T* __restrict__ Limg = reinterpret_cast<const T*>(a.L) + (long)img * hw * a.ldl + c0;
  const T* __restrict__ Himg =
      reinterpret_cast<const T*>(a.Hr) + (long)img * a.h2 * a.w2 * a.ldh + c0;
  const T* __restrict__ Gimg =
      BWD ? reinterpret_cast<const T*>(a.g) + (long)img * hw * a.ldg + c0 : nullptr;
  T* __restrict__ Oimg = reinterpret_cast<T*>(a.out) + (long)img * hw * a.ldo + c0;
  float* __restrict__ SA = a.sa + (long)img * hw;
  float acc1[2][V], acc2[2][V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc1[0][e] = acc1[1][e] = acc2[0][e] = acc2[1][e] = 0.f;
  const long q0 = (long)blockIdx.y * a.per;
  const long q1 = q0 + a.per < hw ? q0 + a.per : hw;
  // (a uniform trip count: every lane of a wave takes part in the group sums)
  for (long qb = q0; qb < q1; qb += spb) {
    const bool ok = qb + sy < q1;
    const bool on = ok && live;
    const long q = ok ? qb + sy : q0;  // (always a valid address)
    const int ho = (int)(q / a.w), wo = (int)(q - (long)ho * a.w);
    float l[V], lbn[V], up[V], g[V];
    HVec<T>::load(Limg + q * a.ldl, l);
#pragma unroll
    for (int e = 0; e < V; ++e) lbn[e] = on ? fmaf(l[e], sl[e], tl[e]) : 0.f;
    const float m = meu_group_sum((lbn[0] + lbn[1]) + (lbn[2] + lbn[3]), a.cvb_log2) * a.inv_c;
    meu_high_up<T>(Himg, a, ho, wo, sh, th, up);
    if (!BWD) {
      const float sg = 1.f / (1.f + expf(-(wsa * m)));
      if (on) {
        float o[V];
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = av[e] * lbn[e] + sg * up[e];
        HVec<T>::store(Oimg + q * a.ldo, o);
        if (cx == 0) SA[q] = sg;
      }
    } else {
      HVec<T>::load(Gimg + q * a.ldg, g);
#pragma unroll
      for (int e = 0; e < V; ++e) g[e] = on ? g[e] : 0.f;
      const float S = meu_group_sum((g[0] * up[0] + g[1] * up[1]) + (g[2] * up[2] + g[3] * up[3]),
                                    a.cvb_log2);
      const float sg = SA[q];
      const float ds = sg * (1.f - sg);
      const float common = wsa * ds * a.inv_c * S;
      if (on) {
        float d[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          d[e] = av[e] * g[e] + common;
          acc1[0][e] = fmaf(g[e], lbn[e], acc1[0][e]);
          acc2[0][e] += d[e];
          acc2[1][e] = fmaf(d[e], l[e], acc2[1][e]);
        }
        if (cx == 0) acc1[1][0] = fmaf(ds * m, S, acc1[1][0]);
        HVec<T>::store(Oimg + q * a.ldo, d);
      }
    }
  }
  if (BWD) {
    const long row = (long)blockIdx.y * a.N + img;
    rows_block_reduce<V, 2>(smem, acc1, a.cvb_log2, blockIdx.x, a.C, a.p1 + row * 2 * a.C, a.C);
    rows_block_reduce<V, 2>(smem, acc2, a.cvb_log2, blockIdx.x, a.C, a.p2 + row * 2 * a.C, a.C);
  }
}

// dH[q][c] = sum_p wgt(p, q) * sa[p] * g[p][c] + dpool[n][c] / (h2*w2): every dH written once;
// p2 = rows (sum dH | sum dH*Hraw).  grid (channel-vector blocks, chunks over h2*w2, N).
template <typename T>
__global__ __launch_bounds__(CGN_THREADS) void meu_high_bwd_kernel(const MeuArgs a) {
  constexpr int V = FPE_V;
  __shared__ __attribute__((aligned(16))) float smem[2 * CGN_THREADS * V];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2, spb = CGN_THREADS >> a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int cv = blockIdx.x * cvb + cx;
  const int img = blockIdx.z;
  float acc[2][V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[0][e] = acc[1][e] = 0.f;
  if (cv < a.CV) {
    const int c0 = cv * V;
    const long hw = (long)a.h * a.w, hw2 = (long)a.h2 * a.w2;
    float dp[V];
    cgn_params<V>(a.dpool, (long)img * a.C, c0, a.C, 0.f, dp);
#pragma unroll
    for (int e = 0; e < V; ++e) dp[e] *= a.inv_hw2;
    const T* __restrict__ Gimg = reinterpret_cast<const T*>(a.g) + (long)img * hw * a.ldg + c0;
    const T* __restrict__ Himg = reinterpret_cast<const T*>(a.Hr) + (long)img * hw2 * a.ldh + c0;
    T* __restrict__ Oimg = reinterpret_cast<T*>(a.out) + (long)img * hw2 * a.ldo + c0;
    const float* __restrict__ SA = a.sa + (long)img * hw;
    const long q0 = (long)blockIdx.y * a.per;
    const long q1 = q0 + a.per < hw2 ? q0 + a.per : hw2;
    for (long q = q0 + sy; q < q1; q += spb) {
      const int qh = (int)(q / a.w2), qw = (int)(q - (long)qh * a.w2);
      int lo_h, hi_h, lo_w, hi_w;
      cand_range(a.scale_h, qh, a.h, 1, lo_h, hi_h);
      cand_range(a.scale_w, qw, a.w, 1, lo_w, hi_w);
      float d[V];
#pragma unroll
      for (int e = 0; e < V; ++e) d[e] = 0.f;
      for (int ho = lo_h; ho <= hi_h; ++ho) {
        const float wy = tap_weight(a.scale_h, ho, a.h2, 1, qh);
        if (wy == 0.f) continue;
        for (int wo = lo_w; wo <= hi_w; ++wo) {
          const float wx = tap_weight(a.scale_w, wo, a.w2, 1, qw);
          if (wx == 0.f) continue;
          const long p = (long)ho * a.w + wo;
          const float k = wy * wx * SA[p];
          float g[V];
          HVec<T>::load(Gimg + p * a.ldg, g);
#pragma unroll
          for (int e = 0; e < V; ++e) d[e] = fmaf(k, g[e], d[e]);
        }
      }
      float hr[V];
      HVec<T>::load(Himg + q * a.ldh, hr);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        d[e] += dp[e];
        acc[0][e] += d[e];
        acc[1][e] = fmaf(d[e], hr[e], acc[1][e]);
      }
      HVec<T>::store(Oimg + q * a.ldo, d);
    }
  }
  rows_block_reduce<V, 2>(smem, acc, a.cvb_log2, blockIdx.x, a.C,
                          a.p2 + ((long)blockIdx.y * a.N + img) * 2 * a.C, a.C);
}

// ------------------------------------------------------------------------------- host side
// chunks per image: about 2048 blocks, at least one block row of pixels per chunk, at most 256
static int fpe_chunks(int N, long HW, int CV, int cvb_log2) {
  return rows_chunks(N, rows_gx(CV, cvb_log2), HW, CGN_THREADS >> cvb_log2, 2048, CGN_MAX_CHUNKS);
}

static int fpe_rows_ok(const char* what, int rows, int N, int* chunks) {
  SEG_REQUIRE(N >= 1 && rows >= N && rows % N == 0 && rows / N <= CGN_MAX_CHUNKS,
              "%s: %d partial rows are not 1..%d chunks of %d images", what, rows, CGN_MAX_CHUNKS, N);
  *chunks = rows / N;
  return 0;
}

// the `nld` pitches hold n channels in whole 4-channel vectors; rows -> chunks
static int fpe_geometry(const char* what, int dtype, int N, int H, int W, int n, int dil, int rows,
                        const long* lds, int nld, int* chunks) {
  SEG_REQUIRE(H >= 1 && W >= 1 && (long)H * W < (1L << 31), "%s: bad shape H=%d W=%d", what, H, W);
  SEG_REQUIRE(n <= FPE_MAX_N, "%s: n=%d is not a positive multiple of 4 up to %d", what, n,
              FPE_MAX_N);
  SEG_REQUIRE(dil >= 1 && dil <= FPE_MAX_DIL, "%s: dilation %d not in 1..%d", what, dil,
              FPE_MAX_DIL);
  if (fpe_rows_ok(what, rows, N, chunks)) return 1;
  return rows_require(what, dtype, N, (long)H * W, n, FPE_V, FPE_V, lds, nullptr, nld, *chunks,
                      CGN_MAX_CHUNKS);
}

// C a multiple of 8 (the low kernels' lane groups), pitches in whole 4-channel vectors
static int meu_geometry(const char* what, int dtype, int N, int h, int w, int h2, int w2, int C,
                        const long* lds, int nld, int chunks) {
  SEG_REQUIRE(C <= MEU_MAX_C, "%s: C=%d is not a positive multiple of 8 up to %d", what, C,
              MEU_MAX_C);
  SEG_REQUIRE(h >= 1 && w >= 1 && h2 >= 1 && w2 >= 1 && h2 <= h && w2 <= w &&
                  (long)h * w < (1L << 31),
              "%s: bad shape low %dx%d high %dx%d (1 <= high <= low)", what, h, w, h2, w2);
  return rows_require(what, dtype, N, (long)h * w, C, 8, FPE_V, lds, nullptr, nld, chunks,
                      CGN_MAX_CHUNKS);
}

static void meu_fill(MeuArgs* a, int N, int h, int w, int h2, int w2, int C) {
  a->N = N; a->h = h; a->w = w; a->h2 = h2; a->w2 = w2; a->C = C; a->CV = C / FPE_V;
  a->scale_h = host_scale(h2, h, 1); a->scale_w = host_scale(w2, w, 1);
  a->inv_c = 1.f / (float)C;
  a->inv_hw2 = 1.f / (float)((long)h2 * w2);
}

}  // namespace seg

// rows of the partial arrays of seg_fpe_stage_fwd / _bwd: chunks * N (-1: out of contract)
extern "C" int seg_fpe_stage_rows(int dtype, int N, int H, int W, int n) {
  using namespace seg;
  if ((dtype != DT_F32 && dtype != DT_BF16) || N < 1 || N > 65535 || H < 1 || W < 1 || n < 4 ||
      n % 4 != 0 || n > FPE_MAX_N)
    return -1;
  const int CV = n / FPE_V;
  return fpe_chunks(N, (long)H * W, CV, rows_pick_cvb_log2(CV, 0)) * N;
}

extern "C" int seg_fpe_stage_fwd(int dtype, const void* a_, long lda, const float* sa,
                                 const float* ta, const void* b, long ldb, const float* sb,
                                 const float* tb, const float* w, int dil, void* y, long ldy,
                                 void* b_act, long ldo, int N, int H, int W, int n, float* partial,
                                 int rows, void* stream) {
  using namespace seg;
  int chunks;
  // (a's pitch stands in for an absent operand's)
  const long lds[4] = {lda, ldy, b != nullptr ? ldb : lda, b_act != nullptr ? ldo : lda};
  if (fpe_geometry("fpe_stage_fwd", dtype, N, H, W, n, dil, rows, lds, 4, &chunks)) return 1;
  SEG_REQUIRE(a_ != nullptr && sa != nullptr && ta != nullptr && w != nullptr && y != nullptr,
              "fpe_stage_fwd: null a / sa / ta / w / y");
  SEG_REQUIRE(b == nullptr ? b_act == nullptr : (sb != nullptr && tb != nullptr),
              "fpe_stage_fwd: b needs sb / tb (b_act needs b)");
  FpeFwdArgs a = FpeFwdArgs();
  a.a = a_; a.lda = lda; a.sa = sa; a.ta = ta; a.b = b; a.ldb = ldb; a.sb = sb; a.tb = tb;
  a.w = w; a.dil = dil; a.y = y; a.ldy = ldy; a.b_act = b_act; a.ldo = ldo; a.partial = partial;
  a.N = N; a.H = H; a.W = W; a.n = n; a.CV = n / FPE_V; a.cvb_log2 = rows_pick_cvb_log2(a.CV, 0);
  a.per = rows_per((long)H * W, chunks, a.cvb_log2);
  const dim3 grid = rows_grid(a.CV, a.cvb_log2, chunks, N);
  if (b != nullptr)
    SEG_LAUNCH_T((fpe_stage_fwd_kernel, true), grid, dim3(CGN_THREADS), 0, stream, a);
  else
    SEG_LAUNCH_T((fpe_stage_fwd_kernel, false), grid, dim3(CGN_THREADS), 0, stream, a);
  return check_launch("fpe_stage_fwd");
}

static int fpe_flat(const char* what, bool bwd, int dtype, const void* g, long ldg, const void* x,
                    long ldx, const float* s, const float* t, const float* c0, const float* c1,
                    void* y, long ldy, long rows, int n, void* stream) {
  using namespace seg;
  SEG_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "%s: bad dtype %d", what, dtype);
  SEG_REQUIRE(rows >= 1 && n >= 4 && n % 4 == 0, "%s: bad shape rows=%ld n=%d (a multiple of 4)",
              what, rows, n);
  SEG_REQUIRE(x != nullptr && y != nullptr && s != nullptr && (bwd ? g != nullptr : t != nullptr),
              "%s: null operand", what);
  SEG_REQUIRE(ldx % 4 == 0 && ldx >= n && ldy % 4 == 0 && ldy >= n &&
                  (!bwd || (ldg % 4 == 0 && ldg >= n)),
              "%s: a pitch is not a multiple of 4 or below n", what);
  SEG_REQUIRE((c0 == nullptr) == (c1 == nullptr), "%s: c0 and c1 go together", what);
  FpeFlatArgs a = FpeFlatArgs();
  a.x = x; a.ldx = ldx; a.g = g; a.ldg = ldg; a.y = y; a.ldy = ldy; a.s = s; a.t = t;
  a.c0 = c0; a.c1 = c1; a.n = n; a.CV = n / FPE_V; a.total = rows * a.CV;
  SEG_REQUIRE((a.total + 255) / 256 < (1L << 31), "%s: too large", what);
  const dim3 grid((unsigned)((a.total + 255) / 256));
  if (bwd)
    SEG_LAUNCH_T((fpe_flat_kernel, true), grid, dim3(256), 0, stream, a);
  else
    SEG_LAUNCH_T((fpe_flat_kernel, false), grid, dim3(256), 0, stream, a);
  return check_launch(what);
}

extern "C" int seg_fpe_act_fwd(int dtype, const void* b, long ldb, const float* sb, const float* tb,
                               void* y, long ldy, long rows, int n, void* stream) {
  return fpe_flat("fpe_act_fwd", false, dtype, nullptr, 0, b, ldb, sb, tb, nullptr, nullptr, y, ldy,
                  rows, n, stream);
}

extern "C" int seg_fpe_bn_bwd_apply(int dtype, const void* g, long ldg, const void* x, long ldx,
                                    const float* scale, const float* c0, const float* c1, void* dx,
                                    long lddx, long rows, int n, void* stream) {
  return fpe_flat("fpe_bn_bwd_apply", true, dtype, g, ldg, x, ldx, scale, nullptr, c0, c1, dx, lddx,
                  rows, n, stream);
}

extern "C" int seg_fpe_stage_bwd(int dtype, const void* dy, long lddy, const void* a_, long lda,
                                 const float* sa, const float* ta, const void* b, long ldb,
                                 const float* sb, const float* tb, const void* res, long ldres,
                                 const float* w, int dil, void* ga, long ldga, void* gb, long ldgb,
                                 int N, int H, int W, int n, float* pw, float* pa, long pa_pitch,
                                 int pa_col, float* pb, int rows, void* stream) {
  using namespace seg;
  const bool tail = dy == nullptr, has_b = b != nullptr;
  SEG_REQUIRE(!tail || has_b, "fpe_stage_bwd: neither dy nor b");
  int chunks;
  const long any = tail ? ldb : lda;  // (a present operand's pitch stands in for an absent one's)
  const long lds[6] = {tail ? any : lddy, tail ? any : lda, tail ? any : ldga,
                       has_b ? ldb : any, has_b ? ldres : any, has_b ? ldgb : any};
  if (fpe_geometry("fpe_stage_bwd", dtype, N, H, W, n, dil, rows, lds, 6, &chunks)) return 1;
  if (!tail) {
    SEG_REQUIRE(a_ != nullptr && sa != nullptr && ta != nullptr && w != nullptr && ga != nullptr &&
                    pw != nullptr && pa != nullptr,
                "fpe_stage_bwd: null a / sa / ta / w / ga / pw / pa");
    SEG_REQUIRE(pa_col >= 0 && pa_col % 4 == 0 && pa_pitch >= (long)pa_col + n,
                "fpe_stage_bwd: partial_a column %d + %d beyond its pitch %ld", pa_col, n, pa_pitch);
  }
  SEG_REQUIRE(has_b == (res != nullptr) && has_b == (gb != nullptr) && has_b == (pb != nullptr),
              "fpe_stage_bwd: b, res, gb and partial_b are null together");
  SEG_REQUIRE(!has_b || (sb != nullptr && tb != nullptr), "fpe_stage_bwd: b needs sb / tb");
  FpeBwdArgs a = FpeBwdArgs();
  a.dy = dy; a.lddy = lddy; a.a = a_; a.lda = lda; a.sa = sa; a.ta = ta;
  a.b = b; a.ldb = ldb; a.sb = sb; a.tb = tb; a.res = res; a.ldres = ldres; a.w = w; a.dil = dil;
  a.ga = ga; a.ldga = ldga; a.gb = gb; a.ldgb = ldgb; a.pw = pw; a.pa = pa; a.pa_pitch = pa_pitch;
  a.pa_col = pa_col; a.pb = pb;
  a.N = N; a.H = H; a.W = W; a.n = n; a.CV = n / FPE_V; a.cvb_log2 = rows_pick_cvb_log2(a.CV, 0);
  a.per = rows_per((long)H * W, chunks, a.cvb_log2);
  const dim3 grid = rows_grid(a.CV, a.cvb_log2, chunks, N);
  if (tail)
    SEG_LAUNCH_T((fpe_stage_bwd_kernel, 2), grid, dim3(CGN_THREADS), 0, stream, a);
  else if (has_b)
    SEG_LAUNCH_T((fpe_stage_bwd_kernel, 1), grid, dim3(CGN_THREADS), 0, stream, a);
  else
    SEG_LAUNCH_T((fpe_stage_bwd_kernel, 0), grid, dim3(CGN_THREADS), 0, stream, a);
  return check_launch("fpe_stage_bwd");
}

// rows of the partial arrays: high = 0 for seg_meu_bwd_low (pixels h*w), 1 for seg_meu_bwd_high
// (pixels h2*w2, passed as h, w); -1: out of contract
extern "C" int seg_meu_rows(int N, int h, int w, int C, int high) {
  using namespace seg;
  if (N < 1 || N > 65535 || h < 1 || w < 1 || C < 8 || C % 8 != 0 || C > MEU_MAX_C) return -1;
  const int CV = C / FPE_V;
  const int l = high ? rows_pick_cvb_log2(CV, 0) : rows_fit_cvb_log2(CV, 30);
  // (the low kernels keep a pixel's channels in one block row: one block column)
  return fpe_chunks(N, (long)h * w, high ? CV : 1 << l, l) * N;
}

extern "C" int seg_meu_fwd(int dtype, const void* L, long ldl, const float* sl, const float* tl,
                           const void* Hr, long ldh, const float* sh, const float* th,
                           const float* a_, const float* wsa, void* out, long ldo, float* sa, int N,
                           int h, int w, int h2, int w2, int C, void* stream) {
  using namespace seg;
  const long lds[3] = {ldl, ldh, ldo};
  if (meu_geometry("meu_fwd", dtype, N, h, w, h2, w2, C, lds, 3, 1)) return 1;
  SEG_REQUIRE(L != nullptr && Hr != nullptr && a_ != nullptr && wsa != nullptr && out != nullptr &&
                  sa != nullptr,
              "meu_fwd: null L / H / a / w_sa / out / sa");
  SEG_REQUIRE((sl == nullptr) == (tl == nullptr) && (sh == nullptr) == (th == nullptr),
              "meu_fwd: scale and shift go together");
  MeuArgs a = MeuArgs();
  meu_fill(&a, N, h, w, h2, w2, C);
  a.L = L; a.ldl = ldl; a.sl = sl; a.tl = tl; a.Hr = Hr; a.ldh = ldh; a.sh = sh; a.th = th;
  a.a = a_; a.wsa = wsa; a.out = out; a.ldo = ldo; a.sa = sa;
  a.cvb_log2 = rows_fit_cvb_log2(a.CV, 30);
  const int chunks = fpe_chunks(N, (long)h * w, 1 << a.cvb_log2, a.cvb_log2);
  a.per = rows_per((long)h * w, chunks, a.cvb_log2);
  SEG_LAUNCH_T((meu_low_kernel, false), dim3(1, chunks, N), dim3(CGN_THREADS), 0, stream, a);
  return check_launch("meu_fwd");
}

extern "C" int seg_meu_bwd_low(int dtype, const void* g, long ldg, const void* L, long ldl,
                               const float* sl, const float* tl, const void* Hr, long ldh,
                               const float* sh, const float* th, const float* a_, const float* wsa,
                               const float* sa, void* dL, long lddl, int N, int h, int w, int h2,
                               int w2, int C, float* p_a, float* p_bn, int rows, void* stream) {
  using namespace seg;
  int chunks;
  const long lds[4] = {ldg, ldl, ldh, lddl};
  if (fpe_rows_ok("meu_bwd_low", rows, N, &chunks)) return 1;
  if (meu_geometry("meu_bwd_low", dtype, N, h, w, h2, w2, C, lds, 4, chunks)) return 1;
  SEG_REQUIRE(g != nullptr && L != nullptr && Hr != nullptr && a_ != nullptr && wsa != nullptr &&
                  sa != nullptr && dL != nullptr && p_a != nullptr && p_bn != nullptr,
              "meu_bwd_low: null operand");
  SEG_REQUIRE((sl == nullptr) == (tl == nullptr) && (sh == nullptr) == (th == nullptr),
              "meu_bwd_low: scale and shift go together");
  MeuArgs a = MeuArgs();
  meu_fill(&a, N, h, w, h2, w2, C);
  a.g = g; a.ldg = ldg; a.L = L; a.ldl = ldl; a.sl = sl; a.tl = tl; a.Hr = Hr; a.ldh = ldh;
  a.sh = sh; a.th = th; a.a = a_; a.wsa = wsa; a.sa = const_cast<float*>(sa);
  a.out = dL; a.ldo = lddl; a.p1 = p_a; a.p2 = p_bn;
  a.cvb_log2 = rows_fit_cvb_log2(a.CV, 30);
  a.per = rows_per((long)h * w, chunks, a.cvb_log2);
  SEG_LAUNCH_T((meu_low_kernel, true), dim3(1, chunks, N), dim3(CGN_THREADS), 0, stream, a);
  return check_launch("meu_bwd_low");
}

extern "C" int seg_meu_bwd_high(int dtype, const void* g, long ldg, const float* sa, const void* Hr,
                                long ldh, const float* dpool, void* dH, long lddh, int N, int h,
                                int w, int h2, int w2, int C, float* p_bn, int rows, void* stream) {
  using namespace seg;
  int chunks;
  const long lds[3] = {ldg, ldh, lddh};
  if (fpe_rows_ok("meu_bwd_high", rows, N, &chunks)) return 1;
  if (meu_geometry("meu_bwd_high", dtype, N, h, w, h2, w2, C, lds, 3, chunks)) return 1;
  SEG_REQUIRE(g != nullptr && sa != nullptr && Hr != nullptr && dH != nullptr && p_bn != nullptr,
              "meu_bwd_high: null operand");
  MeuArgs a = MeuArgs();
  meu_fill(&a, N, h, w, h2, w2, C);
  a.g = g; a.ldg = ldg; a.sa = const_cast<float*>(sa); a.Hr = Hr; a.ldh = ldh; a.dpool = dpool;
  a.out = dH; a.ldo = lddh; a.p2 = p_bn;
  a.cvb_log2 = rows_pick_cvb_log2(a.CV, 0);
  a.per = rows_per((long)h2 * w2, chunks, a.cvb_log2);
  SEG_LAUNCH_T(meu_high_bwd_kernel, rows_grid(a.CV, a.cvb_log2, chunks, N), dim3(CGN_THREADS), 0,
               stream, a);
  return check_launch("meu_bwd_high");
}
