// CGNet's ContextGuidedBlock (segmentron/models/cgnet.py:149-181) on NHWC tensors: the operators
// the conv / BatchNorm / gate machinery lacks.
//   seg_cg_joint_fwd     joi[..., :C] = f_loc(x) (depthwise 3x3, dilation 1), joi[..., C:2C] =
//                        f_sur(x) (depthwise 3x3, dilation d) in ONE pass over x: the centre tap is
//                        loaded once for both, the 16 others once each; the BatchNorm statistic
//                        partials [rows][2][2C] of the fp32 accumulators come out of the same pass
//                        (its backward stays two fused depthwise backward launches: a direct joint
//                        backward of this form measured 3 - 5 x slower than them, profiles/cgnet.md)
//   seg_bn_prelu_fwd    y = prelu(x * scale + shift, alpha) (+ per-image channel sums of the fp32
//                        activated values: nn.AdaptiveAvgPool2d(1) behind it)
//   seg_prelu_bwd        g = g_y + g_pool / HW;  g_z = z > 0 ? g : alpha * g  (z recomputed) and
//                        partial rows of dalpha = sum over z <= 0 of g * z
// One launch geometry: grid (channel-vector blocks, pixel chunks, images); a chunk is a CONTIGUOUS
// pixel range of one image, a thread keeps one channel vector of one image for its whole life, so
// the per-channel parameters and the per-channel sums live in registers.  A block sums its rows
// through LDS in row order and writes one fp32 partial row per (chunk, image); the rows are summed
// in index order.  No atomics: the same inputs give the same bits, and an image never reaches
// another image's outputs or partial rows.
// Ragged channel counts (CGNet concatenates 32 + 3 and 128 + 3 channels): the element-wise kernels
// take any C >= 1 in a buffer whose pitch holds C rounded up to 8; they read the per-channel
// parameters below C only and write finite zeros to channels [C, round_up(C, 8)).
#include "cgn_rows.h"

namespace seg {

// ------------------------------------------------------------------------------- BN + PReLU
struct PreluArgs {
  const void* x; const void* gy; void* y;
  const float* scale; const float* shift; const float* alpha; const float* gpool;
  float* partial;  // [chunks][N][C]
  long ldx, ldgy, ldy, HW, per;
  int N, C, CV, cvb_log2;
  float inv_hw;
};

template <typename T>
__global__ __launch_bounds__(CGN_THREADS) void bn_prelu_fwd_kernel(const PreluArgs a) {
  constexpr int VEC = Vec<T>::N;
  __shared__ __attribute__((aligned(16))) float smem[CGN_THREADS * VEC];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2, spb = CGN_THREADS >> a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int cv = blockIdx.x * cvb + cx;
  const int n = blockIdx.z;
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  T* __restrict__ Y = reinterpret_cast<T*>(a.y);
  float acc[1][VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[0][e] = 0.f;
  if (cv < a.CV) {
    const int c0 = cv * VEC;
    float s[VEC], t[VEC], al[VEC];
    cgn_params<VEC>(a.scale, 0, c0, a.C, 1.f, s);
    cgn_params<VEC>(a.shift, 0, c0, a.C, 0.f, t);
    cgn_params<VEC>(a.alpha, 0, c0, a.C, 0.f, al);
    const long q0 = (long)blockIdx.y * a.per;
    const long q1 = q0 + a.per < a.HW ? q0 + a.per : a.HW;
    for (long q = q0 + sy; q < q1; q += spb) {
      const long row = (long)n * a.HW + q;
      float f[VEC];
      Vec<T>::unpack(ldg16(X + row * a.ldx + c0), f);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float z = fmaf(f[e], s[e], t[e]);
        const float v = z > 0.f ? z : al[e] * z;
        f[e] = c0 + e < a.C ? v : 0.f;  // (a select: the pad channels of x may hold anything)
        acc[0][e] += f[e];
      }
      if (Y != nullptr) stg16(Y + row * a.ldy + c0, Vec<T>::pack(f));
    }
  }
  if (a.partial != nullptr)
    rows_block_reduce<VEC, 1>(smem, acc, a.cvb_log2, blockIdx.x, a.C,
                              a.partial + ((long)blockIdx.y * a.N + n) * a.C, 0);
}

template <typename T>
__global__ __launch_bounds__(CGN_THREADS) void prelu_bwd_kernel(const PreluArgs a) {
  constexpr int VEC = Vec<T>::N;
  __shared__ __attribute__((aligned(16))) float smem[CGN_THREADS * VEC];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2, spb = CGN_THREADS >> a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int cv = blockIdx.x * cvb + cx;
  const int n = blockIdx.z;
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ GY = reinterpret_cast<const T*>(a.gy);
  T* __restrict__ GZ = reinterpret_cast<T*>(a.y);
  float acc[1][VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[0][e] = 0.f;
  if (cv < a.CV) {
    const int c0 = cv * VEC;
    float s[VEC], t[VEC], al[VEC], gp[VEC];
    cgn_params<VEC>(a.scale, 0, c0, a.C, 1.f, s);
    cgn_params<VEC>(a.shift, 0, c0, a.C, 0.f, t);
    cgn_params<VEC>(a.alpha, 0, c0, a.C, 0.f, al);
    cgn_params<VEC>(a.gpool, (long)n * a.C, c0, a.C, 0.f, gp);
#pragma unroll
    for (int e = 0; e < VEC; ++e) gp[e] *= a.inv_hw;
    const long q0 = (long)blockIdx.y * a.per;
    const long q1 = q0 + a.per < a.HW ? q0 + a.per : a.HW;
    for (long q = q0 + sy; q < q1; q += spb) {
      const long row = (long)n * a.HW + q;
      float f[VEC], g[VEC];
      Vec<T>::unpack(ldg16(X + row * a.ldx + c0), f);
      if (GY != nullptr) {
        Vec<T>::unpack(ldg16(GY + row * a.ldgy + c0), g);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) g[e] = 0.f;
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const bool live = c0 + e < a.C;
        const float z = fmaf(f[e], s[e], t[e]);
        const float gg = g[e] + gp[e];
        const bool pos = z > 0.f;  // (z == 0: the slope is alpha, as torch's prelu backward)
        g[e] = live ? (pos ? gg : al[e] * gg) : 0.f;
        acc[0][e] += (live && !pos) ? gg * z : 0.f;
      }
      stg16(GZ + row * a.ldy + c0, Vec<T>::pack(g));
    }
  }
  rows_block_reduce<VEC, 1>(smem, acc, a.cvb_log2, blockIdx.x, a.C,
                            a.partial + ((long)blockIdx.y * a.N + n) * a.C, 0);
}

// ------------------------------------------------------------------------------- joint depthwise
struct JointArgs {
  const void* x; const void* g; void* y;
  const float* wl; const float* ws;  // [C][9] each: the [C,1,3,3] parameters as they are
  float* partial;
  long ldx, ldg, ldy, per;
  int N, H, W, C, CV, cvb_log2, d;
};

template <typename T>
__global__ __launch_bounds__(CGN_THREADS) void cg_joint_fwd_kernel(const JointArgs a) {
  constexpr int V = CGN_JV;
  __shared__ __attribute__((aligned(16))) float smem[4 * CGN_THREADS * V];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2, spb = CGN_THREADS >> a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int cv = blockIdx.x * cvb + cx;
  const int n = blockIdx.z;
  const long HW = (long)a.H * a.W;
  float acc[4][V];  // sum loc, sum sur, sum loc^2, sum sur^2
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < V; ++e) acc[k][e] = 0.f;
  if (cv < a.CV) {
    const int c0 = cv * V;
    float wl[9][V], ws[9][V];
#pragma unroll
    for (int e = 0; e < V; ++e)
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        wl[k][e] = a.wl[(long)(c0 + e) * 9 + k];
        ws[k][e] = a.ws[(long)(c0 + e) * 9 + k];
      }
    const T* __restrict__ img = reinterpret_cast<const T*>(a.x) + (long)n * HW * a.ldx + c0;
    T* __restrict__ out = reinterpret_cast<T*>(a.y) + (long)n * HW * a.ldy + c0;
    const int d = a.d;
    const long q0 = (long)blockIdx.y * a.per;
    const long q1 = q0 + a.per < HW ? q0 + a.per : HW;
    for (long q = q0 + sy; q < q1; q += spb) {
      const int h = (int)(q / a.W), w = (int)(q - (long)h * a.W);
      float ol[V], os[V], f[V];
      HVec<T>::load(img + q * a.ldx, f);  // the centre: one load, both branches
#pragma unroll
      for (int e = 0; e < V; ++e) { ol[e] = wl[4][e] * f[e]; os[e] = ws[4][e] * f[e]; }
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          if (kh == 1 && kw == 1) continue;
          cgn_tap<T>(img, a.ldx, a.H, a.W, h + kh - 1, w + kw - 1, f);
#pragma unroll
          for (int e = 0; e < V; ++e) ol[e] = fmaf(wl[kh * 3 + kw][e], f[e], ol[e]);
          cgn_tap<T>(img, a.ldx, a.H, a.W, h + (kh - 1) * d, w + (kw - 1) * d, f);
#pragma unroll
          for (int e = 0; e < V; ++e) os[e] = fmaf(ws[kh * 3 + kw][e], f[e], os[e]);
        }
      HVec<T>::store(out + q * a.ldy, ol);
      HVec<T>::store(out + q * a.ldy + a.C, os);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        acc[0][e] += ol[e]; acc[1][e] += os[e];
        acc[2][e] = fmaf(ol[e], ol[e], acc[2][e]); acc[3][e] = fmaf(os[e], os[e], acc[3][e]);
      }
    }
  }
  // partial[row][2][2C]: k = 0..3 -> (sum | loc), (sum | sur), (sq | loc), (sq | sur)
  if (a.partial != nullptr)
    rows_block_reduce<V, 4>(smem, acc, a.cvb_log2, blockIdx.x, a.C,
                            a.partial + ((long)blockIdx.y * a.N + n) * 4 * a.C, a.C);
}

static int prelu_common(const char* what, int dtype, int N, long HW, int C, const long* lds,
                        int nld, int chunks, PreluArgs* a) {
  const int vec = dtype == DT_BF16 ? 8 : 4;
  // (any C >= 1; every pitch holds C rounded up to 8)
  const int Cp = cgn_round8(C), need[3] = {Cp, Cp, Cp};
  if (rows_require(what, dtype, N, HW, C, 1, vec, lds, need, nld, chunks, CGN_MAX_CHUNKS)) return 1;
  *a = PreluArgs();
  a->N = N; a->HW = HW; a->C = C; a->CV = Cp / vec; a->cvb_log2 = rows_pick_cvb_log2(a->CV, 0);
  a->per = rows_per(HW, chunks, a->cvb_log2);
  return 0;
}

static int joint_common(const char* what, int dtype, int N, int H, int W, int C, int d,
                        const long* lds, const int* need, int nld, int chunks, JointArgs* a) {
  SEG_REQUIRE(H >= 1 && W >= 1 && d >= 1 && (long)H * W < (1L << 31) && (long)H + d < (1L << 30) &&
                  (long)W + d < (1L << 30),
              "%s: bad shape H=%d W=%d d=%d", what, H, W, d);
  if (rows_require(what, dtype, N, (long)H * W, C, CGN_JV, CGN_JV, lds, need, nld, chunks,
                   CGN_MAX_CHUNKS))
    return 1;
  *a = JointArgs();
  a->N = N; a->H = H; a->W = W; a->C = C; a->d = d; a->CV = C / CGN_JV;
  a->cvb_log2 = rows_pick_cvb_log2(a->CV, 0);
  a->per = rows_per((long)H * W, chunks, a->cvb_log2);
  return 0;
}

}  // namespace seg

// Pixel chunks per image of the joint launches (rows of their partial buffers per image): about
// 2048 blocks, at least one block row of pixels per chunk, at most 256 chunks.
extern "C" int seg_cg_joint_chunks(int N, int H, int W, int C) {
  using namespace seg;
  if (N < 1 || H < 1 || W < 1 || C < CGN_JV || C % CGN_JV != 0) return -1;
  const int CV = C / CGN_JV, l = rows_pick_cvb_log2(CV, 0);
  return rows_chunks(N, rows_gx(CV, l), (long)H * W, CGN_THREADS >> l, 2048, CGN_MAX_CHUNKS);
}

// y [N,H,W,2C] (pitch ldy >= 2C); partial fp32 [chunks * N][2][2C], nullable
extern "C" int seg_cg_joint_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                                const float* w_loc, const float* w_sur, int dil, void* y, long ldy,
                                float* partial, int chunks, void* stream) {
  using namespace seg;
  JointArgs a;
  const long lds[2] = {ldx, ldy};
  const int need[2] = {C, 2 * C};
  if (joint_common("cg_joint_fwd", dtype, N, H, W, C, dil, lds, need, 2, chunks, &a)) return 1;
  SEG_REQUIRE(x != nullptr && y != nullptr && w_loc != nullptr && w_sur != nullptr,
              "cg_joint_fwd: null x / y / weights");
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.wl = w_loc; a.ws = w_sur; a.partial = partial;
  SEG_LAUNCH_T(cg_joint_fwd_kernel, rows_grid(a.CV, a.cvb_log2, chunks, N), dim3(CGN_THREADS), 0,
               stream, a);
  return check_launch("cg_joint_fwd");
}

// y nullable (pool only), partial [chunks][N][C] nullable (no pool), scale / shift both null:
// plain PReLU.  Pitches hold C rounded up to 8; y's channels [C, round_up(C, 8)) become zero.
extern "C" int seg_bn_prelu_fwd(int dtype, const void* x, long ldx, const float* scale,
                                const float* shift, const float* alpha, void* y, long ldy, int N,
                                long HW, int C, float* partial, int chunks, void* stream) {
  using namespace seg;
  PreluArgs a;
  const long lds[2] = {ldx, y != nullptr ? ldy : ldx};
  if (prelu_common("bn_prelu_fwd", dtype, N, HW, C, lds, 2, chunks, &a)) return 1;
  SEG_REQUIRE(x != nullptr && alpha != nullptr && (y != nullptr || partial != nullptr),
              "bn_prelu_fwd: null x / alpha, or neither y nor partial");
  SEG_REQUIRE((scale == nullptr) == (shift == nullptr), "bn_prelu_fwd: scale and shift go together");
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.scale = scale; a.shift = shift; a.alpha = alpha;
  a.partial = partial;
  SEG_LAUNCH_T(bn_prelu_fwd_kernel, rows_grid(a.CV, a.cvb_log2, chunks, N), dim3(CGN_THREADS), 0,
               stream, a);
  return check_launch("bn_prelu_fwd");
}

// g_y nullable (the pooled output alone carried gradient), g_pool fp32 [N][C] nullable;
// partial [chunks][N][C]: dalpha = seg_colsum over its chunks * N rows
extern "C" int seg_prelu_bwd(int dtype, const void* g_y, long ldgy, const float* g_pool,
                             const void* x, long ldx, const float* scale, const float* shift,
                             const float* alpha, void* g_z, long ldgz, int N, long HW, int C,
                             float* partial, int chunks, void* stream) {
  using namespace seg;
  PreluArgs a;
  const long lds[3] = {ldx, ldgz, g_y != nullptr ? ldgy : ldx};
  if (prelu_common("prelu_bwd", dtype, N, HW, C, lds, 3, chunks, &a)) return 1;
  SEG_REQUIRE(x != nullptr && alpha != nullptr && g_z != nullptr && partial != nullptr &&
                  (g_y != nullptr || g_pool != nullptr),
              "prelu_bwd: null x / alpha / g_z / partial, or no gradient at all");
  SEG_REQUIRE((scale == nullptr) == (shift == nullptr), "prelu_bwd: scale and shift go together");
  a.x = x; a.ldx = ldx; a.gy = g_y; a.ldgy = ldgy; a.gpool = g_pool; a.y = g_z; a.ldy = ldgz;
  a.scale = scale; a.shift = shift; a.alpha = alpha; a.partial = partial;
  a.inv_hw = 1.f / (float)HW;
  SEG_LAUNCH_T(prelu_bwd_kernel, rows_grid(a.CV, a.cvb_log2, chunks, N), dim3(CGN_THREADS), 0,
               stream, a);
  return check_launch("prelu_bwd");
}
