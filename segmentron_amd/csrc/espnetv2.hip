// ESPNetv2's EESP unit (segmentron/modules/module.py:165-207) and DownSampler
// (segmentron/models/backbones/eespnet.py:14-43) on NHWC tensors: the operators the conv /
// BatchNorm / PReLU machinery lacks.
//   seg_eesp_pyr_fwd       the depthwise pyramid: four depthwise 3x3 of dilation d0 <= d1 <= d2 <= d3
//                          (padding = dilation, stride 1 or 2) of the same n-channel x with the
//                          hierarchical fusion y_j = sum_{i <= j} dw_i(x), written as the 4n-channel
//                          concat, in ONE pass over x: the centre tap is loaded once for all four
//                          branches, a branch whose dilation equals its predecessor's reuses all of
//                          its taps, so x is fetched once per distinct tap offset (33 for 1,2,3,4;
//                          25 for 1,1,2,3).  The sums are fp32 and round once at the store.  The
//                          BatchNorm statistic partials [rows][2][4n] of the fp32 values come out of
//                          the same pass.
//   seg_eesp_suffix_sum    S_j = sum_{i >= j} g_i over the four n-channel slices of the pyramid's
//                          output gradient: what branch j's depthwise backward sees.  One
//                          element-wise pass, in place if wanted.
//   seg_avgpool3x3s2_*     nn.AvgPool2d(3, 2, 1), count_include_pad: the divisor is 9 everywhere;
//                          the backward gathers the <= 4 outputs that read an input pixel.
//   seg_bn_add_prelu_*     y = prelu(a * sa + ta + b * sb + tb, alpha) and its mask / dalpha pass:
//                          the EESP tail and the DownSampler tail.
// The pyramid and the tails use the launch geometry of csrc/cgnet.hip (rows.h): no atomics, fp32
// partial rows per (chunk, image) summed in index order, the same bits on every launch, and an
// image never reaches another image's outputs or partial rows.
#include "cgn_rows.h"

namespace seg {

// ------------------------------------------------------------------------------- pyramid forward
struct PyrArgs {
  const void* x; void* y;
  const float* w[4];  // [n][9] each: the [n,1,3,3] parameters as they are
  float* partial;
  long ldx, ldy, per;
  int N, H, W, Ho, Wo, n, CV, cvb_log2, s;
  int d[4];
};

constexpr int PYR_SMEM = 8 * CGN_THREADS * CGN_JV;  // the reduce's rows; the 36 weight rows fit

// FRESH: bit j set where branch j's dilation differs from branch j - 1's (bit 0 always).  A
// compile-time pattern: with the test at run time every tap load sits behind a branch and waits
// for the one before it (33 serial round trips per pixel); here all of a pixel's loads are in
// flight together.
template <typename T, int FRESH>
__global__ __launch_bounds__(CGN_THREADS) void eesp_pyr_fwd_kernel(const PyrArgs a) {
  constexpr int V = CGN_JV;
  __shared__ __attribute__((aligned(16))) float smem[PYR_SMEM];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2, spb = CGN_THREADS >> a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int cv = blockIdx.x * cvb + cx;
  const int img_n = blockIdx.z;
  const int Wd = cvb * V;
  // weights -> LDS [branch * 9 + tap][Wd]: 144 values per thread would not stay in registers
  for (int i = tid; i < 36 * Wd; i += CGN_THREADS) {
    const int jk = i / Wd, e = i - jk * Wd;
    const int j = jk / 9, k = jk - j * 9;
    const int c = blockIdx.x * Wd + e;
    smem[i] = c < a.n ? a.w[j][(long)c * 9 + k] : 0.f;
  }
  __syncthreads();
  float acc[8][V];  // sums of y_0..y_3, then of their squares
#pragma unroll
  for (int k = 0; k < 8; ++k)
#pragma unroll
    for (int e = 0; e < V; ++e) acc[k][e] = 0.f;
  if (cv < a.CV) {
    const int c0 = cv * V;
    const long HW = (long)a.H * a.W, HWo = (long)a.Ho * a.Wo;
    const T* __restrict__ img = reinterpret_cast<const T*>(a.x) + (long)img_n * HW * a.ldx + c0;
    T* __restrict__ out = reinterpret_cast<T*>(a.y) + (long)img_n * HWo * a.ldy + c0;
    const float* wsm = smem + cx * V;
    const long q0 = (long)blockIdx.y * a.per;
    const long q1 = q0 + a.per < HWo ? q0 + a.per : HWo;
    for (long q = q0 + sy; q < q1; q += spb) {
      const int ho = (int)(q / a.Wo), wo = (int)(q - (long)ho * a.Wo);
      const int h = ho * a.s, w = wo * a.s;
      float o[4][V], f[V];
      HVec<T>::load(img + ((long)h * a.W + w) * a.ldx, f);  // the centre: one load, four branches
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 wv = *reinterpret_cast<const float4*>(wsm + (j * 9 + 4) * Wd);
        o[j][0] = wv.x * f[0]; o[j][1] = wv.y * f[1]; o[j][2] = wv.z * f[2]; o[j][3] = wv.w * f[3];
      }
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          if (kh == 1 && kw == 1) continue;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            // (zero padding per branch at its own dilation: the mask is of this branch's offset)
            if ((FRESH >> j) & 1)
              cgn_tap<T>(img, a.ldx, a.H, a.W, h + (kh - 1) * a.d[j], w + (kw - 1) * a.d[j], f);
            const float4 wv = *reinterpret_cast<const float4*>(wsm + (j * 9 + kh * 3 + kw) * Wd);
            o[j][0] = fmaf(wv.x, f[0], o[j][0]); o[j][1] = fmaf(wv.y, f[1], o[j][1]);
            o[j][2] = fmaf(wv.z, f[2], o[j][2]); o[j][3] = fmaf(wv.w, f[3], o[j][3]);
          }
        }
#pragma unroll
      for (int j = 1; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < V; ++e) o[j][e] += o[j - 1][e];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        HVec<T>::store(out + q * a.ldy + (long)j * a.n, o[j]);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          acc[j][e] += o[j][e];
          acc[4 + j][e] = fmaf(o[j][e], o[j][e], acc[4 + j][e]);
        }
      }
    }
  }
  // partial[row][2][4n]: k = stat * 4 + branch at offset k * n
  if (a.partial != nullptr) {
    __syncthreads();  // (the weights are read until the last pixel; the reduce reuses their LDS)
    rows_block_reduce<V, 8>(smem, acc, a.cvb_log2, blockIdx.x, a.n,
                            a.partial + ((long)blockIdx.y * a.N + img_n) * 8 * a.n, a.n);
  }
}

// ------------------------------------------------------------------------------- flat element-wise
struct FlatArgs {
  const void* x; void* y;
  long ldx, ldy, total;
  int N, H, W, Ho, Wo, CV, n;
};

// S_j = g_j + ... + g_3 (fp32, one rounding per slice); S may be g
template <typename T>
__global__ __launch_bounds__(256) void eesp_suffix_sum_kernel(const FlatArgs a) {
  constexpr int VEC = Vec<T>::N;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  const long row = i / a.CV;
  const int c0 = (int)(i - row * a.CV) * VEC;
  const T* g = reinterpret_cast<const T*>(a.x) + row * a.ldx + c0;
  T* s = reinterpret_cast<T*>(a.y) + row * a.ldy + c0;
  float f[4][VEC];
#pragma unroll
  for (int j = 0; j < 4; ++j) Vec<T>::unpack(ldg16(g + (long)j * a.n), f[j]);
#pragma unroll
  for (int j = 2; j >= 0; --j)
#pragma unroll
    for (int e = 0; e < VEC; ++e) f[j][e] += f[j + 1][e];
#pragma unroll
  for (int j = 0; j < 4; ++j) stg16(s + (long)j * a.n, Vec<T>::pack(f[j]));
}

template <typename T>
__global__ __launch_bounds__(256) void avgpool3x3s2_fwd_kernel(const FlatArgs a) {
  constexpr int VEC = Vec<T>::N;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  long r = i / a.CV;
  const int c0 = (int)(i - r * a.CV) * VEC;
  const int wo = (int)(r % a.Wo); r /= a.Wo;
  const int ho = (int)(r % a.Ho);
  const long n = r / a.Ho;
  const T* img = reinterpret_cast<const T*>(a.x) + n * a.H * a.W * a.ldx + c0;
  float s[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) s[e] = 0.f;
#pragma unroll
  for (int kh = -1; kh <= 1; ++kh)
#pragma unroll
    for (int kw = -1; kw <= 1; ++kw) {
      const int hh = 2 * ho + kh, ww = 2 * wo + kw;
      if ((unsigned)hh < (unsigned)a.H && (unsigned)ww < (unsigned)a.W) {
        float f[VEC];
        Vec<T>::unpack(ldg16(img + ((long)hh * a.W + ww) * a.ldx), f);
#pragma unroll
        for (int e = 0; e < VEC; ++e) s[e] += f[e];
      }
    }
#pragma unroll
  for (int e = 0; e < VEC; ++e) s[e] *= (1.f / 9.f);
  T* y = reinterpret_cast<T*>(a.y) + ((n * a.Ho + ho) * a.Wo + wo) * a.ldy + c0;
  stg16(y, Vec<T>::pack(s));
}

// gx[h][w] = (1/9) * sum of gy[ho][wo] over |2 ho - h| <= 1, |2 wo - w| <= 1: each gx written once
template <typename T>
__global__ __launch_bounds__(256) void avgpool3x3s2_bwd_kernel(const FlatArgs a) {
  constexpr int VEC = Vec<T>::N;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  long r = i / a.CV;
  const int c0 = (int)(i - r * a.CV) * VEC;
  const int w = (int)(r % a.W); r /= a.W;
  const int h = (int)(r % a.H);
  const long n = r / a.H;
  const T* gy = reinterpret_cast<const T*>(a.x) + n * a.Ho * a.Wo * a.ldx + c0;
  float s[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) s[e] = 0.f;
  // outputs whose window holds h: ho = h/2 (h even), (h-1)/2 and (h+1)/2 (h odd)
  const int ho0 = h >> 1, ho1 = (h + 1) >> 1, wo0 = w >> 1, wo1 = (w + 1) >> 1;
  for (int ho = ho0; ho <= ho1; ++ho)
    for (int wo = wo0; wo <= wo1; ++wo)
      if (ho < a.Ho && wo < a.Wo) {
        float f[VEC];
        Vec<T>::unpack(ldg16(gy + ((long)ho * a.Wo + wo) * a.ldx), f);
#pragma unroll
        for (int e = 0; e < VEC; ++e) s[e] += f[e];
      }
#pragma unroll
  for (int e = 0; e < VEC; ++e) s[e] *= (1.f / 9.f);
  T* gx = reinterpret_cast<T*>(a.y) + ((n * a.H + h) * a.W + w) * a.ldy + c0;
  stg16(gx, Vec<T>::pack(s));
}

// ------------------------------------------------------------------------------- BN + add + PReLU
struct AddPreluArgs {
  const void* a; const void* b; const void* g; void* y;
  const float* sa; const float* ta; const float* sb; const float* tb; const float* alpha;
  float* partial;  // [chunks][N][C]
  long lda, ldb, ldg, ldy, HW, per;
  int N, C, CV, cvb_log2;
};

// BWD false: y = prelu(z);  BWD true: y = g_z = z > 0 ? g : alpha * g and the dalpha rows
template <typename T, bool BWD>
__global__ __launch_bounds__(CGN_THREADS) void bn_add_prelu_kernel(const AddPreluArgs a) {
  constexpr int VEC = Vec<T>::N;
  __shared__ __attribute__((aligned(16))) float smem[CGN_THREADS * VEC];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2, spb = CGN_THREADS >> a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int cv = blockIdx.x * cvb + cx;
  const int n = blockIdx.z;
  const T* __restrict__ A = reinterpret_cast<const T*>(a.a);
  const T* __restrict__ B = reinterpret_cast<const T*>(a.b);
  const T* __restrict__ G = reinterpret_cast<const T*>(a.g);
  T* __restrict__ Y = reinterpret_cast<T*>(a.y);
  float acc[1][VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[0][e] = 0.f;
  if (cv < a.CV) {
    const int c0 = cv * VEC;
    float sa[VEC], ta[VEC], sb[VEC], tb[VEC], al[VEC];
    cgn_params<VEC>(a.sa, 0, c0, a.C, 1.f, sa);
    cgn_params<VEC>(a.ta, 0, c0, a.C, 0.f, ta);
    cgn_params<VEC>(a.sb, 0, c0, a.C, 1.f, sb);
    cgn_params<VEC>(a.tb, 0, c0, a.C, 0.f, tb);
    cgn_params<VEC>(a.alpha, 0, c0, a.C, 0.f, al);
    const long q0 = (long)blockIdx.y * a.per;
    const long q1 = q0 + a.per < a.HW ? q0 + a.per : a.HW;
    for (long q = q0 + sy; q < q1; q += spb) {
      const long row = (long)n * a.HW + q;
      float fa[VEC], fb[VEC], g[VEC];
      Vec<T>::unpack(ldg16(A + row * a.lda + c0), fa);
      Vec<T>::unpack(ldg16(B + row * a.ldb + c0), fb);
      if (BWD) Vec<T>::unpack(ldg16(G + row * a.ldg + c0), g);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float z = fmaf(fa[e], sa[e], ta[e]) + fmaf(fb[e], sb[e], tb[e]);
        const bool pos = z > 0.f;  // (z == 0: the slope is alpha, as torch's prelu backward)
        if (BWD) {
          acc[0][e] += pos ? 0.f : g[e] * z;
          fa[e] = pos ? g[e] : al[e] * g[e];
        } else {
          fa[e] = pos ? z : al[e] * z;
        }
      }
      stg16(Y + row * a.ldy + c0, Vec<T>::pack(fa));
    }
  }
  if (BWD)
    rows_block_reduce<VEC, 1>(smem, acc, a.cvb_log2, blockIdx.x, a.C,
                              a.partial + ((long)blockIdx.y * a.N + n) * a.C, 0);
}

static int pyr_geometry(const char* what, int dtype, int N, int H, int W, int n, const int* d,
                        int stride) {
  SEG_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "%s: bad dtype %d", what, dtype);
  SEG_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && W >= 1, "%s: bad shape N=%d H=%d W=%d", what, N, H,
              W);
  SEG_REQUIRE(n >= 8 && n % 8 == 0, "%s: n=%d is not a positive multiple of 8", what, n);
  SEG_REQUIRE(stride == 1 || stride == 2, "%s: stride %d not in {1, 2}", what, stride);
  for (int j = 0; j < 4; ++j)
    SEG_REQUIRE(d[j] >= 1 && d[j] <= 4 && (j == 0 || d[j] >= d[j - 1]),
                "%s: dilations %d,%d,%d,%d are not in 1..4 and nondecreasing", what, d[0], d[1],
                d[2], d[3]);
  SEG_REQUIRE((long)H * W < (1L << 31), "%s: too large", what);
  return 0;
}

static int flat_common(const char* what, int dtype, long rows, int C, const long* lds,
                       const int* need, int nld, FlatArgs* a) {
  SEG_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "%s: bad dtype %d", what, dtype);
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(rows >= 1 && C >= vec && C % vec == 0,
              "%s: bad shape rows=%ld C=%d (C a multiple of %d)", what, rows, C, vec);
  for (int i = 0; i < nld; ++i)
    SEG_REQUIRE(lds[i] % vec == 0 && lds[i] >= need[i],
                "%s: row pitch %ld not a multiple of %d / < %d", what, lds[i], vec, need[i]);
  *a = FlatArgs();
  a->CV = C / vec;
  a->total = rows * a->CV;
  SEG_REQUIRE((a->total + 255) / 256 < (1L << 31), "%s: too large", what);
  return 0;
}

static int add_prelu_common(const char* what, int dtype, int N, long HW, int C, const long* lds,
                            int nld, int chunks, AddPreluArgs* a) {
  const int vec = dtype == DT_BF16 ? 8 : 4;
  if (rows_require(what, dtype, N, HW, C, vec, vec, lds, nullptr, nld, chunks, CGN_MAX_CHUNKS))
    return 1;
  *a = AddPreluArgs();
  a->N = N; a->HW = HW; a->C = C; a->CV = C / vec; a->cvb_log2 = rows_pick_cvb_log2(a->CV, 0);
  a->per = rows_per(HW, chunks, a->cvb_log2);
  return 0;
}

}  // namespace seg

// Pixel chunks per image of the pyramid launch (rows of its partial buffer per image), over the
// OUTPUT pixels: about 2048 blocks, at least one block row of pixels per chunk, at most 256.
extern "C" int seg_eesp_pyr_chunks(int N, int H, int W, int n, int stride) {
  using namespace seg;
  if (N < 1 || H < 1 || W < 1 || n < 8 || n % 8 != 0 || (stride != 1 && stride != 2)) return -1;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const int CV = n / CGN_JV, l = rows_pick_cvb_log2(CV, 0);
  return rows_chunks(N, rows_gx(CV, l), (long)Ho * Wo, CGN_THREADS >> l, 2048, CGN_MAX_CHUNKS);
}

// y [N,Ho,Wo,4n] (pitch ldy >= 4n), Ho = (H-1)/stride + 1; partial fp32 [chunks * N][2][4n], nullable
extern "C" int seg_eesp_pyr_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int n,
                                const float* w0, const float* w1, const float* w2, const float* w3,
                                int d0, int d1, int d2, int d3, int stride, void* y, long ldy,
                                float* partial, int chunks, void* stream) {
  using namespace seg;
  const int d[4] = {d0, d1, d2, d3};
  if (pyr_geometry("eesp_pyr_fwd", dtype, N, H, W, n, d, stride)) return 1;
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(ldx % vec == 0 && ldx >= n && ldy % vec == 0 && ldy >= 4L * n,
              "eesp_pyr_fwd: row pitches %ld / %ld not multiples of %d, or below n / 4n", ldx, ldy,
              vec);
  SEG_REQUIRE(chunks >= 1 && chunks <= CGN_MAX_CHUNKS, "eesp_pyr_fwd: chunks %d out of [1, %d]",
              chunks, CGN_MAX_CHUNKS);
  SEG_REQUIRE(x != nullptr && y != nullptr && w0 != nullptr && w1 != nullptr && w2 != nullptr &&
                  w3 != nullptr, "eesp_pyr_fwd: null x / y / weights");
  PyrArgs a = PyrArgs();
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.partial = partial;
  a.w[0] = w0; a.w[1] = w1; a.w[2] = w2; a.w[3] = w3;
  a.N = N; a.H = H; a.W = W; a.n = n; a.s = stride;
  a.Ho = (H - 1) / stride + 1; a.Wo = (W - 1) / stride + 1;
  for (int j = 0; j < 4; ++j) a.d[j] = d[j];
  a.CV = n / CGN_JV; a.cvb_log2 = rows_pick_cvb_log2(a.CV, 0);
  a.per = rows_per((long)a.Ho * a.Wo, chunks, a.cvb_log2);
  const int fresh = 1 | (d[1] != d[0]) << 1 | (d[2] != d[1]) << 2 | (d[3] != d[2]) << 3;
  const dim3 grid = rows_grid(a.CV, a.cvb_log2, chunks, a.N);
#define PYR_CASE(F)                                                                          \
  case F:                                                                                    \
    SEG_LAUNCH_T((eesp_pyr_fwd_kernel, F), grid, dim3(CGN_THREADS), 0, stream, a);           \
    break;
  switch (fresh) {
    PYR_CASE(1) PYR_CASE(3) PYR_CASE(5) PYR_CASE(7) PYR_CASE(9) PYR_CASE(11) PYR_CASE(13)
    PYR_CASE(15)
  }
#undef PYR_CASE
  return check_launch("eesp_pyr_fwd");
}

// g, s: [rows][4n] with pitches; s may be g (each thread reads its four vectors before it writes)
extern "C" int seg_eesp_suffix_sum(int dtype, const void* g, long ldg, void* s, long lds, long rows,
                                   int n, void* stream) {
  using namespace seg;
  FlatArgs a;
  const long lda[2] = {ldg, lds};
  const int need[2] = {4 * n, 4 * n};
  if (flat_common("eesp_suffix_sum", dtype, rows, n, lda, need, 2, &a)) return 1;
  SEG_REQUIRE(g != nullptr && s != nullptr, "eesp_suffix_sum: null g / s");
  a.x = g; a.ldx = ldg; a.y = s; a.ldy = lds; a.n = n;
  SEG_LAUNCH_T(eesp_suffix_sum_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0,
               stream, a);
  return check_launch("eesp_suffix_sum");
}

// y [N,Ho,Wo,C], Ho = (H-1)/2 + 1
extern "C" int seg_avgpool3x3s2_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                                    void* y, long ldy, void* stream) {
  using namespace seg;
  SEG_REQUIRE(N >= 1 && H >= 1 && W >= 1, "avgpool3x3s2_fwd: bad shape N=%d H=%d W=%d", N, H, W);
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  FlatArgs a;
  const long lda[2] = {ldx, ldy};
  const int need[2] = {C, C};
  if (flat_common("avgpool3x3s2_fwd", dtype, (long)N * Ho * Wo, C, lda, need, 2, &a)) return 1;
  SEG_REQUIRE(x != nullptr && y != nullptr, "avgpool3x3s2_fwd: null x / y");
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.N = N; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo;
  SEG_LAUNCH_T(avgpool3x3s2_fwd_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0,
               stream, a);
  return check_launch("avgpool3x3s2_fwd");
}

// gy [N,Ho,Wo,C] -> gx [N,H,W,C], every element written
extern "C" int seg_avgpool3x3s2_bwd(int dtype, const void* gy, long ldgy, int N, int H, int W, int C,
                                    void* gx, long ldgx, void* stream) {
  using namespace seg;
  SEG_REQUIRE(N >= 1 && H >= 1 && W >= 1, "avgpool3x3s2_bwd: bad shape N=%d H=%d W=%d", N, H, W);
  FlatArgs a;
  const long lda[2] = {ldgy, ldgx};
  const int need[2] = {C, C};
  if (flat_common("avgpool3x3s2_bwd", dtype, (long)N * H * W, C, lda, need, 2, &a)) return 1;
  SEG_REQUIRE(gy != nullptr && gx != nullptr, "avgpool3x3s2_bwd: null gy / gx");
  a.x = gy; a.ldx = ldgy; a.y = gx; a.ldy = ldgx; a.N = N; a.H = H; a.W = W;
  a.Ho = (H - 1) / 2 + 1; a.Wo = (W - 1) / 2 + 1;
  SEG_LAUNCH_T(avgpool3x3s2_bwd_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0,
               stream, a);
  return check_launch("avgpool3x3s2_bwd");
}

// sa / ta and sb / tb each nullable as a pair: that operand is plain
extern "C" int seg_bn_add_prelu_fwd(int dtype, const void* a_, long lda, const float* sa,
                                    const float* ta, const void* b_, long ldb, const float* sb,
                                    const float* tb, const float* alpha, void* y, long ldy, int N,
                                    long HW, int C, int chunks, void* stream) {
  using namespace seg;
  AddPreluArgs a;
  const long lds[3] = {lda, ldb, ldy};
  if (add_prelu_common("bn_add_prelu_fwd", dtype, N, HW, C, lds, 3, chunks, &a)) return 1;
  SEG_REQUIRE(a_ != nullptr && b_ != nullptr && alpha != nullptr && y != nullptr,
              "bn_add_prelu_fwd: null a / b / alpha / y");
  SEG_REQUIRE((sa == nullptr) == (ta == nullptr) && (sb == nullptr) == (tb == nullptr),
              "bn_add_prelu_fwd: scale and shift go together");
  a.a = a_; a.lda = lda; a.b = b_; a.ldb = ldb; a.y = y; a.ldy = ldy;
  a.sa = sa; a.ta = ta; a.sb = sb; a.tb = tb; a.alpha = alpha;
  SEG_LAUNCH_T((bn_add_prelu_kernel, false), rows_grid(a.CV, a.cvb_log2, chunks, N),
               dim3(CGN_THREADS), 0, stream, a);
  return check_launch("bn_add_prelu_fwd");
}

// g_z = z > 0 ? g : alpha * g with z recomputed; partial [chunks][N][C]: dalpha = seg_colsum over
// its chunks * N rows
extern "C" int seg_bn_add_prelu_bwd(int dtype, const void* g, long ldg, const void* a_, long lda,
                                    const float* sa, const float* ta, const void* b_, long ldb,
                                    const float* sb, const float* tb, const float* alpha, void* g_z,
                                    long ldgz, int N, long HW, int C, float* partial, int chunks,
                                    void* stream) {
  using namespace seg;
  AddPreluArgs a;
  const long lds[4] = {lda, ldb, ldg, ldgz};
  if (add_prelu_common("bn_add_prelu_bwd", dtype, N, HW, C, lds, 4, chunks, &a)) return 1;
  SEG_REQUIRE(a_ != nullptr && b_ != nullptr && alpha != nullptr && g != nullptr &&
                  g_z != nullptr && partial != nullptr,
              "bn_add_prelu_bwd: null a / b / alpha / g / g_z / partial");
  SEG_REQUIRE((sa == nullptr) == (ta == nullptr) && (sb == nullptr) == (tb == nullptr),
              "bn_add_prelu_bwd: scale and shift go together");
  a.a = a_; a.lda = lda; a.b = b_; a.ldb = ldb; a.g = g; a.ldg = ldg; a.y = g_z; a.ldy = ldgz;
  a.sa = sa; a.ta = ta; a.sb = sb; a.tb = tb; a.alpha = alpha; a.partial = partial;
  SEG_LAUNCH_T((bn_add_prelu_kernel, true), rows_grid(a.CV, a.cvb_log2, chunks, N),
               dim3(CGN_THREADS), 0, stream, a);
  return check_launch("bn_add_prelu_bwd");
}
