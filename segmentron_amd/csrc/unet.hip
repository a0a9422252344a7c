// UNet (segmentron/models/unet.py): the two full-resolution passes the other kernels do not cover.
//
//   seg_skip_pool_fwd / _bwd   An encoder level's raw convolution output y is consumed twice: through
//       BatchNorm + ReLU into the decoder's torch.cat([skip, up]) (unet.py:120) and through
//       nn.MaxPool2d(2) (unet.py:86) into the next level.  Forward is ONE pass over y: skip = act(y)
//       into a channel slice of the level's concat buffer, pooled = the 2x2 / stride-2 max of the
//       STORED (rounded) values; no index tensor.  Backward is one pass too: the activation is
//       recomputed through the same device function (un_act; -ffp-contract=off, the bits agree), the
//       window's winner is the first maximum in row-major order (ATen's max_pool2d rule),
//       g' = relu_mask * (g_skip + scatter(g_pool)) is written densely and the block's sums
//       (sum g', sum g' * y) go to partial rows [R][2][C] in seg_bn_bwd_finalize_p's layout.  The rows
//       are summed in a fixed order: no atomics, bit-identical results on every launch.
//   seg_bilinear_pad_fwd / _bwd   Up.forward (unet.py:109-120) pads the upsampled map to the skip's
//       size: seg_bilinear_fwd with a destination window.  The resized Ho x Wo map lands at
//       (top, left) of an Hd x Wd map inside a pitched channel slice, the rest of the slice is zero;
//       the backward gathers from the window alone.  Same tap arithmetic (resize_taps.h) and the same
//       blend expression as resize.hip.  Only the levels with an odd size come here.
//
// All four are memory-bound: one 16-byte vector along C per lane and access.
#include "rows.h"
#include "resize_taps.h"

namespace seg {

constexpr int UN_THREADS = 256;
constexpr int UN_MAX_ROWS = 1024;  // partial rows of the backward: one finalize pass takes them

struct SkipPoolArgs {
  const void* y; const void* gs; const void* gp;
  void* skip; void* pooled; void* gx;
  float* partial;
  const float* scale; const float* shift;
  long ldy, lds, ldp, ldgs, ldgp, ldgx;
  int N, H, W, Hw, Ww, C, CV, mode;  // Hw x Ww windows (ceil): the last ones may be half outside
};

template <int N>
__device__ __forceinline__ void un_params(const SkipPoolArgs& a, int c0, float (&s)[N], float (&t)[N]) {
  if (a.mode & PRO_AFFINE) {
    load_params<N>(a.scale, c0, s);
    load_params<N>(a.shift, c0, t);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) { s[i] = 1.f; t[i] = 0.f; }
  }
}

// The stored activation of one raw vector: prologue in fp32, rounded to T once.  -> the vector as it
// is stored; r: the same values widened again (what the max and the mask are taken of).
template <typename T>
__device__ __forceinline__ uint4 un_act(const uint4& raw, int mode, const float (&s)[Vec<T>::N],
                                        const float (&t)[Vec<T>::N], float* r) {
  float f[Vec<T>::N];
  Vec<T>::unpack(raw, f);
  apply_prologue_regs<Vec<T>::N>(f, mode, s, t);
  const uint4 v = Vec<T>::pack(f);
  Vec<T>::unpack(v, r);
  return v;
}

// thread = (window, channel vector); the four taps of a window in row-major order
template <typename T>
__global__ __launch_bounds__(UN_THREADS) void skip_pool_fwd_kernel(const SkipPoolArgs a) {
  constexpr int VEC = Vec<T>::N;
  const T* __restrict__ Y = reinterpret_cast<const T*>(a.y);
  T* __restrict__ S = reinterpret_cast<T*>(a.skip);
  T* __restrict__ P = reinterpret_cast<T*>(a.pooled);
  const int total = a.N * a.Hw * a.Ww * a.CV;
  const int Hp = a.H >> 1, Wp = a.W >> 1;
  const float inv_cv = 1.f / (float)a.CV, inv_ww = 1.f / (float)a.Ww, inv_hw = 1.f / (float)a.Hw;
  for (int i = blockIdx.x * UN_THREADS + threadIdx.x; i < total; i += gridDim.x * UN_THREADS) {
    int p = fast_div(i, a.CV, inv_cv);
    const int cv = i - p * a.CV;
    int q = fast_div(p, a.Ww, inv_ww);
    const int ww = p - q * a.Ww;
    const int n = fast_div(q, a.Hw, inv_hw);
    const int hw = q - n * a.Hw;
    const int c0 = cv * VEC;
    float s[VEC], t[VEC];
    un_params<VEC>(a, c0, s, t);
    const bool hr = 2 * hw + 1 < a.H, wr = 2 * ww + 1 < a.W;
    const long p00 = ((long)n * a.H + 2 * hw) * a.W + 2 * ww;
    uint4 raw[4];
    raw[0] = ldg16(Y + p00 * a.ldy + c0);
    raw[1] = raw[0]; raw[2] = raw[0]; raw[3] = raw[0];
    if (wr) raw[1] = ldg16(Y + (p00 + 1) * a.ldy + c0);
    if (hr) raw[2] = ldg16(Y + (p00 + a.W) * a.ldy + c0);
    if (hr && wr) raw[3] = ldg16(Y + (p00 + a.W + 1) * a.ldy + c0);
    float best[VEC], r[VEC];
    uint4 v = un_act<T>(raw[0], a.mode, s, t, best);
    stg16(S + p00 * a.lds + c0, v);
    v = un_act<T>(raw[1], a.mode, s, t, r);
    if (wr) stg16(S + (p00 + 1) * a.lds + c0, v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) best[e] = r[e] > best[e] ? r[e] : best[e];
    v = un_act<T>(raw[2], a.mode, s, t, r);
    if (hr) stg16(S + (p00 + a.W) * a.lds + c0, v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) best[e] = r[e] > best[e] ? r[e] : best[e];
    v = un_act<T>(raw[3], a.mode, s, t, r);
    if (hr && wr) {
      stg16(S + (p00 + a.W + 1) * a.lds + c0, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) best[e] = r[e] > best[e] ? r[e] : best[e];
      // (a trailing odd row or column has no window: it goes to the skip only)
      stg16(P + (((long)n * Hp + hw) * Wp + ww) * a.ldp + c0, Vec<T>::pack(best));
    }
  }
}

// block = (cvb channel-vector lanes) x (UN_THREADS / cvb window lanes); blockIdx.y = channel block,
// blockIdx.x = partial row.  A thread keeps its channel vector and strides over the windows.
template <typename T>
__global__ __launch_bounds__(UN_THREADS) void skip_pool_bwd_kernel(const SkipPoolArgs a,
                                                                   int cvb_log2) {
  constexpr int VEC = Vec<T>::N;
  __shared__ float red[2 * UN_THREADS * VEC];
  const T* __restrict__ Y = reinterpret_cast<const T*>(a.y);
  const T* __restrict__ GS = reinterpret_cast<const T*>(a.gs);
  const T* __restrict__ GP = reinterpret_cast<const T*>(a.gp);
  T* __restrict__ GX = reinterpret_cast<T*>(a.gx);
  const int tid = threadIdx.x;
  const int cvb = 1 << cvb_log2, cx = tid & (cvb - 1), pl = tid >> cvb_log2;
  const int npl = UN_THREADS >> cvb_log2;
  const int cv = blockIdx.y * cvb + cx;
  const bool cok = cv < a.CV;
  const int c0 = (cok ? cv : 0) * VEC;
  const int Hp = a.H >> 1, Wp = a.W >> 1;
  const int nwin = a.N * a.Hw * a.Ww;
  const float inv_ww = 1.f / (float)a.Ww, inv_hw = 1.f / (float)a.Hw;
  float s[VEC], t[VEC], acc[2][VEC];  // sum g, sum g * y
  un_params<VEC>(a, c0, s, t);
#pragma unroll
  for (int e = 0; e < VEC; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
  if (cok) {
    for (int w = blockIdx.x * npl + pl; w < nwin; w += gridDim.x * npl) {
      int q = fast_div(w, a.Ww, inv_ww);
      const int ww = w - q * a.Ww;
      const int n = fast_div(q, a.Hw, inv_hw);
      const int hw = q - n * a.Hw;
      const bool hr = 2 * hw + 1 < a.H, wr = 2 * ww + 1 < a.W;
      const bool ok[4] = {true, wr, hr, hr && wr};
      const long p00 = ((long)n * a.H + 2 * hw) * a.W + 2 * ww;
      const long off[4] = {p00, p00 + 1, p00 + a.W, p00 + a.W + 1};
      uint4 raw[4], gs[4];
      raw[0] = ldg16(Y + p00 * a.ldy + c0);
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        raw[k] = raw[0];
        if (ok[k]) raw[k] = ldg16(Y + off[k] * a.ldy + c0);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        gs[k] = make_uint4(0u, 0u, 0u, 0u);
        if (GS != nullptr && ok[k]) gs[k] = ldg16(GS + off[k] * a.ldgs + c0);
      }
      float gp[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) gp[e] = 0.f;
      const bool full = ok[3] && GP != nullptr;
      if (full) Vec<T>::unpack(ldg16(GP + (((long)n * Hp + hw) * Wp + ww) * a.ldgp + c0), gp);
      float r[4][VEC], best[VEC];
      int bi[VEC];
#pragma unroll
      for (int k = 0; k < 4; ++k) un_act<T>(raw[k], a.mode, s, t, r[k]);
      // the winner: the first maximum of the stored values in row-major order
#pragma unroll
      for (int e = 0; e < VEC; ++e) { best[e] = r[0][e]; bi[e] = 0; }
#pragma unroll
      for (int k = 1; k < 4; ++k) {
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (r[k][e] > best[e]) { best[e] = r[k][e]; bi[e] = k; }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!ok[k]) continue;
        float g[VEC], yf[VEC];
        Vec<T>::unpack(gs[k], g);
        Vec<T>::unpack(raw[k], yf);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          if (full && bi[e] == k) g[e] += gp[e];
          if ((a.mode & PRO_RELU) && !(r[k][e] > 0.f)) g[e] = 0.f;
          acc[0][e] += g[e];
          acc[1][e] += g[e] * yf[e];
        }
        stg16(GX + off[k] * a.ldgx + c0, Vec<T>::pack(g));
      }
    }
  }
  // the window lanes' sums meet in lane order: [row][which][C]
  rows_block_reduce<VEC, 2, UN_THREADS>(red, acc, cvb_log2, blockIdx.y, a.C,
                                        a.partial + (long)blockIdx.x * 2 * a.C, a.C);
}

// ---------------------------------------------------------------- bilinear with a destination window
struct PlaceArgs {
  const void* x; void* y;
  const float* scale; const float* shift;
  long ldx, ldy;
  int N, Hi, Wi, Ho, Wo, Hd, Wd, top, left, C, CV, mode, align;
  float sh, sw;
};

// thread = (destination pixel of the Hd x Wd map, channel vector)
template <typename T>
__global__ __launch_bounds__(UN_THREADS) void bilinear_pad_fwd_kernel(const PlaceArgs a) {
  constexpr int VEC = Vec<T>::N;
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  T* __restrict__ Y = reinterpret_cast<T*>(a.y);
  const int total = a.N * a.Hd * a.Wd * a.CV;
  const float inv_cv = 1.f / (float)a.CV, inv_wd = 1.f / (float)a.Wd, inv_hd = 1.f / (float)a.Hd;
  for (int i = blockIdx.x * UN_THREADS + threadIdx.x; i < total; i += gridDim.x * UN_THREADS) {
    int p = fast_div(i, a.CV, inv_cv);
    const int cv = i - p * a.CV;
    int q = fast_div(p, a.Wd, inv_wd);
    const int wd = p - q * a.Wd;
    const int n = fast_div(q, a.Hd, inv_hd);
    const int hd = q - n * a.Hd;
    const int c0 = cv * VEC;
    const int ho = hd - a.top, wo = wd - a.left;
    T* __restrict__ dst = Y + (((long)n * a.Hd + hd) * a.Wd + wd) * a.ldy + c0;
    if (ho < 0 || ho >= a.Ho || wo < 0 || wo >= a.Wo) {
      stg16(dst, make_uint4(0u, 0u, 0u, 0u));
      continue;
    }
    int h0, h1, w0, w1; float lh, lw;
    taps(a.sh, ho, a.Hi, a.align, h0, h1, lh);
    taps(a.sw, wo, a.Wi, a.align, w0, w1, lw);
    const long base = (long)n * a.Hi * a.Wi;
    float f00[VEC], f01[VEC], f10[VEC], f11[VEC];
    Vec<T>::unpack(ldg16(X + (base + (long)h0 * a.Wi + w0) * a.ldx + c0), f00);
    Vec<T>::unpack(ldg16(X + (base + (long)h0 * a.Wi + w1) * a.ldx + c0), f01);
    Vec<T>::unpack(ldg16(X + (base + (long)h1 * a.Wi + w0) * a.ldx + c0), f10);
    Vec<T>::unpack(ldg16(X + (base + (long)h1 * a.Wi + w1) * a.ldx + c0), f11);
    if (a.mode != PRO_NONE) {
      float s[VEC], t[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) { s[e] = 1.f; t[e] = 0.f; }
      if (a.mode & PRO_AFFINE) {
        load_params<VEC>(a.scale, c0, s);
        load_params<VEC>(a.shift, c0, t);
      }
      apply_prologue_regs<VEC>(f00, a.mode, s, t);
      apply_prologue_regs<VEC>(f01, a.mode, s, t);
      apply_prologue_regs<VEC>(f10, a.mode, s, t);
      apply_prologue_regs<VEC>(f11, a.mode, s, t);
    }
    float o[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {  // (the expression and association of bilinear_fwd_kernel)
      const float up = (1.f - lw) * f00[k] + lw * f01[k];
      const float dn = (1.f - lw) * f10[k] + lw * f11[k];
      o[k] = (1.f - lh) * up + lh * dn;
    }
    stg16(dst, Vec<T>::pack(o));
  }
}

// thread = (source pixel, channel vector): a gather over the window's outputs that carry weight, ho
// ascending, wo ascending (deterministic, every gx written once)
template <typename T>
__global__ __launch_bounds__(UN_THREADS) void bilinear_pad_bwd_kernel(const PlaceArgs a) {
  constexpr int VEC = Vec<T>::N;
  const T* __restrict__ GY = reinterpret_cast<const T*>(a.y);
  T* __restrict__ GX = reinterpret_cast<T*>(const_cast<void*>(a.x));
  const int total = a.N * a.Hi * a.Wi * a.CV;
  const float inv_cv = 1.f / (float)a.CV, inv_wi = 1.f / (float)a.Wi, inv_hi = 1.f / (float)a.Hi;
  for (int i = blockIdx.x * UN_THREADS + threadIdx.x; i < total; i += gridDim.x * UN_THREADS) {
    int p = fast_div(i, a.CV, inv_cv);
    const int cv = i - p * a.CV;
    int q = fast_div(p, a.Wi, inv_wi);
    const int wi = p - q * a.Wi;
    const int n = fast_div(q, a.Hi, inv_hi);
    const int hi = q - n * a.Hi;
    const int c0 = cv * VEC;
    int hlo, hhi, wlo, whi;
    cand_range(a.sh, hi, a.Ho, a.align, hlo, hhi);
    cand_range(a.sw, wi, a.Wo, a.align, wlo, whi);
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    for (int ho = hlo; ho <= hhi; ++ho) {
      const float wh = tap_weight(a.sh, ho, a.Hi, a.align, hi);
      if (wh == 0.f) continue;
      const T* __restrict__ grow = GY + (((long)n * a.Hd + ho + a.top) * a.Wd + a.left) * a.ldy + c0;
      for (int wo = wlo; wo <= whi; ++wo) {
        const float wgt = tap_weight(a.sw, wo, a.Wi, a.align, wi);
        if (wgt == 0.f) continue;
        float g[VEC];
        Vec<T>::unpack(ldg16(grow + (long)wo * a.ldy), g);
        const float w = wh * wgt;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = fmaf(w, g[e], acc[e]);
      }
    }
    stg16(GX + (((long)n * a.Hi + hi) * a.Wi + wi) * a.ldx + c0, Vec<T>::pack(acc));
  }
}

constexpr int UN_MAX_BLOCKS = 8192;  // grid-stride beyond

// channel-vector lanes of a backward block: the smallest power of two that holds CV
// (rows_fit_cvb_log2), 32 at the most; the rest of the block's threads are its window lanes
constexpr int UN_MAX_LANES_LOG2 = 5;

static int fill_skip_pool(SkipPoolArgs& a, const char* what, int dtype, int N, int H, int W, int C,
                          int pro_mode, const float* pro_scale, const float* pro_shift) {
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "%s: bad dtype %d", what, dtype);
  SEG_REQUIRE(N >= 1 && C >= vec && C % vec == 0, "%s: N = %d, C = %d (a positive multiple of %d)",
              what, N, C, vec);
  SEG_REQUIRE(H >= 2 && W >= 2, "%s: a %d x %d map has no 2x2 window", what, H, W);
  SEG_REQUIRE((pro_mode & ~(PRO_AFFINE | PRO_RELU)) == 0, "%s: prologue mode %d", what, pro_mode);
  SEG_REQUIRE(((pro_mode & PRO_AFFINE) == 0) || (pro_scale && pro_shift),
              "%s: missing scale/shift", what);
  a.N = N; a.H = H; a.W = W; a.Hw = (H + 1) / 2; a.Ww = (W + 1) / 2; a.C = C; a.CV = C / vec;
  a.mode = pro_mode; a.scale = pro_scale; a.shift = pro_shift;
  a.y = a.gs = a.gp = nullptr; a.skip = a.pooled = a.gx = nullptr; a.partial = nullptr;
  a.ldy = a.lds = a.ldp = a.ldgs = a.ldgp = a.ldgx = 0;
  SEG_REQUIRE((long)N * a.Hw * a.Ww * a.CV < (1L << 30), "%s: too many vectors", what);
  return 0;
}

}  // namespace seg

extern "C" int seg_skip_pool_fwd(int dtype, const void* y, long ldy, int N, int H, int W, int C,
                                 int pro_mode, const float* pro_scale, const float* pro_shift,
                                 void* skip, long ldskip, void* pooled, long ldpool, void* stream) {
  using namespace seg;
  SkipPoolArgs a;
  if (fill_skip_pool(a, "skip_pool_fwd", dtype, N, H, W, C, pro_mode, pro_scale, pro_shift))
    return 1;
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(y && skip && pooled, "skip_pool_fwd: null operand");
  SEG_REQUIRE(ldy >= C && ldskip >= C && ldpool >= C && ldy % vec == 0 && ldskip % vec == 0 &&
                  ldpool % vec == 0, "skip_pool_fwd: pitches are multiples of %d, at least C", vec);
  SEG_REQUIRE_FAST_DIV("skip_pool_fwd", (long)N * a.Hw * a.Ww, a.CV);
  a.y = y; a.ldy = ldy; a.skip = skip; a.lds = ldskip; a.pooled = pooled; a.ldp = ldpool;
  const int grid = grid_1d((long)N * a.Hw * a.Ww * a.CV, UN_THREADS, UN_MAX_BLOCKS);
  SEG_LAUNCH_T(skip_pool_fwd_kernel, dim3(grid), dim3(UN_THREADS), 0, stream, a);
  return check_launch("skip_pool_fwd");
}

// partial rows of seg_skip_pool_bwd (0: bad arguments)
extern "C" int seg_skip_pool_bwd_rows(int dtype, int N, int H, int W, int C) {
  using namespace seg;
  if ((dtype != DT_F32 && dtype != DT_BF16) || N < 1 || H < 2 || W < 2 || C < 1) return 0;
  const int vec = dtype == DT_BF16 ? 8 : 4;
  if (C % vec != 0) return 0;
  const int npl = UN_THREADS >> rows_fit_cvb_log2(C / vec, UN_MAX_LANES_LOG2);
  const long nwin = (long)N * ((H + 1) / 2) * ((W + 1) / 2);
  long r = (nwin + npl - 1) / npl;
  if (r > UN_MAX_ROWS) r = UN_MAX_ROWS;
  return (int)r;
}

extern "C" int seg_skip_pool_bwd(int dtype, const void* g_skip, long ldgs, const void* g_pool,
                                 long ldgp, const void* y, long ldy, int N, int H, int W, int C,
                                 int pro_mode, const float* pro_scale, const float* pro_shift,
                                 void* gx, long ldgx, float* partial, int rows, void* stream) {
  using namespace seg;
  SkipPoolArgs a;
  if (fill_skip_pool(a, "skip_pool_bwd", dtype, N, H, W, C, pro_mode, pro_scale, pro_shift))
    return 1;
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(y && gx && partial, "skip_pool_bwd: null operand");
  SEG_REQUIRE(rows >= 1 && rows <= 65535, "skip_pool_bwd: %d partial rows", rows);
  SEG_REQUIRE(ldy >= C && ldgx >= C && ldy % vec == 0 && ldgx % vec == 0 &&
                  (!g_skip || (ldgs >= C && ldgs % vec == 0)) &&
                  (!g_pool || (ldgp >= C && ldgp % vec == 0)),
              "skip_pool_bwd: pitches are multiples of %d, at least C", vec);
  SEG_REQUIRE_FAST_DIV("skip_pool_bwd", (long)N * a.Hw, a.Ww);
  a.y = y; a.ldy = ldy; a.gs = g_skip; a.ldgs = ldgs; a.gp = g_pool; a.ldgp = ldgp;
  a.gx = gx; a.ldgx = ldgx; a.partial = partial;
  const int l2 = rows_fit_cvb_log2(a.CV, UN_MAX_LANES_LOG2);
  const dim3 grid(rows, rows_gx(a.CV, l2));
  SEG_REQUIRE(grid.y <= 65535, "skip_pool_bwd: C = %d beyond the launch grid", C);
  SEG_LAUNCH_T(skip_pool_bwd_kernel, grid, dim3(UN_THREADS), 0, stream, a, l2);
  return check_launch("skip_pool_bwd");
}

namespace seg {
static int fill_place(PlaceArgs& a, const char* what, int dtype, int N, int Hi, int Wi, int C,
                      int Ho, int Wo, int Hd, int Wd, int top, int left, long ldx, long ldy,
                      int align) {
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "%s: bad dtype %d", what, dtype);
  SEG_REQUIRE(N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "%s: empty", what);
  SEG_REQUIRE(C >= vec && C % vec == 0 && ldx % vec == 0 && ldy % vec == 0 && ldx >= C && ldy >= C,
              "%s: C and the pitches are multiples of %d", what, vec);
  SEG_REQUIRE(top >= 0 && left >= 0 && (long)top + Ho <= Hd && (long)left + Wo <= Wd,
              "%s: the %d x %d window at (%d, %d) leaves the %d x %d map", what, Ho, Wo, top, left,
              Hd, Wd);
  a.ldx = ldx; a.ldy = ldy; a.N = N; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.Hd = Hd;
  a.Wd = Wd; a.top = top; a.left = left; a.C = C; a.CV = C / vec; a.mode = PRO_NONE;
  a.scale = a.shift = nullptr; a.align = align;
  a.sh = host_scale(Hi, Ho, align); a.sw = host_scale(Wi, Wo, align);
  return 0;
}
}  // namespace seg

extern "C" int seg_bilinear_pad_fwd(int dtype, const void* x, long ldx, int N, int Hi, int Wi, int C,
                                    int pro_mode, const float* pro_scale, const float* pro_shift,
                                    void* y, long ldy, int Ho, int Wo, int Hd, int Wd, int top,
                                    int left, int align_corners, void* stream) {
  using namespace seg;
  PlaceArgs a;
  if (fill_place(a, "bilinear_pad_fwd", dtype, N, Hi, Wi, C, Ho, Wo, Hd, Wd, top, left, ldx, ldy,
                 align_corners))
    return 1;
  SEG_REQUIRE(x && y, "bilinear_pad_fwd: null operand");
  SEG_REQUIRE((pro_mode & ~(PRO_AFFINE | PRO_RELU | PRO_CLAMP6)) == 0 &&
                  (((pro_mode & PRO_AFFINE) == 0) || (pro_scale && pro_shift)),
              "bilinear_pad_fwd: prologue mode %d / missing scale/shift", pro_mode);
  SEG_REQUIRE_FAST_DIV("bilinear_pad_fwd", (long)N * Hd * Wd, a.CV);
  SEG_REQUIRE((long)N * Hd * Wd * a.CV < (1L << 30), "bilinear_pad_fwd: too many vectors");
  a.x = x; a.y = y; a.mode = pro_mode; a.scale = pro_scale; a.shift = pro_shift;
  const int grid = grid_1d((long)N * Hd * Wd * a.CV, UN_THREADS, UN_MAX_BLOCKS);
  SEG_LAUNCH_T(bilinear_pad_fwd_kernel, dim3(grid), dim3(UN_THREADS), 0, stream, a);
  return check_launch("bilinear_pad_fwd");
}

// gx [N,Hi,Wi,C] (written) <- the Ho x Wo window at (top, left) of gy [N,Hd,Wd,C]
extern "C" int seg_bilinear_pad_bwd(int dtype, void* gx, long ldgx, int N, int Hi, int Wi, int C,
                                    const void* gy, long ldgy, int Ho, int Wo, int Hd, int Wd,
                                    int top, int left, int align_corners, void* stream) {
  using namespace seg;
  PlaceArgs a;
  if (fill_place(a, "bilinear_pad_bwd", dtype, N, Hi, Wi, C, Ho, Wo, Hd, Wd, top, left, ldgx, ldgy,
                 align_corners))
    return 1;
  SEG_REQUIRE(gx && gy, "bilinear_pad_bwd: null operand");
  SEG_REQUIRE_FAST_DIV("bilinear_pad_bwd", (long)N * Hi * Wi, a.CV);
  SEG_REQUIRE((long)N * Hi * Wi * a.CV < (1L << 30), "bilinear_pad_bwd: too many vectors");
  a.x = gx; a.y = const_cast<void*>(gy);
  const int grid = grid_1d((long)N * Hi * Wi * a.CV, UN_THREADS, UN_MAX_BLOCKS);
  SEG_LAUNCH_T(bilinear_pad_bwd_kernel, dim3(grid), dim3(UN_THREADS), 0, stream, a);
  return check_launch("bilinear_pad_bwd");
}
