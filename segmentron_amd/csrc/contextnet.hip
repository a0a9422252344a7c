// ContextNet (segmentron/models/contextnet.py:165-188): FeatureFusionModule resizes the 1/32 map to
// the 1/8 map's size and runs a depthwise 3x3 on the result.  The upsampled map U holds 16 times the
// pixels of the map it is computed from; here it never reaches memory.
//
//   seg_up_dw_fwd   y = depthwise 3x3 (zero padding 1 around U) of U = bilinear(act(lo), (H, W)).
//       U is recomputed from the cache-resident lo, in fp32, and is never rounded to the activation
//       dtype.  Optional BatchNorm statistics rows [rows][2][C] (sum | sum of squares of the fp32
//       outputs), the layout seg_bn_finalize_p takes.
//   seg_up_dw_bwd   one pass over dy and lo: d_up = correlation of dy with the flipped taps (what
//       seg_bilinear_bwd takes next) and the weight-gradient rows [rows][9][C] with U recomputed,
//       the layout seg_dwconv3x3_wgrad_finalize takes.
//
// Both are sliding kernels in the manner of dwconv_slide.hip: a thread owns one image column x four
// channels and slides down a strip of rows with a 3 x 3 window of fp32 vectors in registers.  Per
// step it produces ONE new vector of the row that enters the window (forward: four taps of lo, the
// prologue, the blend of resize.hip; backward: one load of dy), hands it to its two column
// neighbours through a double-buffered LDS row (one barrier per step) and issues the nine taps.
// The first and the last column lane of a block are halo lanes: they feed their neighbour and
// store nothing, so a block of `ncol` column lanes writes ncol - 2 columns.  Zero padding is a zero
// vector of the window (a column or row outside the map), never a tap of lo.
//
// Geometry (ud_geom, shared by the launchers and the host query seg_up_dw_rows): cvb = 2^cvb_log2
// channel-quad lanes (rows_fit_cvb_log2, 16 at the most: 64 channels), ncol = 256 / cvb column
// lanes; grid = (channel blocks x column blocks, row strips, images); one partial row per (image,
// strip, column block), summed in lane order through rows_block_reduce: no atomics, the same bits
// on every launch.
#include "rows.h"
#include "resize_taps.h"

namespace seg {

constexpr int UD_THREADS = ROWS_THREADS;
constexpr int UD_MAX_LANES_LOG2 = 4;    // channel-quad lanes of a block: 64 channels at the most
constexpr long UD_TARGET_BLOCKS = 1024;  // about four blocks per CU
constexpr long UD_MIN_STRIP = 4;         // rows of a strip: two halo rows are recomputed per strip
constexpr int UD_Q = 4;                  // channels per thread

struct UpDwGeom { int cvb_log2, ncol, nwblk, ncblk, rs, nstrips; };

static inline UpDwGeom ud_geom(int N, int H, int W, int C) {
  UpDwGeom g;
  g.cvb_log2 = rows_fit_cvb_log2(C / UD_Q, UD_MAX_LANES_LOG2);
  g.ncol = UD_THREADS >> g.cvb_log2;
  const int outc = g.ncol - 2;
  g.nwblk = (W + outc - 1) / outc;
  g.ncblk = rows_gx(C / UD_Q, g.cvb_log2);
  const int strips = rows_chunks(1, (long)N * g.nwblk * g.ncblk, H, UD_MIN_STRIP, UD_TARGET_BLOCKS,
                                 65535);
  g.rs = (H + strips - 1) / strips;
  g.nstrips = (H + g.rs - 1) / g.rs;
  return g;
}

struct UpDwArgs {
  const void* lo; const void* dy;  // dy: backward only
  void* y;                         // forward: the output; backward: d_up
  const float* w;                  // [9][C] tap-major
  const float* scale; const float* shift;
  float* partial;                  // forward: [rows][2][C] or null; backward: [rows][9][C]
  long ldlo, lddy, ldy;
  int N, h, w_lo, H, W, C, mode, align;
  int cvb_log2, ncol, ncblk, nwblk, rs;
  float sh, sw;
};

// what a thread is: its channel quad, its column and the column's two source taps
struct UdThread {
  int cq, wl, cblk, wblk, c, X, w0, w1, lcol, rcol, r0, r1;
  float lw;
  bool colok, outok;
};
__device__ __forceinline__ UdThread ud_thread(const UpDwArgs& a) {
  UdThread t;
  const int tid = threadIdx.x, cvb = 1 << a.cvb_log2;
  t.cq = tid & (cvb - 1);
  t.wl = tid >> a.cvb_log2;
  t.cblk = blockIdx.x % a.ncblk;
  t.wblk = blockIdx.x / a.ncblk;
  const int cfull = (t.cblk * cvb + t.cq) * UD_Q;
  const bool cok = cfull < a.C;
  t.c = cok ? cfull : a.C - UD_Q;  // (lanes past the last quad mirror it and store nothing)
  t.X = t.wblk * (a.ncol - 2) + t.wl - 1;
  t.colok = t.X >= 0 && t.X < a.W;
  t.outok = cok && t.colok && t.wl >= 1 && t.wl <= a.ncol - 2;
  t.w0 = t.w1 = 0;
  t.lw = 0.f;
  if (t.colok) taps(a.sw, t.X, a.w_lo, a.align, t.w0, t.w1, t.lw);
  t.lcol = max(t.wl - 1, 0);
  t.rcol = min(t.wl + 1, a.ncol - 1);
  t.r0 = blockIdx.y * a.rs;
  t.r1 = min(a.H, t.r0 + a.rs);
  return t;
}

__device__ __forceinline__ void ud_load4(const float* __restrict__ p, float (&f)[UD_Q]) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
}

// U[n, r, X, c .. c+3] in fp32: zero outside the map, else the blend of resize.hip on the four
// activated source taps (the same expression and association)
template <typename T>
__device__ __forceinline__ void ud_up(const UpDwArgs& a, const UdThread& t,
                                      const T* __restrict__ lo_n, int r, const float (&s)[UD_Q],
                                      const float (&sh)[UD_Q], float (&u)[UD_Q]) {
#pragma unroll
  for (int e = 0; e < UD_Q; ++e) u[e] = 0.f;
  if (!t.colok || r < 0 || r >= a.H) return;
  int h0, h1; float lh;
  taps(a.sh, r, a.h, a.align, h0, h1, lh);
  const T* __restrict__ ra = lo_n + (long)h0 * a.w_lo * a.ldlo + t.c;
  const T* __restrict__ rb = lo_n + (long)h1 * a.w_lo * a.ldlo + t.c;
  float f00[UD_Q], f01[UD_Q], f10[UD_Q], f11[UD_Q];
  HVec<T>::load(ra + (long)t.w0 * a.ldlo, f00);
  HVec<T>::load(ra + (long)t.w1 * a.ldlo, f01);
  HVec<T>::load(rb + (long)t.w0 * a.ldlo, f10);
  HVec<T>::load(rb + (long)t.w1 * a.ldlo, f11);
  apply_prologue_regs<UD_Q>(f00, a.mode, s, sh);
  apply_prologue_regs<UD_Q>(f01, a.mode, s, sh);
  apply_prologue_regs<UD_Q>(f10, a.mode, s, sh);
  apply_prologue_regs<UD_Q>(f11, a.mode, s, sh);
  const float lw = t.lw;
#pragma unroll
  for (int e = 0; e < UD_Q; ++e) {
    const float up = (1.f - lw) * f00[e] + lw * f01[e];
    const float dn = (1.f - lw) * f10[e] + lw * f11[e];
    u[e] = (1.f - lh) * up + lh * dn;
  }
}

// the row that enters the window: own vector -> LDS, barrier, the neighbours' vectors back.  buf is
// the step's half of the double buffer: a thread overwrites a half two steps later, behind the
// barrier of the step in between, which every thread reaches after it has read this one.
__device__ __forceinline__ void ud_exchange(float* buf, const UdThread& t, int cvb_log2,
                                            const float (&v)[UD_Q], float (&row)[3][UD_Q]) {
  *reinterpret_cast<float4*>(buf + threadIdx.x * UD_Q) = make_float4(v[0], v[1], v[2], v[3]);
  __syncthreads();
  ud_load4(buf + ((t.lcol << cvb_log2) + t.cq) * UD_Q, row[0]);
  ud_load4(buf + ((t.rcol << cvb_log2) + t.cq) * UD_Q, row[2]);
#pragma unroll
  for (int e = 0; e < UD_Q; ++e) row[1][e] = v[e];
}

__device__ __forceinline__ void ud_params(const UpDwArgs& a, int c, float (&s)[UD_Q],
                                          float (&sh)[UD_Q], float (&wt)[9][UD_Q]) {
#pragma unroll
  for (int e = 0; e < UD_Q; ++e) { s[e] = 1.f; sh[e] = 0.f; }
  if (a.mode & PRO_AFFINE) {
    load_params<UD_Q>(a.scale, c, s);
    load_params<UD_Q>(a.shift, c, sh);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) ud_load4(a.w + (long)k * a.C + c, wt[k]);
}

template <typename T>
__global__ __launch_bounds__(UD_THREADS) void up_dw_fwd_kernel(const UpDwArgs a) {
  __shared__ float xch[2][UD_THREADS * UD_Q];
  __shared__ float red[2 * UD_THREADS * UD_Q];
  const UdThread t = ud_thread(a);
  const int n = blockIdx.z;
  const T* __restrict__ lo_n = reinterpret_cast<const T*>(a.lo) + (long)n * a.h * a.w_lo * a.ldlo;
  T* __restrict__ Y = reinterpret_cast<T*>(a.y);
  float s[UD_Q], sh[UD_Q], wt[9][UD_Q];
  ud_params(a, t.c, s, sh, wt);
  float win[3][3][UD_Q], acc[2][UD_Q];  // acc: sum, sum of squares
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int e = 0; e < UD_Q; ++e) win[i][j][e] = 0.f;
#pragma unroll
  for (int e = 0; e < UD_Q; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }

  for (int r = t.r0 - 1; r <= t.r1; ++r) {  // the upsampled row r enters; output row r - 1 leaves
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int e = 0; e < UD_Q; ++e) { win[0][j][e] = win[1][j][e]; win[1][j][e] = win[2][j][e]; }
    float u[UD_Q];
    ud_up<T>(a, t, lo_n, r, s, sh, u);
    ud_exchange(xch[(r - t.r0 + 1) & 1], t, a.cvb_log2, u, win[2]);
    if (r - 1 < t.r0) continue;  // (uniform in the block)
    float o[UD_Q];
#pragma unroll
    for (int e = 0; e < UD_Q; ++e) o[e] = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int e = 0; e < UD_Q; ++e) o[e] = fmaf(win[i][j][e], wt[i * 3 + j][e], o[e]);
    if (t.outok) {
      HVec<T>::store(Y + (((long)n * a.H + (r - 1)) * a.W + t.X) * a.ldy + t.c, o);
#pragma unroll
      for (int e = 0; e < UD_Q; ++e) {
        acc[0][e] += o[e];
        acc[1][e] = fmaf(o[e], o[e], acc[1][e]);
      }
    }
  }
  if (a.partial != nullptr) {
    const long prow = ((long)n * gridDim.y + blockIdx.y) * a.nwblk + t.wblk;
    rows_block_reduce<UD_Q, 2, UD_THREADS>(red, acc, a.cvb_log2, t.cblk, a.C,
                                           a.partial + prow * 2 * a.C, a.C);
  }
}

// The window holds dy; position (i, j) of the window pairs with tap 8 - (3 i + j):
//   d_up[P, Q] = sum_ij dy[P + i - 1, Q + j - 1] * w[8 - (3 i + j)]
//   dW[8 - (3 i + j)] += U[P, Q] * dy[P + i - 1, Q + j - 1]
template <typename T>
__global__ __launch_bounds__(UD_THREADS) void up_dw_bwd_kernel(const UpDwArgs a) {
  __shared__ float xch[2][UD_THREADS * UD_Q];
  __shared__ float red[9 * UD_THREADS * UD_Q];
  const UdThread t = ud_thread(a);
  const int n = blockIdx.z;
  const T* __restrict__ lo_n = reinterpret_cast<const T*>(a.lo) + (long)n * a.h * a.w_lo * a.ldlo;
  const T* __restrict__ DY = reinterpret_cast<const T*>(a.dy);
  T* __restrict__ G = reinterpret_cast<T*>(a.y);
  float s[UD_Q], sh[UD_Q], wt[9][UD_Q];
  ud_params(a, t.c, s, sh, wt);
  float win[3][3][UD_Q], dw[9][UD_Q];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int e = 0; e < UD_Q; ++e) { win[i][j][e] = 0.f; dw[i * 3 + j][e] = 0.f; }

  for (int r = t.r0 - 1; r <= t.r1; ++r) {  // row r of dy enters; row r - 1 of d_up leaves
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int e = 0; e < UD_Q; ++e) { win[0][j][e] = win[1][j][e]; win[1][j][e] = win[2][j][e]; }
    float g[UD_Q];
#pragma unroll
    for (int e = 0; e < UD_Q; ++e) g[e] = 0.f;
    if (t.colok && r >= 0 && r < a.H)
      HVec<T>::load(DY + (((long)n * a.H + r) * a.W + t.X) * a.lddy + t.c, g);
    ud_exchange(xch[(r - t.r0 + 1) & 1], t, a.cvb_log2, g, win[2]);
    if (r - 1 < t.r0) continue;  // (uniform in the block)
    if (t.outok) {
      float u[UD_Q], o[UD_Q];
      ud_up<T>(a, t, lo_n, r - 1, s, sh, u);
#pragma unroll
      for (int e = 0; e < UD_Q; ++e) o[e] = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
          for (int e = 0; e < UD_Q; ++e) {
            o[e] = fmaf(win[i][j][e], wt[8 - (3 * i + j)][e], o[e]);
            dw[8 - (3 * i + j)][e] = fmaf(u[e], win[i][j][e], dw[8 - (3 * i + j)][e]);
          }
      HVec<T>::store(G + (((long)n * a.H + (r - 1)) * a.W + t.X) * a.ldy + t.c, o);
    }
  }
  const long prow = ((long)n * gridDim.y + blockIdx.y) * a.nwblk + t.wblk;
  rows_block_reduce<UD_Q, 9, UD_THREADS>(red, dw, a.cvb_log2, t.cblk, a.C,
                                         a.partial + prow * 9 * a.C, a.C);
}

static bool ud_shape_ok(int dtype, int N, int H, int W, int C) {
  if ((dtype != DT_F32 && dtype != DT_BF16) || N < 1 || N > 65535 || H < 1 || W < 1) return false;
  const int vec = dtype == DT_BF16 ? 8 : 4;
  return C >= vec && C % vec == 0 && (long)N * H * W < (1L << 31) / 16;
}

static int fill_up_dw(UpDwArgs& a, UpDwGeom& g, const char* what, int dtype, const void* lo,
                      long ldlo, int N, int h, int w, int C, int pro_mode, const float* pro_scale,
                      const float* pro_shift, const float* w9c, int H, int W, int align,
                      int rows) {
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(ud_shape_ok(dtype, N, H, W, C) && h >= 1 && w >= 1,
              "%s: bad dtype %d / shape N=%d %dx%d -> %dx%d C=%d (C a positive multiple of %d)",
              what, dtype, N, h, w, H, W, C, vec);
  SEG_REQUIRE(lo && w9c, "%s: null operand", what);
  SEG_REQUIRE(ldlo >= C && ldlo % vec == 0, "%s: the low map's pitch %ld is no multiple of %d "
              "that holds %d channels", what, ldlo, vec, C);
  SEG_REQUIRE((pro_mode & ~(PRO_AFFINE | PRO_RELU | PRO_CLAMP6)) == 0 &&
                  (((pro_mode & PRO_AFFINE) == 0) || (pro_scale && pro_shift)),
              "%s: prologue mode %d / missing scale/shift", what, pro_mode);
  g = ud_geom(N, H, W, C);
  SEG_REQUIRE(g.nstrips <= 65535 && (long)g.ncblk * g.nwblk < (1L << 31),
              "%s: beyond the launch grid", what);
  SEG_REQUIRE(rows == N * g.nstrips * g.nwblk, "%s: %d partial rows, seg_up_dw_rows says %d", what,
              rows, N * g.nstrips * g.nwblk);
  a.lo = lo; a.dy = nullptr; a.y = nullptr; a.w = w9c; a.scale = pro_scale; a.shift = pro_shift;
  a.partial = nullptr; a.ldlo = ldlo; a.lddy = a.ldy = 0;
  a.N = N; a.h = h; a.w_lo = w; a.H = H; a.W = W; a.C = C; a.mode = pro_mode; a.align = align;
  a.cvb_log2 = g.cvb_log2; a.ncol = g.ncol; a.ncblk = g.ncblk; a.nwblk = g.nwblk; a.rs = g.rs;
  a.sh = host_scale(h, H, align); a.sw = host_scale(w, W, align);
  return 0;
}

}  // namespace seg

// partial rows of seg_up_dw_fwd's statistics (kind 0) and seg_up_dw_bwd's weight gradient (kind 1):
// one per (image, row strip, column block) in both; 0: bad arguments.  Pure host.
extern "C" int seg_up_dw_rows(int dtype, int N, int H, int W, int C, int kind) {
  using namespace seg;
  if (!ud_shape_ok(dtype, N, H, W, C) || (kind != 0 && kind != 1)) return 0;
  const UpDwGeom g = ud_geom(N, H, W, C);
  const long r = (long)N * g.nstrips * g.nwblk;
  return r < (1L << 31) ? (int)r : 0;
}

extern "C" int seg_up_dw_fwd(int dtype, const void* lo, long ldlo, int N, int h, int w, int C,
                             int pro_mode, const float* pro_scale, const float* pro_shift,
                             const float* w9c, void* y, long ldy, int H, int W, int align_corners,
                             float* stat_partial, int rows, void* stream) {
  using namespace seg;
  UpDwArgs a;
  UpDwGeom g;
  if (fill_up_dw(a, g, "up_dw_fwd", dtype, lo, ldlo, N, h, w, C, pro_mode, pro_scale, pro_shift,
                 w9c, H, W, align_corners, rows))
    return 1;
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(y != nullptr && ldy >= C && ldy % vec == 0,
              "up_dw_fwd: null output / its pitch %ld is no multiple of %d that holds C", ldy, vec);
  a.y = y; a.ldy = ldy; a.partial = stat_partial;
  const dim3 grid(g.ncblk * g.nwblk, g.nstrips, N);
  SEG_LAUNCH_T(up_dw_fwd_kernel, grid, dim3(UD_THREADS), 0, stream, a);
  return check_launch("up_dw_fwd");
}

extern "C" int seg_up_dw_bwd(int dtype, const void* dy, long lddy, const void* lo, long ldlo, int N,
                             int h, int w, int C, int pro_mode, const float* pro_scale,
                             const float* pro_shift, const float* w9c, void* d_up, long ldd, int H,
                             int W, int align_corners, float* partial_w, int rows, void* stream) {
  using namespace seg;
  UpDwArgs a;
  UpDwGeom g;
  if (fill_up_dw(a, g, "up_dw_bwd", dtype, lo, ldlo, N, h, w, C, pro_mode, pro_scale, pro_shift,
                 w9c, H, W, align_corners, rows))
    return 1;
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(dy && d_up && partial_w, "up_dw_bwd: null operand");
  SEG_REQUIRE(lddy >= C && lddy % vec == 0 && ldd >= C && ldd % vec == 0,
              "up_dw_bwd: pitches %ld / %ld are multiples of %d, at least C", lddy, ldd, vec);
  a.dy = dy; a.lddy = lddy; a.y = d_up; a.ldy = ldd; a.partial = partial_w;
  const dim3 grid(g.ncblk * g.nwblk, g.nstrips, N);
  SEG_LAUNCH_T(up_dw_bwd_kernel, grid, dim3(UD_THREADS), 0, stream, a);
  return check_launch("up_dw_bwd");
}
