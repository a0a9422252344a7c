// Channel attention ("squeeze / gate") on NHWC tensors: the operator BiSeNet's
// AttentionRefinmentModule and FeatureFusion are made of (segmentron/models/bisenet.py:106-186),
//     s = sigmoid(branch(mean_hw(act(x)))),   y = act(x) * s   resp.   act(x) + act(x) * s.
//   seg_apply_pool_fwd      y = act(x) written once + per-image channel sums of the fp32 activated
//                           values (nn.AdaptiveAvgPool2d(1) of a deferred activation), all images
//                           in one launch
//   seg_chan_gate_fwd       y = x * (identity + sigmoid(a[n][c])) + r + radd[n][c]
//   seg_chan_gate_bwd       dx = dy * (identity + sigmoid(a)) and partial rows of
//                           (sum_hw dy*x, sum_hw dy) in the same pass
//   seg_chan_gate_bwd_finalize   da = s(1-s) * sum dy*x,  dradd = sum dy
//   seg_bcast_add           g[n,h,w,c] (+)= v[n][c] * scale: the pool's backward joined to the
//                           gradient that reaches y
// All five are bandwidth kernels with one launch geometry: grid (channel-vector blocks, pixel
// chunks, images); a thread keeps ONE 16-byte channel vector of ONE image for its whole life, so
// the per-(n, c) gate — eight expf per bf16 vector — is computed once per thread instead of once
// per element, and the per-(n, c) sums live in registers.  A block reduces its rows through LDS
// in row order and writes one fp32 partial row; the chunks are summed in index order
// (seg_colsum / the finalize kernel).  No atomics: the same inputs give the same bits.
#include "rows.h"

namespace seg {

constexpr int CG_THREADS = ROWS_THREADS;
constexpr int CG_MAX_CHUNKS = 64;

struct ChanGateArgs {
  const void* x; const void* r; const void* dy; void* y;
  const float* a; const float* radd; const float* scale; const float* shift;
  float* partial;  // [chunks][N][K][C]
  long ldx, ldr, lddy, ldy, HW;
  int N, C, CV, cvb_log2, chunks, mode, identity;
  float vscale;
};

__device__ __forceinline__ float cg_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

template <typename T>
__global__ __launch_bounds__(CG_THREADS) void apply_pool_fwd_kernel(const ChanGateArgs a) {
  constexpr int VEC = Vec<T>::N;
  __shared__ __attribute__((aligned(16))) float smem[CG_THREADS * VEC];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2, spb = CG_THREADS >> a.cvb_log2;
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
    float s[VEC], t[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { s[e] = 1.f; t[e] = 0.f; }
    if (a.mode & PRO_AFFINE) {
      load_params<VEC>(a.scale, c0, s);
      load_params<VEC>(a.shift, c0, t);
    }
    const long step = (long)a.chunks * spb;
    for (long q = (long)blockIdx.y * spb + sy; q < a.HW; q += step) {
      const long row = (long)n * a.HW + q;
      float f[VEC];
      Vec<T>::unpack(ldg16(X + row * a.ldx + c0), f);
      apply_prologue_regs<VEC>(f, a.mode, s, t);
      if (Y != nullptr) stg16(Y + row * a.ldy + c0, Vec<T>::pack(f));
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[0][e] += f[e];
    }
  }
  rows_block_reduce<VEC, 1>(smem, acc, a.cvb_log2, blockIdx.x, a.C,
                            a.partial + ((long)blockIdx.y * a.N + n) * a.C, 0);
}

template <typename T>
__global__ __launch_bounds__(CG_THREADS) void chan_gate_fwd_kernel(const ChanGateArgs a) {
  constexpr int VEC = Vec<T>::N;
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2, spb = CG_THREADS >> a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int cv = blockIdx.x * cvb + cx;
  const int n = blockIdx.z;
  if (cv >= a.CV) return;
  const int c0 = cv * VEC;
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ R = reinterpret_cast<const T*>(a.r);
  T* __restrict__ Y = reinterpret_cast<T*>(a.y);
  float m[VEC], b[VEC];
  load_params<VEC>(a.a, n * a.C + c0, m);
#pragma unroll
  for (int e = 0; e < VEC; ++e) { m[e] = (float)a.identity + cg_sigmoid(m[e]); b[e] = 0.f; }
  if (a.radd != nullptr) load_params<VEC>(a.radd, n * a.C + c0, b);
  const long step = (long)a.chunks * spb;
  for (long q = (long)blockIdx.y * spb + sy; q < a.HW; q += step) {
    const long row = (long)n * a.HW + q;
    float f[VEC];
    Vec<T>::unpack(ldg16(X + row * a.ldx + c0), f);
#pragma unroll
    for (int e = 0; e < VEC; ++e) f[e] = f[e] * m[e];
    if (R != nullptr) {
      float rr[VEC];
      Vec<T>::unpack(ldg16(R + row * a.ldr + c0), rr);
#pragma unroll
      for (int e = 0; e < VEC; ++e) f[e] += rr[e];
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) f[e] += b[e];
    stg16(Y + row * a.ldy + c0, Vec<T>::pack(f));
  }
}

template <typename T>
__global__ __launch_bounds__(CG_THREADS) void chan_gate_bwd_kernel(const ChanGateArgs a) {
  constexpr int VEC = Vec<T>::N;
  __shared__ __attribute__((aligned(16))) float smem[2 * CG_THREADS * VEC];
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2, spb = CG_THREADS >> a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int cv = blockIdx.x * cvb + cx;
  const int n = blockIdx.z;
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ DY = reinterpret_cast<const T*>(a.dy);
  T* __restrict__ DX = reinterpret_cast<T*>(a.y);
  float acc[2][VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
  if (cv < a.CV) {
    const int c0 = cv * VEC;
    float m[VEC];
    load_params<VEC>(a.a, n * a.C + c0, m);
#pragma unroll
    for (int e = 0; e < VEC; ++e) m[e] = (float)a.identity + cg_sigmoid(m[e]);
    const long step = (long)a.chunks * spb;
    for (long q = (long)blockIdx.y * spb + sy; q < a.HW; q += step) {
      const long row = (long)n * a.HW + q;
      float g[VEC], f[VEC], d[VEC];
      Vec<T>::unpack(ldg16(DY + row * a.lddy + c0), g);
      Vec<T>::unpack(ldg16(X + row * a.ldx + c0), f);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        d[e] = g[e] * m[e];
        acc[0][e] = fmaf(g[e], f[e], acc[0][e]);
        acc[1][e] += g[e];
      }
      if (DX != nullptr) stg16(DX + row * a.ldy + c0, Vec<T>::pack(d));
    }
  }
  rows_block_reduce<VEC, 2>(smem, acc, a.cvb_log2, blockIdx.x, a.C,
                            a.partial + ((long)blockIdx.y * a.N + n) * 2 * a.C, a.C);
}

// partial [chunks][N][2][C] -> da[n][c] = s(1-s) * sum dy*x, dradd[n][c] = sum dy (nullable)
__global__ __launch_bounds__(CG_THREADS) void chan_gate_bwd_finalize_kernel(
    const float* __restrict__ partial, int chunks, int NC, int C, const float* __restrict__ a,
    float* __restrict__ da, float* __restrict__ dradd) {
  const int i = blockIdx.x * CG_THREADS + threadIdx.x;
  if (i >= NC) return;
  const int n = i / C, c = i - n * C;
  float s1 = 0.f, s2 = 0.f;
  for (int k = 0; k < chunks; ++k) {
    const float* row = partial + ((long)k * (NC / C) + n) * 2 * C;
    s1 += row[c];
    s2 += row[C + c];
  }
  const float s = cg_sigmoid(a[i]);
  if (da != nullptr) da[i] = s * (1.f - s) * s1;
  if (dradd != nullptr) dradd[i] = s2;
}

template <typename T>
__global__ __launch_bounds__(CG_THREADS) void bcast_add_kernel(const ChanGateArgs a) {
  constexpr int VEC = Vec<T>::N;
  const int tid = threadIdx.x;
  const int cvb = 1 << a.cvb_log2, spb = CG_THREADS >> a.cvb_log2;
  const int cx = tid & (cvb - 1), sy = tid >> a.cvb_log2;
  const int cv = blockIdx.x * cvb + cx;
  const int n = blockIdx.z;
  if (cv >= a.CV) return;
  const int c0 = cv * VEC;
  const T* G = reinterpret_cast<const T*>(a.x);  // (may be Y itself: in place)
  T* Y = reinterpret_cast<T*>(a.y);
  float v[VEC];
  load_params<VEC>(a.a, n * a.C + c0, v);
#pragma unroll
  for (int e = 0; e < VEC; ++e) v[e] *= a.vscale;
  const long step = (long)a.chunks * spb;
  for (long q = (long)blockIdx.y * spb + sy; q < a.HW; q += step) {
    const long row = (long)n * a.HW + q;
    float f[VEC];
    if (G != nullptr) {
      Vec<T>::unpack(ldg16(G + row * a.ldx + c0), f);
#pragma unroll
      for (int e = 0; e < VEC; ++e) f[e] += v[e];
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) f[e] = v[e];
    }
    stg16(Y + row * a.ldy + c0, Vec<T>::pack(f));
  }
}

static int cg_common(const char* what, int dtype, int N, long HW, int C, const long* lds, int nld,
                     int chunks, ChanGateArgs* a) {
  const int vec = dtype == DT_BF16 ? 8 : 4;
  if (rows_require(what, dtype, N, HW, C, vec, vec, lds, nullptr, nld, chunks, CG_MAX_CHUNKS))
    return 1;
  *a = ChanGateArgs();
  a->N = N; a->HW = HW; a->C = C; a->CV = C / vec; a->cvb_log2 = rows_pick_cvb_log2(a->CV, 0);
  a->chunks = chunks;
  return 0;
}

}  // namespace seg

// Pixel chunks per image of the launches below (rows of their partial buffers): enough blocks to
// fill the device, at least 32 pixels per chunk, at most 64 chunks.
extern "C" int seg_apply_pool_chunks(int N, long HW, int C) {
  if (N < 1 || HW < 1 || C < 1) return -1;
  return seg::rows_chunks(N, (C + 127) / 128, HW, 32, 1024, seg::CG_MAX_CHUNKS);
}

extern "C" int seg_apply_pool_fwd(int dtype, const void* x, long ldx, int pro_mode,
                                  const float* pro_scale, const float* pro_shift, void* y, long ldy,
                                  int N, long HW, int C, float* partial, int chunks,
                                  void* stream) {
  using namespace seg;
  ChanGateArgs a;
  const long lds[2] = {ldx, y != nullptr ? ldy : ldx};
  if (cg_common("apply_pool_fwd", dtype, N, HW, C, lds, 2, chunks, &a)) return 1;
  SEG_REQUIRE(x != nullptr && partial != nullptr, "apply_pool_fwd: null x / partial");
  SEG_REQUIRE(pro_mode >= 0 && pro_mode <= PRO_AFFINE_RELU, "apply_pool_fwd: bad prologue mode %d",
              pro_mode);
  SEG_REQUIRE(!(pro_mode & PRO_AFFINE) || (pro_scale != nullptr && pro_shift != nullptr),
              "apply_pool_fwd: affine prologue without scale / shift");
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.mode = pro_mode; a.scale = pro_scale;
  a.shift = pro_shift; a.partial = partial;
  SEG_LAUNCH_T(apply_pool_fwd_kernel, rows_grid(a.CV, a.cvb_log2, chunks, N), dim3(CG_THREADS), 0,
               stream, a);
  return check_launch("apply_pool_fwd");
}

extern "C" int seg_chan_gate_fwd(int dtype, const void* x, long ldx, const float* a_pre,
                                 int identity, const void* r, long ldr, const float* radd, void* y,
                                 long ldy, int N, long HW, int C, int chunks, void* stream) {
  using namespace seg;
  ChanGateArgs a;
  const long lds[3] = {ldx, ldy, r != nullptr ? ldr : ldx};
  if (cg_common("chan_gate_fwd", dtype, N, HW, C, lds, 3, chunks, &a)) return 1;
  SEG_REQUIRE(x != nullptr && y != nullptr && a_pre != nullptr, "chan_gate_fwd: null x / y / a");
  SEG_REQUIRE(identity == 0 || identity == 1, "chan_gate_fwd: identity must be 0 or 1");
  a.x = x; a.ldx = ldx; a.a = a_pre; a.identity = identity; a.r = r; a.ldr = ldr; a.radd = radd;
  a.y = y; a.ldy = ldy;
  SEG_LAUNCH_T(chan_gate_fwd_kernel, rows_grid(a.CV, a.cvb_log2, chunks, N), dim3(CG_THREADS), 0,
               stream, a);
  return check_launch("chan_gate_fwd");
}

// partial: fp32 [chunks][N][2][C] = (sum_hw dy*x, sum_hw dy); dx nullable (sums only)
extern "C" int seg_chan_gate_bwd(int dtype, const void* dy, long lddy, const void* x, long ldx,
                                 const float* a_pre, int identity, void* dx, long lddx, int N,
                                 long HW, int C, float* partial, int chunks, void* stream) {
  using namespace seg;
  ChanGateArgs a;
  const long lds[3] = {lddy, ldx, dx != nullptr ? lddx : ldx};
  if (cg_common("chan_gate_bwd", dtype, N, HW, C, lds, 3, chunks, &a)) return 1;
  SEG_REQUIRE(dy != nullptr && x != nullptr && a_pre != nullptr && partial != nullptr,
              "chan_gate_bwd: null dy / x / a / partial");
  SEG_REQUIRE(identity == 0 || identity == 1, "chan_gate_bwd: identity must be 0 or 1");
  a.dy = dy; a.lddy = lddy; a.x = x; a.ldx = ldx; a.a = a_pre; a.identity = identity; a.y = dx;
  a.ldy = lddx; a.partial = partial;
  SEG_LAUNCH_T(chan_gate_bwd_kernel, rows_grid(a.CV, a.cvb_log2, chunks, N), dim3(CG_THREADS), 0,
               stream, a);
  return check_launch("chan_gate_bwd");
}

extern "C" int seg_chan_gate_bwd_finalize(const float* partial, int chunks, int N, int C,
                                          const float* a_pre, float* da, float* dradd,
                                          void* stream) {
  using namespace seg;
  SEG_REQUIRE(partial != nullptr && a_pre != nullptr, "chan_gate_bwd_finalize: null partial / a");
  SEG_REQUIRE(chunks >= 1 && chunks <= CG_MAX_CHUNKS && N >= 1 && C >= 1 &&
                  (long)N * C < (1L << 31),
              "chan_gate_bwd_finalize: bad shape");
  const int NC = N * C;
  hipLaunchKernelGGL(chan_gate_bwd_finalize_kernel, dim3((NC + CG_THREADS - 1) / CG_THREADS),
                     dim3(CG_THREADS), 0, (hipStream_t)stream, partial, chunks, NC, C, a_pre, da,
                     dradd);
  return check_launch("chan_gate_bwd_finalize");
}

// y[n,p,c] = (g nullable: g[n,p,c]) + v[n][c] * scale; y may be g itself
extern "C" int seg_bcast_add(int dtype, const void* g, long ldg, const float* v, float scale,
                             void* y, long ldy, int N, long HW, int C, int chunks, void* stream) {
  using namespace seg;
  ChanGateArgs a;
  const long lds[2] = {ldy, g != nullptr ? ldg : ldy};
  if (cg_common("bcast_add", dtype, N, HW, C, lds, 2, chunks, &a)) return 1;
  SEG_REQUIRE(y != nullptr && v != nullptr, "bcast_add: null y / v");
  a.x = g; a.ldx = ldg; a.a = v; a.vscale = scale; a.y = y; a.ldy = ldy;
  SEG_LAUNCH_T(bcast_add_kernel, rows_grid(a.CV, a.cvb_log2, chunks, N), dim3(CG_THREADS), 0,
               stream, a);
  return check_launch("bcast_add");
}
