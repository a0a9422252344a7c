// A PAIR of 3-tap line convolutions in one launch (EDANet's EDABlock, segmentron/models/edanet.py:
// 127-128 and 132-133: conv3x1 -> conv1x3 with nothing but the first bias in between), C == O == 40:
//
//   mid = lineA(act(x)) + biasA        (rounded to the tensor dtype exactly as a store rounds it)
//   y   = lineB(mid) + biasB (+ add)
//
// Axes (A, B) = (H, W) (order 0) or (W, H) (order 1), one dilation for both.  One block (4 waves)
// owns one whole line along axis B — a row (n, h) for order 0, a column (n, w) for order 1 — so
// stage B needs no halo of `mid`: stage A is the MFMA scheme of conv_line.hip (B fragments are
// 16-byte channel vectors straight from global memory, three lines at -d, 0, +d along A) and writes
// the `mid` line to LDS (and to global memory where `mid` is non-null: training needs it for both
// weight gradients); after one __syncthreads stage B takes its three taps from LDS.  A tap outside
// the line is zero AFTER biasA.  Both weight sets live in LDS for the block's lifetime.
// The MFMA sequence of every accumulator (k-steps outer, taps inner) and every rounding are those
// of conv_line_kernel, so y and mid are bit-identical to the two single launches.
// Outputs: y (pitched), statistics of y as stored (nullable, one row [2][C] per block), per-channel
// sums of mid as stored (nullable, one row [C] per block).  No atomics, fixed summation order.
// The data gradient of an (H, W) pair is the (W, H) pair on dy with the weights repacked
// [C][2-t][O] and no biases: its `mid` is the gradient with respect to the forward `mid` and its
// mid sums are the first convolution's bias gradient.
#include "conv_gemm.h"

namespace seg {

constexpr int LP_THREADS = 256, LP_WAVES = 4, LP_C = 40, LP_MAX_BLOCKS = 1024;
constexpr int LP_LDS_BUDGET = 64 * 1024;

struct PairArgs {
  const void* x; long ldx;
  const void* wa; const void* wb;
  const float* ba; const float* bb;  // nullable, [C]
  void* mid; long ldmid;             // nullable
  void* y; long ldy;
  const void* add; long ldadd;       // nullable
  const float* ps; const float* pt; int pro_mode;
  float* stat; float* midsum;        // nullable
  int H, W, order, d;
  int lines, L;
};

template <typename T> struct PairGeom {
  static constexpr int C = LP_C;
  static constexpr int VEC = Vec<T>::N;
  static constexpr int KSTEP = 2 * VEC;
  static constexpr int KS = (C + KSTEP - 1) / KSTEP;
  static constexpr bool KTAIL = C % KSTEP != 0;
  // (bf16: 272 B = 68 words per weight row, so that 32 rows at one offset spread over the banks)
  static constexpr int WPITCH = 3 * C * (int)sizeof(T) + (sizeof(T) == 2 ? 32 : 16);
  static constexpr int MPITCH = C * (int)sizeof(T) + 16;
  static constexpr int RED_BYTES = LP_WAVES * 3 * C * 4;
  static constexpr int FIXED_BYTES = RED_BYTES + 2 * C * WPITCH;
};

static int pair_lds_bytes(int dtype, int L) {
  return dtype == DT_BF16 ? PairGeom<bf16_t>::FIXED_BYTES + L * PairGeom<bf16_t>::MPITCH
                          : PairGeom<float>::FIXED_BYTES + L * PairGeom<float>::MPITCH;
}

// the 4 values of a lane's channel group as the store rounds them
template <typename T> __device__ __forceinline__ void lp_round(float* f);
template <> __device__ __forceinline__ void lp_round<float>(float*) {}
template <> __device__ __forceinline__ void lp_round<bf16_t>(float* f) {
  const uint32_t a = pack_bf16x2(f[0], f[1]), b = pack_bf16x2(f[2], f[3]);
  f[0] = __uint_as_float(a << 16); f[1] = __uint_as_float(a & 0xFFFF0000u);
  f[2] = __uint_as_float(b << 16); f[3] = __uint_as_float(b & 0xFFFF0000u);
}

// acc[og] += sum over k-steps (outer) and taps (inner) of W[og] x B, as conv_line_kernel
template <typename T>
__device__ __forceinline__ void lp_mma(const unsigned char* wl, const uint4 (&b)[3][PairGeom<T>::KS],
                                       int r32, int h, f32x16 (&acc)[2]) {
  using G = PairGeom<T>;
  constexpr int C = G::C, VEC = G::VEC;
#pragma unroll
  for (int og = 0; og < 2; ++og)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[og][e] = 0.f;
#pragma unroll
  for (int ks = 0; ks < G::KS; ++ks) {
    const bool kv = !G::KTAIL || ks * G::KSTEP + h * VEC < C;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
#pragma unroll
      for (int og = 0; og < 2; ++og) {
        const bool orow = og * 32 + r32 < C;
        const int k = kv ? t * C + ks * G::KSTEP + h * VEC : 0;
        const uint4 wv = mask_u4(*reinterpret_cast<const uint4*>(
                                     wl + (orow ? og * 32 + r32 : 0) * G::WPITCH + k * (int)sizeof(T)),
                                 orow && kv);
        Mma<T>::step(wv, b[t][ks], acc[og]);
      }
    }
  }
}

template <typename T, bool PRO>
__global__ __launch_bounds__(LP_THREADS) void conv_line_pair_kernel(const PairArgs a) {
  using G = PairGeom<T>;
  constexpr int C = G::C, VEC = G::VEC, KS = G::KS;
  extern __shared__ __attribute__((aligned(16))) unsigned char lp_smem[];
  float* red = reinterpret_cast<float*>(lp_smem);
  unsigned char* wla = lp_smem + G::RED_BYTES;
  unsigned char* wlb = wla + C * G::WPITCH;
  unsigned char* ml = wlb + C * G::WPITCH;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, h = lane >> 5;
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ A = reinterpret_cast<const T*>(a.add);
  T* __restrict__ Y = reinterpret_cast<T*>(a.y);
  T* __restrict__ M = reinterpret_cast<T*>(a.mid);

  {  // both weight sets -> LDS
    constexpr int VPR = 3 * C / VEC;
    for (int i = tid; i < 2 * C * VPR; i += LP_THREADS) {
      const int which = i / (C * VPR), j = i - which * (C * VPR);
      const int o = j / VPR, v = j - o * VPR;
      const T* src = reinterpret_cast<const T*>(which ? a.wb : a.wa);
      *reinterpret_cast<uint4*>((which ? wlb : wla) + o * G::WPITCH + v * 16) =
          ldg16(src + (long)o * (3 * C) + v * VEC);
    }
  }

  float s1[2][16], s2[2][16], sm[2][16];
#pragma unroll
  for (int og = 0; og < 2; ++og)
#pragma unroll
    for (int e = 0; e < 16; ++e) s1[og][e] = s2[og][e] = sm[og][e] = 0.f;

  const int ngrp = (a.L + 31) / 32;
  for (int line = blockIdx.x; line < a.lines; line += gridDim.x) {
    __syncthreads();  // the weights are in LDS / the previous line's `mid` is consumed
    long p0, sB, sA;
    int posA, limA;
    if (a.order == 0) {
      p0 = (long)line * a.W; sB = 1; sA = a.W; posA = line % a.H; limA = a.H;
    } else {
      const int n = line / a.W, w = line - n * a.W;
      p0 = (long)n * a.H * a.W + w; sB = a.W; sA = 1; posA = w; limA = a.W;
    }
    // ---- stage A: mid = lineA(act(x)) + biasA -> LDS (and global)
    for (int grp = wave; grp < ngrp; grp += LP_WAVES) {
      const int i = grp * 32 + r32;
      const bool pv = i < a.L;
      const long p = p0 + (long)(pv ? i : 0) * sB;
      uint4 b[3][KS];
      bool ok[3];
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const long q = (long)posA + (long)(t - 1) * a.d;
        ok[t] = pv && q >= 0 && q < limA;
        const long off = (p + (ok[t] ? (long)(t - 1) * a.d * sA : 0)) * a.ldx + h * VEC;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bool kv = !G::KTAIL || ks * G::KSTEP + h * VEC < C;
          b[t][ks] = ldg16(X + off + (kv ? ks * G::KSTEP : -h * VEC));
        }
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bool kv = !G::KTAIL || ks * G::KSTEP + h * VEC < C;
        float ps[VEC], pt[VEC];
        if (PRO && (a.pro_mode & PRO_AFFINE) && kv) {
          load_params<VEC>(a.ps, ks * G::KSTEP + h * VEC, ps);
          load_params<VEC>(a.pt, ks * G::KSTEP + h * VEC, pt);
        } else {
#pragma unroll
          for (int k = 0; k < VEC; ++k) { ps[k] = 1.f; pt[k] = 0.f; }
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          uint4 v = b[t][ks];
          if (PRO) {
            float f[VEC];
            Vec<T>::unpack(v, f);
            apply_prologue_regs<VEC>(f, a.pro_mode, ps, pt);
            v = Vec<T>::pack(f);
          }
          b[t][ks] = mask_u4(v, ok[t] && kv);
        }
      }
      f32x16 acc[2];
      lp_mma<T>(wla, b, r32, h, acc);
#pragma unroll
      for (int og = 0; og < 2; ++og)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ch = og * 32 + g * 8 + h * 4;
          if (ch >= C) continue;
          float f[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) f[j] = acc[og][g * 4 + j];
          if (a.ba != nullptr) {
            float bv[4];
            load_params<4>(a.ba, ch, bv);
#pragma unroll
            for (int j = 0; j < 4; ++j) f[j] += bv[j];
          }
          lp_round<T>(f);
          if (pv) {
            HVec<T>::store(reinterpret_cast<T*>(ml + (long)i * G::MPITCH) + ch, f);
            if (M != nullptr) HVec<T>::store(M + p * a.ldmid + ch, f);
#pragma unroll
            for (int j = 0; j < 4; ++j) sm[og][g * 4 + j] += f[j];
          }
        }
    }
    __syncthreads();
    // ---- stage B: y = lineB(mid) + biasB (+ add), taps from LDS, zero outside the line
    for (int grp = wave; grp < ngrp; grp += LP_WAVES) {
      const int i = grp * 32 + r32;
      const bool pv = i < a.L;
      const long p = p0 + (long)(pv ? i : 0) * sB;
      uint4 b[3][KS];
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const long q = (long)i + (long)(t - 1) * a.d;
        const bool ok = pv && q >= 0 && q < a.L;
        const unsigned char* row = ml + (ok ? q : 0) * G::MPITCH;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bool kv = !G::KTAIL || ks * G::KSTEP + h * VEC < C;
          b[t][ks] = mask_u4(*reinterpret_cast<const uint4*>(
                                 row + (kv ? ks * G::KSTEP + h * VEC : 0) * (int)sizeof(T)),
                             ok && kv);
        }
      }
      f32x16 acc[2];
      lp_mma<T>(wlb, b, r32, h, acc);
#pragma unroll
      for (int og = 0; og < 2; ++og)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ch = og * 32 + g * 8 + h * 4;
          if (ch >= C) continue;
          float f[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) f[j] = acc[og][g * 4 + j];
          if (a.bb != nullptr) {
            float bv[4];
            load_params<4>(a.bb, ch, bv);
#pragma unroll
            for (int j = 0; j < 4; ++j) f[j] += bv[j];
          }
          if (A != nullptr) {
            float av[4];
            HVec<T>::load(A + p * a.ldadd + ch, av);
#pragma unroll
            for (int j = 0; j < 4; ++j) f[j] += av[j];
          }
          lp_round<T>(f);
          if (pv) {
            HVec<T>::store(Y + p * a.ldy + ch, f);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              s1[og][g * 4 + j] += f[j];
              s2[og][g * 4 + j] = fmaf(f[j], f[j], s2[og][g * 4 + j]);
            }
          }
        }
    }
  }

  if (a.stat == nullptr && a.midsum == nullptr) return;
  // lanes with the same h hold the same channels: fold bits 0..4, then the waves through LDS
#pragma unroll
  for (int og = 0; og < 2; ++og)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
#pragma unroll
      for (int m = 1; m < 32; m <<= 1) {
        s1[og][e] += __shfl_xor(s1[og][e], m, 64);
        s2[og][e] += __shfl_xor(s2[og][e], m, 64);
        sm[og][e] += __shfl_xor(sm[og][e], m, 64);
      }
    }
  if (r32 == 0) {
#pragma unroll
    for (int og = 0; og < 2; ++og)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int ch = og * 32 + (e >> 2) * 8 + h * 4 + (e & 3);
        if (ch < C) {
          red[(wave * 3 + 0) * C + ch] = s1[og][e];
          red[(wave * 3 + 1) * C + ch] = s2[og][e];
          red[(wave * 3 + 2) * C + ch] = sm[og][e];
        }
      }
  }
  __syncthreads();
  if (tid < 3 * C) {
    float s = 0.f;
    for (int w = 0; w < LP_WAVES; ++w) s += red[w * 3 * C + tid];
    if (tid < 2 * C) {
      if (a.stat != nullptr) a.stat[(long)blockIdx.x * 2 * C + tid] = s;
    } else if (a.midsum != nullptr) {
      a.midsum[(long)blockIdx.x * C + tid - 2 * C] = s;
    }
  }
}

static bool pair_ok(int dtype, int C, int L, int dil) {
  return (dtype == DT_F32 || dtype == DT_BF16) && C == LP_C && L >= 1 && L < (1 << 20) &&
         dil >= 1 && dil < (1 << 20) && pair_lds_bytes(dtype, L) <= LP_LDS_BUDGET;
}

static int pair_grid(long lines) { return (int)(lines < LP_MAX_BLOCKS ? lines : LP_MAX_BLOCKS); }

}  // namespace seg

extern "C" int seg_conv_line_pair_ok(int dtype, int C, int L, int dil) {
  return seg::pair_ok(dtype, C, L, dil) ? 1 : 0;
}

// rows of stat_partial / mid_sums (= blocks) for [N,H,W] and an axis order; -1 on bad input
extern "C" int seg_conv_line_pair_rows(int N, int H, int W, int order) {
  if (N < 1 || H < 1 || W < 1 || (order != 0 && order != 1) || (long)N * H * W >= (1L << 31))
    return -1;
  return seg::pair_grid((long)N * (order == 0 ? H : W));
}

extern "C" int seg_conv_line_pair_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                                      const void* wa, const float* bias_a, const void* wb,
                                      const float* bias_b, int order, int dil, int pro_mode,
                                      const float* pro_scale, const float* pro_shift, void* mid,
                                      long ldmid, void* y, long ldy, const void* add, long ldadd,
                                      float* stat_partial, float* mid_sums, void* stream) {
  using namespace seg;
  SEG_REQUIRE(order == 0 || order == 1, "conv_line_pair_fwd: bad axis order %d", order);
  SEG_REQUIRE(N >= 1 && H >= 1 && W >= 1 && (long)N * H * W < (1L << 31), "conv_line_pair_fwd: bad shape");
  const int L = order == 0 ? W : H;
  SEG_REQUIRE(pair_ok(dtype, C, L, dil),
              "conv_line_pair_fwd: unsupported dtype %d C %d line %d dil %d", dtype, C, L, dil);
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(x != nullptr && y != nullptr && wa != nullptr && wb != nullptr,
              "conv_line_pair_fwd: null x / y / weights");
  SEG_REQUIRE(ldx >= C && ldy >= C && ldx % vec == 0 && ldy % vec == 0 &&
                  (mid == nullptr || (ldmid >= C && ldmid % vec == 0)) &&
                  (add == nullptr || (ldadd >= C && ldadd % vec == 0)),
              "conv_line_pair_fwd: row pitches must hold C and be multiples of %d", vec);
  SEG_REQUIRE(pro_mode >= 0 && pro_mode <= PRO_AFFINE_RELU, "conv_line_pair_fwd: bad pro_mode %d", pro_mode);
  SEG_REQUIRE(!(pro_mode & PRO_AFFINE) || (pro_scale != nullptr && pro_shift != nullptr),
              "conv_line_pair_fwd: affine prologue without scale / shift");
  PairArgs a;
  a.x = x; a.ldx = ldx; a.wa = wa; a.wb = wb; a.ba = bias_a; a.bb = bias_b;
  a.mid = mid; a.ldmid = ldmid; a.y = y; a.ldy = ldy; a.add = add; a.ldadd = ldadd;
  a.ps = pro_scale; a.pt = pro_shift; a.pro_mode = pro_mode; a.stat = stat_partial;
  a.midsum = mid_sums; a.H = H; a.W = W; a.order = order; a.d = dil;
  a.lines = N * (order == 0 ? H : W); a.L = L;
  const int grid = pair_grid(a.lines);
  const int lds = pair_lds_bytes(dtype, L);
  const bool pro = pro_mode != PRO_NONE;
  hipStream_t s = (hipStream_t)stream;
#define SEG_LP(T_, P_) \
  hipLaunchKernelGGL((conv_line_pair_kernel<T_, P_>), dim3(grid), dim3(LP_THREADS), lds, s, a)
  if (dtype == DT_BF16) { if (pro) SEG_LP(bf16_t, true); else SEG_LP(bf16_t, false); }
  else { if (pro) SEG_LP(float, true); else SEG_LP(float, false); }
#undef SEG_LP
  return check_launch("conv_line_pair_fwd");
}
