// Dense 3-tap LINE convolution (factorised 3x1 / 1x3, stride 1, "same" size, per-axis dilation)
// and the split-shuffle tail of LEDNet's SSnbt block (segmentron/models/lednet.py:72-128).
//
//   y[n,h,w,o] = sum_{t=0..2} sum_c act(x[n, h + (t-1)*d*[axis==H], w + (t-1)*d*[axis==W], c])
//                                   * wp[o][t][c]                   (+ add[n,h,w,o], nullable)
//
// C == O in {16, 32, 40, 64}: K = 3C = 48 .. 192 and O <= 64 leave the implicit GEMM's 128x128 tile
// mostly empty and pay LDS staging for an operand that needs none: one MFMA B fragment of a lane
// IS one 16-byte channel vector of one pixel at one tap.  So, as in conv3x3_direct.hip, A = the
// weights (bf16: in registers for the kernel's lifetime, at most 96 VGPRs; float32: in LDS) and
// B = pixels straight from global memory / L2; a lane ends up with 4 consecutive output channels
// of ONE pixel (32x32 C/D map of conv_gemm.h).  O = 16 leaves the upper 16 MFMA rows zero.
// C = 40 (EDANet's growth rate): no padded tensors.  In bf16 a k-step is 16 channels, so the upper
// half of the third step (channels 40..47) is masked to zero in registers on both operands and its
// loads are clamped to the lane's own vector; output rows 40..63 of the second 32-row group are
// zero weights and are never stored.  A nullable per-channel float32 bias is added to the
// accumulators BEFORE `add`, the rounding and the statistics; a consumer's zero padding applies
// after it.
//
// A wave owns 32 consecutive pixels of the flattened [N*H*W] index per tile, a block 4 waves =
// CL_TILE pixels; blocks are persistent and walk a contiguous, XCD-local range of tiles.  A tap
// is taken only if it stays inside ITS OWN row (axis W) / image (axis H): it is zero AFTER the
// prologue, which is applied in float32 and, for bf16, rounded once before the MFMA.
// Statistics (nullable): per block one row [2][C] of sums / sums of squares of the values AS
// STORED (after `add`, after the rounding to bf16), accumulated in registers over the block's
// tiles and folded lanes -> waves in a fixed order.  No atomics anywhere.
#include "conv_gemm.h"
#include "rows.h"

namespace seg {

constexpr int CL_THREADS = 256, CL_WAVES = 4, CL_PX = 32, CL_TILE = CL_WAVES * CL_PX;
constexpr int CL_MAX_BLOCKS = 1024;

struct LineArgs {
  const void* x; long ldx;
  const void* w;
  void* y; long ldy;
  const void* add; long ldadd;
  const float* ps; const float* pt; int pro_mode;
  float* stat;
  const float* bias;  // nullable, [C]
  int H, W, axis, d;  // axis 0: H (3x1 kernel), 1: W (1x3)
  int P, ntiles;
};

// pixel p -> position along the axis; its limit and the pixel step of one tap come from the args
__device__ __forceinline__ int line_pos(const LineArgs& a, int p) {
  const unsigned q = (unsigned)p / (unsigned)a.W;
  return a.axis ? (int)((unsigned)p - q * (unsigned)a.W) : (int)(q % (unsigned)a.H);
}

template <typename T, int C> struct LineGeom {
  static constexpr int VEC = Vec<T>::N;
  static constexpr int KSTEP = 2 * VEC;  // k per vector step: 16 (bf16) / 8 (f32)
  static constexpr int KS = (C + KSTEP - 1) / KSTEP;
  static constexpr bool KTAIL = C % KSTEP != 0;  // C = 40, bf16: the last step's upper half is void
  static_assert(C % VEC == 0, "whole channel vectors");
  static constexpr int NOG = (C + 31) / 32;
  static constexpr bool WREG = sizeof(T) == 2;
  static constexpr int WPITCH = 3 * C * (int)sizeof(T) + 16;  // LDS weight row (f32 only)
  static constexpr int RED_BYTES = CL_WAVES * 2 * C * 4;
  static constexpr int LDS_BYTES = RED_BYTES + (WREG ? 0 : C * WPITCH);
};

template <typename T, int C, bool PRO, bool STATS>
__global__ __launch_bounds__(CL_THREADS) void conv_line_kernel(const LineArgs a) {
  using G = LineGeom<T, C>;
  constexpr int VEC = G::VEC, KS = G::KS, NOG = G::NOG;
  extern __shared__ __attribute__((aligned(16))) unsigned char cl_smem[];
  float* red = reinterpret_cast<float*>(cl_smem);
  unsigned char* wl = cl_smem + G::RED_BYTES;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r32 = lane & 31, h = lane >> 5;
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ Wt = reinterpret_cast<const T*>(a.w);
  const T* __restrict__ A = reinterpret_cast<const T*>(a.add);
  T* __restrict__ Y = reinterpret_cast<T*>(a.y);

  // ---- weights: fragment (og, t, ks) of output channel og*32 + r32, k = ks*KSTEP + h*VEC ..
  uint4 wf[G::WREG ? NOG : 1][3][G::WREG ? KS : 1];
  if (G::WREG) {
#pragma unroll
    for (int og = 0; og < NOG; ++og) {
      const bool orow = og * 32 + r32 < C;
      const T* wrow = Wt + (long)(orow ? og * 32 + r32 : 0) * (3 * C) + h * VEC;
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bool kv = !G::KTAIL || ks * G::KSTEP + h * VEC < C;
          wf[og][t][ks] =
              mask_u4(ldg16(wrow + t * C + (kv ? ks * G::KSTEP : -h * VEC)), orow && kv);
        }
    }
  } else {
    constexpr int VPR = 3 * C / VEC;
    for (int i = tid; i < C * VPR; i += CL_THREADS) {
      const int o = i / VPR, v = i - o * VPR;
      *reinterpret_cast<uint4*>(wl + o * G::WPITCH + v * 16) = ldg16(Wt + (long)o * (3 * C) + v * VEC);
    }
    __syncthreads();
  }

  float s1[NOG][16], s2[NOG][16];
  if (STATS) {
#pragma unroll
    for (int og = 0; og < NOG; ++og)
#pragma unroll
      for (int e = 0; e < 16; ++e) s1[og][e] = s2[og][e] = 0.f;
  }

  const int lim = a.axis ? a.W : a.H;
  const long step = a.axis ? (long)a.d : (long)a.d * a.W;
  const int nblk = gridDim.x;
  const int L = xcd_remap(blockIdx.x, nblk);
  const int per = (a.ntiles + nblk - 1) / nblk;
  const int t_end = min(a.ntiles, (L + 1) * per);
  for (int tile = L * per; tile < t_end; ++tile) {
    const long pl = (long)tile * CL_TILE + wave * CL_PX + r32;
    const bool pv = pl < a.P;
    const int p = pv ? (int)pl : 0;
    const int pos = line_pos(a, p);
    bool ok[3];
    long off[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const long q = (long)pos + (long)(t - 1) * a.d;
      ok[t] = pv && q >= 0 && q < lim;
      off[t] = ((long)p + (ok[t] ? (long)(t - 1) * step : 0)) * a.ldx + h * VEC;
    }
    // ---- all loads of the tile first (unconditional, clamped to the lane's own pixel)
    uint4 raw[3][KS];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bool kv = !G::KTAIL || ks * G::KSTEP + h * VEC < C;
        raw[t][ks] = ldg16(X + off[t] + (kv ? ks * G::KSTEP : -h * VEC));
      }

    f32x16 acc[NOG];
#pragma unroll
    for (int og = 0; og < NOG; ++og)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[og][e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bool kv = !G::KTAIL || ks * G::KSTEP + h * VEC < C;
      float ps[VEC], pt[VEC];
      if (PRO && (a.pro_mode & PRO_AFFINE) && kv) {
        load_params<VEC>(a.ps, ks * G::KSTEP + h * VEC, ps);
        load_params<VEC>(a.pt, ks * G::KSTEP + h * VEC, pt);
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) { ps[i] = 1.f; pt[i] = 0.f; }
      }
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        uint4 b = raw[t][ks];
        if (PRO) {
          float f[VEC];
          Vec<T>::unpack(b, f);
          apply_prologue_regs<VEC>(f, a.pro_mode, ps, pt);
          b = Vec<T>::pack(f);
        }
        b = mask_u4(b, G::KTAIL ? (ok[t] && kv) : ok[t]);
#pragma unroll
        for (int og = 0; og < NOG; ++og) {
          uint4 wv;
          if (G::WREG) {
            wv = wf[og][t][ks];
          } else {
            const bool orow = og * 32 + r32 < C;
            wv = mask_u4(*reinterpret_cast<const uint4*>(wl + (orow ? og * 32 + r32 : 0) * G::WPITCH +
                                                         (t * C + ks * G::KSTEP + h * VEC) * 4),
                         orow);
          }
          Mma<T>::step(wv, b, acc[og]);
        }
      }
    }

    // ---- epilogue: lane holds channels og*32 + 8g + 4h + j (g, j < 4) of pixel p
#pragma unroll
    for (int og = 0; og < NOG; ++og) {
      constexpr int GVmax = 4;
      const int gv = (C - og * 32) >= 32 ? GVmax : (C - og * 32) / 8;  // valid g (C = 16: 2)
      float f[4][4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int j = 0; j < 4; ++j) f[g][j] = acc[og][g * 4 + j];
        if (g < gv && a.bias != nullptr) {
          float bv[4];
          load_params<4>(a.bias, og * 32 + g * 8 + h * 4, bv);
#pragma unroll
          for (int j = 0; j < 4; ++j) f[g][j] += bv[j];
        }
        if (g < gv && A != nullptr) {
          const T* ap = A + (long)p * a.ldadd + og * 32 + g * 8 + h * 4;
          float av[4];
          HVec<T>::load(ap, av);
#pragma unroll
          for (int j = 0; j < 4; ++j) f[g][j] += av[j];
        }
      }
      if (sizeof(T) == 2) {
        uint2 pk[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          pk[g] = make_uint2(pack_bf16x2(f[g][0], f[g][1]), pack_bf16x2(f[g][2], f[g][3]));
          f[g][0] = __uint_as_float(pk[g].x << 16); f[g][1] = __uint_as_float(pk[g].x & 0xFFFF0000u);
          f[g][2] = __uint_as_float(pk[g].y << 16); f[g][3] = __uint_as_float(pk[g].y & 0xFFFF0000u);
        }
        // lanes l and l ^ 32 hold the two halves of each 8-channel vector: h = 0 keeps the even
        // g, h = 1 the odd ones -> 16-byte stores
#pragma unroll
        for (int gp = 0; gp < 4; gp += 2) {
          const uint2 send = h ? pk[gp] : pk[gp + 1];
          uint2 recv;
          recv.x = __shfl_xor(send.x, 32, 64);
          recv.y = __shfl_xor(send.y, 32, 64);
          if (gp + h < gv && pv) {
            const uint2 own = h ? pk[gp + 1] : pk[gp];
            const uint4 v = h ? make_uint4(recv.x, recv.y, own.x, own.y)
                              : make_uint4(own.x, own.y, recv.x, recv.y);
            stg16(Y + (long)p * a.ldy + og * 32 + (gp + h) * 8, v);
          }
        }
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          if (g < gv && pv)
            stg16(Y + (long)p * a.ldy + og * 32 + g * 8 + h * 4, Vec<float>::pack(f[g]));
      }
      if (STATS && pv) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            s1[og][g * 4 + j] += f[g][j];
            s2[og][g * 4 + j] = fmaf(f[g][j], f[g][j], s2[og][g * 4 + j]);
          }
      }
    }
  }

  if (STATS) {
    // lanes with the same h hold the same channels: fold bits 0..4, then the waves through LDS
#pragma unroll
    for (int og = 0; og < NOG; ++og)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
#pragma unroll
        for (int m = 1; m < 32; m <<= 1) {
          s1[og][e] += __shfl_xor(s1[og][e], m, 64);
          s2[og][e] += __shfl_xor(s2[og][e], m, 64);
        }
      }
    if (r32 == 0) {
#pragma unroll
      for (int og = 0; og < NOG; ++og)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int ch = og * 32 + (e >> 2) * 8 + h * 4 + (e & 3);
          if (ch < C) {
            red[(wave * 2 + 0) * C + ch] = s1[og][e];
            red[(wave * 2 + 1) * C + ch] = s2[og][e];
          }
        }
    }
    __syncthreads();
    if (tid < 2 * C) {
      float s = 0.f;
      for (int w = 0; w < CL_WAVES; ++w) s += red[w * 2 * C + tid];
      a.stat[(long)blockIdx.x * 2 * C + tid] = s;
    }
  }
}

// =============================================================================================
// Weight gradient:  dW[o][c][t] = sum_p dy[p][o] * act(x)[p + (t-1)*step][c]
// (stored [O][C][3]: the memory layout of both the [O,C,3,1] and the [O,C,1,3] parameter, so
// that the summed partials ARE the parameter's gradient, without a repacking copy)
// The reduction runs over pixels, so both MFMA operands are wanted pixel-major in k.  A block
// stages, per trip of 64 pixels, the dy rows and the THREE tap rows of x (prologue
// applied, masked per tap exactly as in the forward pass — so the LDS footprint does not depend
// on the dilation) as [pixel][channel] with a 16-byte pad, and reads them transposed: bf16 with
// ds_read_b64_tr_b16 (as conv3x3_direct.hip's weight gradient), float32 element-wise for
// v_mfma_f32_32x32x2_f32.  The three taps share the dy fragment.  C <= 32: one [32 o][32 c] tile
// per tap, the 4 waves split the trip's pixels and are summed through LDS in wave order at the
// end; C = 40 (staged as 64) and 64: wave w owns output half w & 1 and input half w >> 1.  One
// fp32 partial [O][C][3] per block, summed by seg_colsum.
typedef __attribute__((address_space(3))) unsigned char cl_lds_t;
typedef short cl_v4i16 __attribute__((ext_vector_type(4)));
typedef short cl_v8i16 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ bf16x8 cl_tr_frag(const cl_lds_t* p, int second_off) {
  typedef __attribute__((address_space(3))) cl_v4i16 lds_v4;
  const cl_v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)p);
  const cl_v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(p + second_off));
  const cl_v8i16 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return __builtin_bit_cast(bf16x8, v);
}

struct LineWgradArgs {
  const void* x; long ldx;
  const void* dy; long lddy;
  const float* ps; const float* pt; int pro_mode;
  float* partial;
  int H, W, axis, d;
  int P, ntrips;
};

template <typename T, int C> struct LineWGeom {
  static constexpr int VEC = Vec<T>::N;
  // staged channels per pixel: whole 32-channel MFMA tiles (C = 16: upper half 0; C = 40:
  // channels 40..63 are 0 and their products are not stored)
  static constexpr int CP = (C + 31) / 32 * 32;
  // pixels per staging trip (float32 at 64 staged channels: 32, to stay inside 64 KB of LDS)
  static constexpr int TP = (sizeof(T) == 4 && CP == 64) ? 32 : 64;
  static constexpr int NG = CP / 32;
  static constexpr bool KSPLIT = NG == 1;
  static constexpr int PITCH = CP * (int)sizeof(T) + 16;
  static constexpr int ARR = TP * PITCH;
  static constexpr int STAGE_BYTES = 4 * ARR;  // x taps 0..2, dy
  static constexpr int RED_BYTES = KSPLIT ? CL_WAVES * 16 * 64 * 4 : 0;
  static constexpr int LDS_BYTES = STAGE_BYTES > RED_BYTES ? STAGE_BYTES : RED_BYTES;
  static constexpr int VPR = CP / VEC;
  static constexpr int PER_ARR = TP * VPR;            // vectors of one staged array
  static constexpr int ITER = 4 * PER_ARR / CL_THREADS;   // per thread and trip
  static_assert(PER_ARR % CL_THREADS == 0, "one staging pass never straddles two arrays");
};

template <typename T, int C, bool PRO>
__global__ __launch_bounds__(CL_THREADS) void conv_line_wgrad_kernel(const LineWgradArgs a) {
  using G = LineWGeom<T, C>;
  constexpr int VEC = G::VEC;
  extern __shared__ __attribute__((aligned(16))) unsigned char cl_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  const T* __restrict__ DY = reinterpret_cast<const T*>(a.dy);

  const int sv = tid % G::VPR;  // this thread's channel vector (CL_THREADS % VPR == 0)
  const bool cok = sv * VEC < C;
  float ps[VEC], pt[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { ps[i] = 1.f; pt[i] = 0.f; }
  if (PRO && (a.pro_mode & PRO_AFFINE) && cok) {
    load_params<VEC>(a.ps, sv * VEC, ps);
    load_params<VEC>(a.pt, sv * VEC, pt);
  }
  const int og = G::KSPLIT ? 0 : (wave & 1), cg = G::KSPLIT ? 0 : (wave >> 1);
  f32x16 acc[3];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  const int lim = a.axis ? a.W : a.H;
  const long step = a.axis ? (long)a.d : (long)a.d * a.W;
  // transposed-read lane addressing (bf16): see conv3x3_direct.hip
  const int g4 = lane >> 4, i16 = lane & 15;
  const int prow = 8 * (g4 >> 1) + (i16 >> 2), cq = (g4 & 1) * 16 + (i16 & 3) * 4;
  const int r32 = lane & 31, hh = lane >> 5;

  const int nblk = gridDim.x;
  const int L = xcd_remap(blockIdx.x, nblk);
  const int per = (a.ntrips + nblk - 1) / nblk;
  const int t_end = min(a.ntrips, (L + 1) * per);
  for (int trip = L * per; trip < t_end; ++trip) {
    const long p0 = (long)trip * G::TP;
    uint4 raw[G::ITER];
    unsigned okm = 0;
#pragma unroll
    for (int q = 0; q < G::ITER; ++q) {
      const int arr = (q * CL_THREADS) / G::PER_ARR;
      const int i = (tid + (q * CL_THREADS) % G::PER_ARR) / G::VPR;
      const long pl = p0 + i;
      const bool pv = pl < a.P;
      const int p = pv ? (int)pl : 0;
      bool ok = pv && cok;
      long off;
      if (arr < 3) {
        const unsigned qq = (unsigned)p / (unsigned)a.W;
        const int pos = a.axis ? (int)((unsigned)p - qq * (unsigned)a.W) : (int)(qq % (unsigned)a.H);
        const long qa = (long)pos + (long)(arr - 1) * a.d;
        ok = ok && qa >= 0 && qa < lim;
        off = ((long)p + (ok ? (long)(arr - 1) * step : 0)) * a.ldx + (cok ? sv * VEC : 0);
        raw[q] = ldg16(X + off);
      } else {
        off = (long)p * a.lddy + (cok ? sv * VEC : 0);
        raw[q] = ldg16(DY + off);
      }
      okm |= ok ? (1u << q) : 0u;
    }
#pragma unroll
    for (int q = 0; q < G::ITER; ++q) {
      const int arr = (q * CL_THREADS) / G::PER_ARR;
      const int i = (tid + (q * CL_THREADS) % G::PER_ARR) / G::VPR;
      uint4 v = raw[q];
      if (PRO && arr < 3) {
        float f[VEC];
        Vec<T>::unpack(v, f);
        apply_prologue_regs<VEC>(f, a.pro_mode, ps, pt);
        v = Vec<T>::pack(f);
      }
      v = mask_u4(v, (okm >> q) & 1u);
      *reinterpret_cast<uint4*>(cl_smem + arr * G::ARR + i * G::PITCH + sv * 16) = v;
    }
    __syncthreads();
    if (sizeof(T) == 2) {
      const cl_lds_t* db = (const cl_lds_t*)cl_smem + 3 * G::ARR + prow * G::PITCH + (og * 32 + cq) * 2;
      const cl_lds_t* xb = (const cl_lds_t*)cl_smem + prow * G::PITCH + (cg * 32 + cq) * 2;
#pragma unroll
      for (int kk = 0; kk < G::TP / 16; ++kk) {
        if (G::KSPLIT && kk != wave) continue;
        const bf16x8 fa = cl_tr_frag(db + kk * 16 * G::PITCH, 4 * G::PITCH);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const bf16x8 fb = cl_tr_frag(xb + t * G::ARR + kk * 16 * G::PITCH, 4 * G::PITCH);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[t], 0, 0, 0);
        }
      }
    } else {
      const float* db = reinterpret_cast<const float*>(cl_smem + 3 * G::ARR) + og * 32 + r32;
      const float* xb = reinterpret_cast<const float*>(cl_smem) + cg * 32 + r32;
      constexpr int NS = G::KSPLIT ? G::TP / 2 / CL_WAVES : G::TP / 2;
      const int sbase = G::KSPLIT ? wave * NS : 0;
#pragma unroll 4
      for (int s = 0; s < NS; ++s) {
        const int px = 2 * (sbase + s) + hh;
        const float fa = db[px * (G::PITCH / 4)];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const float fb = xb[t * (G::ARR / 4) + px * (G::PITCH / 4)];
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // the trip is consumed: the next one may overwrite it
  }

  // ---- this block's partial: dW[o][c][t], o = og*32 + row(e, hh), c = cg*32 + r32
  float* Pp = a.partial + (long)blockIdx.x * C * (3 * C);
  if (G::KSPLIT) {
    float* red = reinterpret_cast<float*>(cl_smem);  // [wave][e][lane]
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 16; ++e) red[(wave * 16 + e) * 64 + lane] = acc[t][e];
      __syncthreads();
#pragma unroll
      for (int ee = 0; ee < 4; ++ee) {
        const int e = wave * 4 + ee;
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < CL_WAVES; ++w) s += red[(w * 16 + e) * 64 + lane];
        const int o = (e & 3) + 8 * (e >> 2) + 4 * hh;
        if (o < C && r32 < C) Pp[(long)o * (3 * C) + r32 * 3 + t] = s;
      }
    }
  } else {
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int o = og * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
        if (G::CP == C || (o < C && cg * 32 + r32 < C))
          Pp[(long)o * (3 * C) + (cg * 32 + r32) * 3 + t] = acc[t][e];
      }
  }
}

// =============================================================================================
// Split-shuffle tail of an SSnbt block (lednet.py:117-128): the two branches' pending
// BatchNorm + ReLU, torch.cat, + x, ReLU and channel_shuffle(groups = 2) in one pass:
//   out[p][2i + g] = relu(relu(y_g[p][i]*s_g[i] + t_g[i]) + x[p][g*C/2 + i])
// and its backward, unshuffled:  gm[p][g*C/2 + i] = gout[p][2i + g] * (out[p][2i + g] > 0).
// One thread per pixel and 16-byte vector of i: two 16-byte loads/stores on the shuffled side.
constexpr int ST_THREADS = 256, ST_MAX_BLOCKS = 2048;

struct TailArgs {
  const void* y0; long ldy0; const void* y1; long ldy1;
  const float* s0; const float* t0; const float* s1; const float* t1;
  const void* x; long ldx;
  void* out; long ldout;
  const void* outr;  // the stored forward output (backward)
  const void* gout; long ldgout;
  void* gm; long ldgm;
  long items; int vpp;  // vpp = C / 2 / VEC vectors of i per pixel
  int C;
};

template <typename T>
__global__ __launch_bounds__(ST_THREADS) void ssnbt_tail_fwd_kernel(const TailArgs a) {
  constexpr int VEC = Vec<T>::N;
  const T* __restrict__ Y0 = reinterpret_cast<const T*>(a.y0);
  const T* __restrict__ Y1 = reinterpret_cast<const T*>(a.y1);
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  T* __restrict__ O = reinterpret_cast<T*>(a.out);
  const int half = a.C / 2;
  for (long it = (long)blockIdx.x * ST_THREADS + threadIdx.x; it < a.items;
       it += (long)gridDim.x * ST_THREADS) {
    const long p = it / a.vpp;
    const int i0 = (int)(it - p * a.vpp) * VEC;
    float v0[VEC], v1[VEC], x0[VEC], x1[VEC], sc[VEC], sh[VEC], o[2 * VEC];
    Vec<T>::unpack(ldg16(Y0 + p * a.ldy0 + i0), v0);
    Vec<T>::unpack(ldg16(Y1 + p * a.ldy1 + i0), v1);
    Vec<T>::unpack(ldg16(X + p * a.ldx + i0), x0);
    Vec<T>::unpack(ldg16(X + p * a.ldx + half + i0), x1);
    load_params<VEC>(a.s0, i0, sc);
    load_params<VEC>(a.t0, i0, sh);
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      o[2 * k] = fmaxf(fmaxf(fmaf(v0[k], sc[k], sh[k]), 0.f) + x0[k], 0.f);
    load_params<VEC>(a.s1, i0, sc);
    load_params<VEC>(a.t1, i0, sh);
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      o[2 * k + 1] = fmaxf(fmaxf(fmaf(v1[k], sc[k], sh[k]), 0.f) + x1[k], 0.f);
    T* op = O + p * a.ldout + 2 * i0;
    stg16(op, Vec<T>::pack(o));
    stg16(op + VEC, Vec<T>::pack(o + VEC));
  }
}

template <typename T>
__global__ __launch_bounds__(ST_THREADS) void ssnbt_tail_bwd_kernel(const TailArgs a) {
  constexpr int VEC = Vec<T>::N;
  const T* __restrict__ GO = reinterpret_cast<const T*>(a.gout);
  const T* __restrict__ O = reinterpret_cast<const T*>(a.outr);
  T* __restrict__ GM = reinterpret_cast<T*>(a.gm);
  const int half = a.C / 2;
  for (long it = (long)blockIdx.x * ST_THREADS + threadIdx.x; it < a.items;
       it += (long)gridDim.x * ST_THREADS) {
    const long p = it / a.vpp;
    const int i0 = (int)(it - p * a.vpp) * VEC;
    float g[2 * VEC], o[2 * VEC], m0[VEC], m1[VEC];
    Vec<T>::unpack(ldg16(GO + p * a.ldgout + 2 * i0), g);
    Vec<T>::unpack(ldg16(GO + p * a.ldgout + 2 * i0 + VEC), g + VEC);
    Vec<T>::unpack(ldg16(O + p * a.ldout + 2 * i0), o);
    Vec<T>::unpack(ldg16(O + p * a.ldout + 2 * i0 + VEC), o + VEC);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      m0[k] = o[2 * k] > 0.f ? g[2 * k] : 0.f;
      m1[k] = o[2 * k + 1] > 0.f ? g[2 * k + 1] : 0.f;
    }
    stg16(GM + p * a.ldgm + i0, Vec<T>::pack(m0));
    stg16(GM + p * a.ldgm + half + i0, Vec<T>::pack(m1));
  }
}

// ---------------------------------------------------------------------------------------------
// what seg_conv_line_ok / _geom / _fwd have always served ...
static bool line_ok(int dtype, int C, int axis, int dil) {
  return (dtype == DT_F32 || dtype == DT_BF16) && (C == 16 || C == 32 || C == 64) &&
         (axis == 0 || axis == 1) && dil >= 1 && dil < (1 << 20);
}

// ... and what the seg_conv_line_bias_* entries and the weight gradient serve: C = 40 as well
static bool line_bias_ok(int dtype, int C, int axis, int dil) {
  return C == 40 ? line_ok(dtype, 32, axis, dil) : line_ok(dtype, C, axis, dil);
}

static int line_grid(long P) {
  const long nt = (P + CL_TILE - 1) / CL_TILE;
  return (int)(nt < CL_MAX_BLOCKS ? nt : CL_MAX_BLOCKS);
}

static int line_wgrad_cap(int C) { return C > 32 ? 128 : (C == 32 ? 512 : 1024); }

static int line_wgrad_tp(int dtype, int C) { return dtype == DT_F32 && C > 32 ? 32 : 64; }

static int line_wgrad_grid(int dtype, long P, int C) {
  const int tp = line_wgrad_tp(dtype, C);
  const long nt = (P + tp - 1) / tp;
  const int cap = line_wgrad_cap(C);
  return (int)(nt < cap ? nt : cap);
}

template <typename T, int C>
static void launch_line(const LineArgs& a, int grid, hipStream_t s) {
  const bool pro = a.pro_mode != PRO_NONE, st = a.stat != nullptr;
  constexpr int lds = LineGeom<T, C>::LDS_BYTES;
#define SEG_CL(P_, S_) \
  hipLaunchKernelGGL((conv_line_kernel<T, C, P_, S_>), dim3(grid), dim3(CL_THREADS), lds, s, a)
  if (pro && st) SEG_CL(true, true);
  else if (pro) SEG_CL(true, false);
  else if (st) SEG_CL(false, true);
  else SEG_CL(false, false);
#undef SEG_CL
}

template <typename T, int C>
static void launch_line_wgrad(const LineWgradArgs& a, int grid, hipStream_t s) {
  constexpr int lds = LineWGeom<T, C>::LDS_BYTES;
  static_assert(lds <= 64 * 1024, "fits the default dynamic LDS limit");
  if (a.pro_mode != PRO_NONE)
    hipLaunchKernelGGL((conv_line_wgrad_kernel<T, C, true>), dim3(grid), dim3(CL_THREADS), lds, s, a);
  else
    hipLaunchKernelGGL((conv_line_wgrad_kernel<T, C, false>), dim3(grid), dim3(CL_THREADS), lds, s, a);
}

}  // namespace seg

#define SEG_CL_DISPATCH(fn, dtype, C, ...)                      \
  do {                                                          \
    if (dtype == DT_BF16) {                                     \
      if (C == 16) fn<bf16_t, 16>(__VA_ARGS__);                 \
      else if (C == 32) fn<bf16_t, 32>(__VA_ARGS__);            \
      else if (C == 40) fn<bf16_t, 40>(__VA_ARGS__);            \
      else fn<bf16_t, 64>(__VA_ARGS__);                         \
    } else {                                                    \
      if (C == 16) fn<float, 16>(__VA_ARGS__);                  \
      else if (C == 32) fn<float, 32>(__VA_ARGS__);             \
      else if (C == 40) fn<float, 40>(__VA_ARGS__);             \
      else fn<float, 64>(__VA_ARGS__);                          \
    }                                                           \
  } while (0)

extern "C" int seg_conv_line_ok(int dtype, int C, int axis, int dil) {
  return seg::line_ok(dtype, C, axis, dil) ? 1 : 0;
}

extern "C" int seg_conv_line_bias_ok(int dtype, int C, int axis, int dil) {
  return seg::line_bias_ok(dtype, C, axis, dil) ? 1 : 0;
}

// what: 0 pixels per tile, 1 grid (= rows of stat_partial), 2 tiles per block,
//       3 pixels per trip of the weight gradient
extern "C" int seg_conv_line_bias_geom(int dtype, int N, int H, int W, int C, int what) {
  using namespace seg;
  const long P = (long)N * H * W;
  if (!line_bias_ok(dtype, C, 0, 1) || N < 1 || H < 1 || W < 1 || P >= (1L << 31) - CL_TILE)
    return -1;
  const int grid = line_grid(P);
  const long nt = (P + CL_TILE - 1) / CL_TILE;
  switch (what) {
    case 0: return CL_TILE;
    case 1: return grid;
    case 2: return (int)((nt + grid - 1) / grid);
    case 3: return line_wgrad_tp(dtype, C);
    default: return -1;
  }
}

extern "C" int seg_conv_line_geom(int dtype, int N, int H, int W, int C, int what) {
  return seg::line_ok(dtype, C, 0, 1) ? seg_conv_line_bias_geom(dtype, N, H, W, C, what) : -1;
}

extern "C" int seg_conv_line_wgrad_splits(int dtype, int N, int H, int W, int C) {
  using namespace seg;
  const long P = (long)N * H * W;
  if (!line_bias_ok(dtype, C, 0, 1) || N < 1 || H < 1 || W < 1 || P >= (1L << 31) - CL_TILE)
    return -1;
  return line_wgrad_grid(dtype, P, C);
}

extern "C" int seg_conv_line_bias_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                                      const void* wp, const float* bias, int axis, int dil,
                                      int pro_mode, const float* pro_scale, const float* pro_shift,
                                      void* y, long ldy, const void* add, long ldadd,
                                      float* stat_partial, void* stream) {
  using namespace seg;
  SEG_REQUIRE(line_bias_ok(dtype, C, axis, dil),
              "conv_line_bias_fwd: unsupported dtype %d C %d axis %d dil %d", dtype, C, axis, dil);
  const long P = (long)N * H * W;
  SEG_REQUIRE(N >= 1 && H >= 1 && W >= 1 && P < (1L << 31) - CL_TILE, "conv_line_fwd: bad shape");
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(x != nullptr && y != nullptr && wp != nullptr, "conv_line_fwd: null x / y / wp");
  SEG_REQUIRE(ldx >= C && ldy >= C && ldx % vec == 0 && ldy % vec == 0 &&
                  (add == nullptr || (ldadd >= C && ldadd % vec == 0)),
              "conv_line_fwd: row pitches must hold C and be multiples of %d", vec);
  SEG_REQUIRE(pro_mode >= 0 && pro_mode <= PRO_AFFINE_RELU, "conv_line_fwd: bad pro_mode %d", pro_mode);
  SEG_REQUIRE(!(pro_mode & PRO_AFFINE) || (pro_scale != nullptr && pro_shift != nullptr),
              "conv_line_fwd: affine prologue without scale / shift");
  LineArgs a;
  a.x = x; a.ldx = ldx; a.w = wp; a.y = y; a.ldy = ldy; a.add = add; a.ldadd = ldadd;
  a.ps = pro_scale; a.pt = pro_shift; a.pro_mode = pro_mode; a.stat = stat_partial;
  a.bias = bias;
  a.H = H; a.W = W; a.axis = axis; a.d = dil; a.P = (int)P;
  a.ntiles = (int)((P + CL_TILE - 1) / CL_TILE);
  const int grid = line_grid(P);
  SEG_CL_DISPATCH(launch_line, dtype, C, a, grid, (hipStream_t)stream);
  return check_launch("conv_line_fwd");
}

extern "C" int seg_conv_line_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                                 const void* wp, int axis, int dil, int pro_mode,
                                 const float* pro_scale, const float* pro_shift, void* y, long ldy,
                                 const void* add, long ldadd, float* stat_partial, void* stream) {
  // (this entry keeps the classes it has always had; C = 40 is the bias entry's)
  SEG_REQUIRE(seg::line_ok(dtype, C, axis, dil),
              "conv_line_fwd: unsupported dtype %d C %d axis %d dil %d", dtype, C, axis, dil);
  return seg_conv_line_bias_fwd(dtype, x, ldx, N, H, W, C, wp, nullptr, axis, dil, pro_mode,
                                pro_scale, pro_shift, y, ldy, add, ldadd, stat_partial, stream);
}

extern "C" int seg_conv_line_wgrad(int dtype, const void* x, long ldx, const void* dy, long lddy,
                                   int N, int H, int W, int C, int axis, int dil, int pro_mode,
                                   const float* pro_scale, const float* pro_shift, float* partial,
                                   int splits, void* stream) {
  using namespace seg;
  SEG_REQUIRE(line_bias_ok(dtype, C, axis, dil),
              "conv_line_wgrad: unsupported dtype %d C %d axis %d dil %d",
              dtype, C, axis, dil);
  const long P = (long)N * H * W;
  SEG_REQUIRE(N >= 1 && H >= 1 && W >= 1 && P < (1L << 31) - CL_TILE, "conv_line_wgrad: bad shape");
  const int vec = dtype == DT_BF16 ? 8 : 4;
  SEG_REQUIRE(x != nullptr && dy != nullptr && partial != nullptr, "conv_line_wgrad: null pointer");
  SEG_REQUIRE(ldx >= C && lddy >= C && ldx % vec == 0 && lddy % vec == 0,
              "conv_line_wgrad: row pitches must hold C and be multiples of %d", vec);
  SEG_REQUIRE(pro_mode >= 0 && pro_mode <= PRO_AFFINE_RELU, "conv_line_wgrad: bad pro_mode %d", pro_mode);
  SEG_REQUIRE(!(pro_mode & PRO_AFFINE) || (pro_scale != nullptr && pro_shift != nullptr),
              "conv_line_wgrad: affine prologue without scale / shift");
  const int grid = line_wgrad_grid(dtype, P, C);
  SEG_REQUIRE(splits == grid, "conv_line_wgrad: splits %d, seg_conv_line_wgrad_splits says %d", splits,
              grid);
  LineWgradArgs a;
  a.x = x; a.ldx = ldx; a.dy = dy; a.lddy = lddy; a.ps = pro_scale; a.pt = pro_shift;
  a.pro_mode = pro_mode; a.partial = partial; a.H = H; a.W = W; a.axis = axis; a.d = dil;
  a.P = (int)P; const int tp = line_wgrad_tp(dtype, C);
  a.ntrips = (int)((P + tp - 1) / tp);
  SEG_CL_DISPATCH(launch_line_wgrad, dtype, C, a, grid, (hipStream_t)stream);
  return check_launch("conv_line_wgrad");
}

// what: 0 threads per block, 1 grid, 2 loop trips of the busiest thread
extern "C" int seg_ssnbt_tail_geom(int dtype, long P, int C, int what) {
  using namespace seg;
  if ((dtype != DT_F32 && dtype != DT_BF16) || (C != 32 && C != 64 && C != 128) || P < 1 ||
      P >= (1L << 31))
    return -1;
  const long items = P * (C / 2 / (dtype == DT_BF16 ? 8 : 4));
  const int grid = grid_1d(items, ST_THREADS, ST_MAX_BLOCKS);
  switch (what) {
    case 0: return ST_THREADS;
    case 1: return grid;
    case 2: return (int)((items + (long)grid * ST_THREADS - 1) / ((long)grid * ST_THREADS));
    default: return -1;
  }
}

static int tail_common(const char* what, int dtype, long P, int C, const long* lds, int nld,
                       seg::TailArgs* a) {
  using namespace seg;
  SEG_REQUIRE((C == 32 || C == 64 || C == 128) && P < (1L << 31), "%s: bad P=%ld C=%d", what, P, C);
  const int vec = dtype == DT_BF16 ? 8 : 4;
  const int need[5] = {C / 2, C / 2, C, C, C};  // (the two halves, then whole rows)
  // (one "image" of P pixels, no chunks)
  if (rows_require(what, dtype, 1, P, C, vec, vec, lds, need, nld, 1, 1)) return 1;
  *a = TailArgs();
  a->C = C; a->vpp = C / 2 / vec; a->items = P * a->vpp;
  return 0;
}

extern "C" int seg_ssnbt_tail_fwd(int dtype, const void* y0, long ldy0, const float* s0,
                                  const float* t0, const void* y1, long ldy1, const float* s1,
                                  const float* t1, const void* x, long ldx, void* out, long ldout,
                                  long P, int C, void* stream) {
  using namespace seg;
  TailArgs a;
  const long lds[4] = {ldy0, ldy1, ldx, ldout};
  if (tail_common("ssnbt_tail_fwd", dtype, P, C, lds, 4, &a)) return 1;
  SEG_REQUIRE(y0 && y1 && s0 && t0 && s1 && t1 && x && out, "ssnbt_tail_fwd: null pointer");
  a.y0 = y0; a.ldy0 = ldy0; a.y1 = y1; a.ldy1 = ldy1; a.s0 = s0; a.t0 = t0; a.s1 = s1; a.t1 = t1;
  a.x = x; a.ldx = ldx; a.out = out; a.ldout = ldout;
  const dim3 grid(grid_1d(a.items, ST_THREADS, ST_MAX_BLOCKS));
  SEG_LAUNCH_T(ssnbt_tail_fwd_kernel, grid, dim3(ST_THREADS), 0, stream, a);
  return check_launch("ssnbt_tail_fwd");
}

extern "C" int seg_ssnbt_tail_bwd(int dtype, const void* gout, long ldgout, const void* out,
                                  long ldout, void* gm, long ldgm, long P, int C, void* stream) {
  using namespace seg;
  TailArgs a;
  const long lds[5] = {C, C, ldgout, ldout, ldgm};
  if (tail_common("ssnbt_tail_bwd", dtype, P, C, lds, 5, &a)) return 1;
  SEG_REQUIRE(gout && out && gm, "ssnbt_tail_bwd: null pointer");
  a.gout = gout; a.ldgout = ldgout; a.outr = out; a.ldout = ldout; a.gm = gm; a.ldgm = ldgm;
  const dim3 grid(grid_1d(a.items, ST_THREADS, ST_MAX_BLOCKS));
  SEG_LAUNCH_T(ssnbt_tail_bwd_kernel, grid, dim3(ST_THREADS), 0, stream, a);
  return check_launch("ssnbt_tail_bwd");
}
