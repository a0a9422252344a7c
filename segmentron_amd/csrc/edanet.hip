// EDANet's DownsamplerBlock (segmentron/models/edanet.py:90-97) concatenates a stride-2
// convolution with a 2x2 max-pool of the same input: cat([conv(x) 12 | pool(x) 3]) and
// cat([conv(x) 45 | pool(x) 15]).  The pooled part starts at a channel offset (12, 45) that is no
// whole 16-byte vector, which the vector kernels (pool.hip, bn.hip) cannot address.  This is the
// element-wise placement of a few channels at ANY channel offset:
//   dst[p][c] = c < C ? src[p][c] : 0     for c < Cz   (C <= Cz; pointers already offset)
// Forward: the pooled channels into their slice of the concat buffer (Cz = C).  Backward: the
// slice of the gradient into an aligned tensor of the pool's width, zeros in its pad (Cz > C).
#include "common.h"

namespace seg {

constexpr int CC_THREADS = 256, CC_MAX_BLOCKS = 4096;

template <typename T>
__global__ __launch_bounds__(CC_THREADS) void chan_copy_kernel(const T* __restrict__ src, long lds,
                                                               T* __restrict__ dst, long ldd,
                                                               long total, int C, int Cz) {
  for (long i = (long)blockIdx.x * CC_THREADS + threadIdx.x; i < total;
       i += (long)gridDim.x * CC_THREADS) {
    const long p = i / Cz;
    const int c = (int)(i - p * Cz);
    dst[p * ldd + c] = c < C ? src[p * lds + c] : T(0.f);
  }
}

}  // namespace seg

extern "C" int seg_chan_copy(int dtype, const void* src, long lds, void* dst, long ldd, long P,
                             int C, int Cz, void* stream) {
  using namespace seg;
  SEG_REQUIRE(dtype == DT_F32 || dtype == DT_BF16, "chan_copy: bad dtype %d", dtype);
  SEG_REQUIRE(src != nullptr && dst != nullptr, "chan_copy: null pointer");
  SEG_REQUIRE(P >= 1 && P < (1L << 31) && C >= 1 && Cz >= C && Cz <= 4096 && lds >= C && ldd >= Cz,
              "chan_copy: bad P=%ld C=%d Cz=%d lds=%ld ldd=%ld", P, C, Cz, lds, ldd);
  const long total = P * Cz;
  const long nb = (total + CC_THREADS - 1) / CC_THREADS;
  const dim3 grid((unsigned)(nb < CC_MAX_BLOCKS ? nb : CC_MAX_BLOCKS));
  if (dtype == DT_BF16)
    hipLaunchKernelGGL((chan_copy_kernel<bf16_t>), grid, dim3(CC_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const bf16_t*>(src), lds, reinterpret_cast<bf16_t*>(dst), ldd,
                       total, C, Cz);
  else
    hipLaunchKernelGGL((chan_copy_kernel<float>), grid, dim3(CC_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const float*>(src), lds, reinterpret_cast<float*>(dst), ldd,
                       total, C, Cz);
  return check_launch("chan_copy");
}
