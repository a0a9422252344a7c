// Depthwise 3x3: the kernel families, their launchers, and the one place that picks a family for
// a launch (dw_route, dwconv.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace seg {
enum DwFamily {
  DW_SLIDE,     // register-sliding (dwconv_slide.hip)
  DW_TILED,     // LDS-tiled (dwconv_tiled.hip)
  DW_TILED_S2,  // LDS-tiled stride-2 forward (dwconv_tiled.hip; its fused backward: dwconv_s2.hip)
  DW_ROW,       // row-chain (dwconv_row.hip)
  DW_STRIP      // strip fallback (dwconv.hip)
};
enum DwOp {
  DW_OP_FWD,      // forward; with reversed taps also the stride-1 data gradient
  DW_OP_DGRAD,    // strided data gradient
  DW_OP_BWD,      // fused backward
  DW_OP_BWD_ADD,  // fused backward with a residual added in the store path (sliding family only)
  DW_OP_WGRAD     // separate weight gradient (tiled at dilation 1 and 2, else strip)
};
struct DwRoute {
  DwFamily family;
  int vec;          // C and the pitches must be multiples of this in the family's launcher
  bool torch_taps;  // reads torch's [C,1,3,3] taps too (w_layout bit 0); else tap-major [9][C] only
};
DwRoute dw_route(DwOp op, int dtype, int C, int stride, int dil);
// partial rows / persistent blocks per channel block of that launch; -1: no such launch
int dw_route_grid_y(DwRoute r, DwOp op, int dtype, int C, int N, int Ho, int Wo, int dil);

// ---- register-sliding, stride 1, dilation 1
// partial rows one launch writes (forward statistics / backward partials): image x strip x column block
int dw_slide_rows(int C, int N, int H, int W);
int launch_dw_slide_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                        const float* w, int w_layout, int pro_mode, const float* sc,
                        const float* sh, void* y, long ldy, float* stat_partial, int rows,
                        hipStream_t st);
int launch_dw_slide_bwd(int dtype, const void* dy, long lddy, const void* x, long ldx, int N, int H,
                        int W, int C, const float* w, int w_layout, int pro_mode, const float* sc,
                        const float* sh, void* g, long ldg, float* partial_w, float* partial_bn,
                        int rows, hipStream_t st, const void* res = nullptr, long ldr = 0,
                        int res_mode = 1);  // 1: g + res, one rounding; 2: as the 2-ary sum
// ---- LDS-tiled, stride 1: forward / data gradient and fused backward at dilation 2 (the launchers
// refuse any other), weight gradient at dilation 1 and 2
int dw_tiled_grid_y(int dtype, int C, int N, int H, int W, int kind);
int launch_dw_tiled(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                    const float* w, int w_layout, int dil, int pro_mode, const float* sc,
                    const float* sh, void* y, long ldy, float* stat_partial, int grid_y,
                    hipStream_t st);
int launch_dw_bwd_tiled(int dtype, const void* dy, long lddy, const void* x, long ldx, int N, int H,
                        int W, int C, const float* w, int w_layout, int dil, int pro_mode,
                        const float* sc, const float* sh, void* g, long ldg, float* partial_w,
                        float* partial_bn, int grid_y, hipStream_t st);
int launch_dw_wgrad_finalize(const float* partial, int R, int C, float* out, hipStream_t st);
int launch_dw_wgrad_tiled(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                          const void* dy, long lddy, int dil, int pro_mode, const float* sc,
                          const float* sh, float* partial, int grid_y, hipStream_t st);
// ---- LDS-tiled, stride 2, pad 1, dilation 1 (H x W: input size)
int dw_tiled_s2_grid_y(int dtype, int C, int N, int Ho, int Wo);
int launch_dw_tiled_s2(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                       const float* w, int w_layout, int pro_mode, const float* sc,
                       const float* sh, void* y, long ldy, float* stat_partial, int grid_y,
                       hipStream_t st);
// ---- row-chain, stride 1, dilation 3..64
int dw_row_grid_y(int dtype, int C, int N, int H, int W, int dil);
int launch_dw_row_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                      const float* w9c, int dil, int pro_mode, const float* sc, const float* sh,
                      void* y, long ldy, float* stat_partial, int grid_y, hipStream_t st);
int launch_dw_row_bwd(int dtype, const void* dy, long lddy, const void* x, long ldx, int N, int H,
                      int W, int C, const float* w9c, int dil, int pro_mode, const float* sc,
                      const float* sh, void* g, long ldg, float* partial_w, float* partial_bn,
                      int grid_y, hipStream_t st);
}  // namespace seg
