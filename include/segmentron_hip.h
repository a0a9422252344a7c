/* segmentron_hip.h — C ABI of libsegmentron_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for SegmenTron's dense-convolution hot path.  The reference has NO native
 * boundary for this path: all arithmetic is delegated to torch.nn / torch.nn.functional
 * (ATen -> MIOpen/oneDNN), see SURVEY.md §1 "Op layer" and §8(b).  Each entry point below is what
 * a binding for the corresponding reference call site would call instead of the ATen op; the
 * reference-side binding (ctypes stub) is shown in INTEGRATION.md.  The reference's only native
 * code (segmentron/modules/csrc/vision.cpp:6-11, CCNet criss-cross attention) is out of scope.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; every pointer is DEVICE memory unless noted
 *   - activations are NHWC: element (n,h,w,c) of a tensor with row pitch `ld` (elements) lives at
 *     base + ((n*H + h)*W + w)*ld + c ; `ld >= C` lets an op read/write a channel slice of a wider
 *     (concatenation) buffer.  C and ld must be multiples of 16 bytes / sizeof(element).
 *   - dtype: 0 = float32, 1 = bfloat16 (element type of activations / packed weights);
 *     BatchNorm parameters, statistics and all accumulation are float32 / float64
 *   - pro_mode ("prologue"): the producer's BatchNorm(+ReLU) applied on the fly to an input:
 *     0 none, 1 relu(x), 2 x*scale[c]+shift[c], 3 relu(x*scale[c]+shift[c]); +4 = ReLU6 clamp
 *     (5 = relu6(x), 7 = relu6(x*scale[c]+shift[c]))
 *   - `stream` is a hipStream_t; all launches are asynchronous on it; no host synchronisation,
 *     no allocation; re-entrant and graph-capturable; no process-wide state.
 *   - return value 0 = ok; otherwise seg_last_error() (thread-local) describes the failure.
 *     Never aborts.
 */
#ifndef SEGMENTRON_HIP_H
#define SEGMENTRON_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

const char* seg_last_error(void);
int seg_version(void);

/* The float-reciprocal index division of the grid-stride kernels (csrc/common.h: fast_div), run on
 * the HOST (no device needed): q[i] = fast_div(s[i], d, 1.f / (float)d) for i < n, returns 0.
 * seg_fast_div_exact: 1 iff the launchers' guard accepts a largest dividend s with divisor d, i.e.
 * the division is proven exact for every dividend 0 .. s; seg_fast_div_max_quot: floor(2^24 / 3),
 * the quotient bound of that guard (as a long through *out). */
int seg_fast_div_host(const int* s, long n, int d, int* q);
int seg_fast_div_exact(long s, long d);
int seg_fast_div_max_quot(long* out);

/* ---- nn.Conv2d, groups=1 (1x1 any stride, dense KxK): implicit GEMM on MFMA ----------------
 * Replaces F.conv2d for segmentron/modules/basic.py:42,69; segmentron/modules/module.py:45,57;
 * segmentron/models/backbones/xception.py:21,77,81; segmentron/models/deeplabv3_plus.py:64.
 * y[n,ho,wo,o] = bias[o] + sum_{kh,kw,c} act(x[n,ho*stride-pad+kh*dil, wo*stride-pad+kw*dil, c])
 *                                        * w[o][(kh*KW+kw)*C + c]
 * w is packed [O][KH*KW*C] in `dtype`.  stat_partial (nullable): [seg_conv_gemm_tiles_m][2][O]
 * fp32 per-tile (sum, sum of squares) of the pre-bias fp32 results, for the following BatchNorm.
 * out_s != 1 scatters output pixel (n,ho,wo) to row ((n*out_H + ho*out_s)*out_W + wo*out_s)
 * (data-gradient of a strided 1x1 conv; the caller zero-fills y first).
 * The same entry point computes data gradients: pass dy as x and the transposed/flipped weights.
 * tconv = 1: transposed-stride gather — x is dy [N,Hi,Wi,C=O_fwd], (Ho,Wo) the size of dx, w packed
 * [C_fwd][KH*KW*O_fwd] (not flipped): dx[h,w] = sum dy[(h+pad-kh*dil)/stride, ...] W (exact
 * divisions only) = data gradient of a strided KxK convolution (resnet.py:52-53, hrnet.py:195-204).
 * ep_x (nullable, addressed like y with pitch ldep) fuses the BatchNorm-backward correction of a
 * folded layer into the store: y = acc - ep_c0[o] - ep_c1[o]*ep_x[row][o] (see seg_fold_*). */
int seg_conv_gemm_fwd(int dtype, const void* x, long ldx, int N, int Hi, int Wi, int C,
                      const void* w, int O, int KH, int KW, int stride, int pad, int dil,
                      int pro_mode, const float* pro_scale, const float* pro_shift,
                      const float* bias, void* y, long ldy, int Ho, int Wo, int out_H, int out_W,
                      int out_s, float* stat_partial, const void* ep_x, long ldep,
                      const float* ep_c0, const float* ep_c1, int tconv, void* stream);
int seg_conv_gemm_tiles_m(int N, int Ho, int Wo);

/* Weight gradient of the same convolution (autograd's conv2d backward wrt weight):
 * partial[s][o][k] for s < splits (fp32); sum over s with seg_colsum gives dW[O][KH*KW*C].
 * The forward prologue is re-applied to x (the activated input is never stored). */
int seg_conv_gemm_wgrad(int dtype, const void* x, long ldx, int N, int Hi, int Wi, int C,
                        const void* dy, long lddy, int Ho, int Wo, int O, int KH, int KW,
                        int stride, int pad, int dil, int pro_mode, const float* pro_scale,
                        const float* pro_shift, float* partial, int splits, void* stream);
/* rows of the [rows][2][O] statistics buffer seg_conv_gemm_fwd writes for this geometry */
int seg_conv_gemm_stat_rows(int dtype, int N, int Ho, int Wo, int C, int O, int KH, int KW,
                            int stride, int pad, int dil, int tconv, int has_bias, int pro_mode);
/* splits to allocate `partial` for (same geometry arguments as the seg_conv_gemm_wgrad call:
 * plain 1x1 convolutions run on the direct-to-LDS kernel, which wants ~one block per CU; the
 * 3x3 stride-1 stems with 32 input channels on persistent blocks, one partial each) */
int seg_conv_gemm_wgrad_splits(int dtype, int N, int Ho, int Wo, int C, int O, int KH, int KW,
                               int stride, int pad, int dil, int pro_mode);

/* ---- nn.Conv2d, groups=C, 3x3, padding=dilation (depthwise) --------------------------------
 * Replaces segmentron/modules/basic.py:38-40 (SeparableConv2d.depthwise), :152-153.
 * w9c: fp32 taps; w_layout 0 = [9][C] tap-major, bit 0 = torch's own [C,1,3,3] (no repacking,
 * stride 1 / dilation <= 2 only), bit 1 = taps read reversed (stride-1 data gradient = forward
 * correlation with flipped taps).  mode 0: forward (x -> y).  mode 1: data gradient
 * (x = dy with geometry N,Hi,Wi; y = dx with geometry Ho,Wo; same w9c, stride, dil).
 * stat_partial (forward only, nullable): [grid_y][2][C].  grid_y from seg_dwconv_grid_y.
 * Which kernel family runs a launch (sliding, LDS-tiled, LDS-tiled stride 2, row-chain, strip),
 * the channel-vector width and the tap layouts it takes: the table on dw_route, csrc/dwconv.hip. */
int seg_dwconv3x3(int dtype, int mode, const void* x, long ldx, int N, int Hi, int Wi, int C,
                  const float* w9c, int w_layout, int stride, int dil, int pro_mode,
                  const float* pro_scale, const float* pro_shift, void* y, long ldy, int Ho, int Wo,
                  float* stat_partial, int grid_y, void* stream);
/* partial rows (= persistent blocks per channel block) of one depthwise launch, or -1 where there
 * is no such launch (a non-positive size; C not a positive multiple of the channel vector the
 * family's geometry counts in).  kind: 0 forward / data gradient, 1 fused backward, 2 weight
 * gradient */
int seg_dwconv_grid_y(int dtype, int C, int N, int Ho, int Wo, int stride, int dil, int kind);
/* partial: fp32 [grid_y][9][C]; column-sum gives dW[9][C];
 * seg_dwconv3x3_wgrad_finalize reduces it straight into torch's [C,1,3,3] layout. */
int seg_dwconv3x3_wgrad_finalize(const float* partial, int R, int C, float* dw_c9, void* stream);
int seg_dwconv3x3_wgrad(int dtype, const void* x, long ldx, int N, int Hi, int Wi, int C,
                        const void* dy, long lddy, int Ho, int Wo, int stride, int dil,
                        int pro_mode, const float* pro_scale, const float* pro_shift,
                        float* partial, int grid_y, void* stream);

/* Fused stride-1 backward of the depthwise conv in ONE pass over (dy, x):
 *   g[p]  = relu_mask(x[p]) * sum_k dy[p - d_k] * w9c[k]        (gradient wrt act(x), masked)
 *   partial_w  [grid_y][9][C] : weight-gradient partials (sum rows -> dW[9][C])
 *   partial_bn [grid_y][2][C] : (sum g, sum g*x_raw) for seg_bn_bwd_finalize_p (nullable)
 * x is the forward input (raw tensor + prologue), w9c the FORWARD taps (w_layout as above, bit 1
 * unused).  grid_y from seg_dwconv_grid_y(dtype, C, N, H, W, 1, dil, 1).  dil 1: register-sliding
 * kernel (csrc/dwconv_slide.hip); dil 2: LDS-tiled kernel with a tile software pipeline
 * (csrc/dwconv_tiled.hip); dil 3..64: row-chain kernel (csrc/dwconv_row.hip); wider: strip kernel.
 * C and the three pitches must be multiples of 4.  The LDS-tiled kernel (dil 2) wants all of them
 * multiples of 8 in bf16; the row-chain kernel (dil 3..64, csrc/dwconv_row.hip), which stages dy
 * with 16-byte vectors, wants C and lddy multiples of 8 in bf16 — a bf16 C = 4 (mod 8) there is
 * an error, not an over-read.  The sliding (dil 1) and strip (dil > 64) kernels take 4. */
int seg_dwconv3x3_bwd_fused(int dtype, const void* dy, long lddy, const void* x, long ldx, int N,
                            int H, int W, int C, const float* w9c, int w_layout, int dil,
                            int pro_mode, const float* pro_scale, const float* pro_shift, void* g,
                            long ldg, float* partial_w, float* partial_bn, int grid_y,
                            void* stream);
/* The same with `res` ([N,H,W,C], pitch ldr, element type of g) ADDED to the masked data gradient
 * in the store path: g = relu_mask(x) * dgrad + res — the second gradient of a forked activation
 * (an Xception block input feeds the residual sum and the first separable conv,
 * segmentron/models/backbones/xception.py:36-42), which autograd would add in a separate
 * element-wise pass.  Stride 1, dilation 1 only (seg_..._add_ok(dil) != 0): the register-sliding
 * kernel.  C and the pitches of dy, x, g: multiples of 8 in bf16, 4 in fp32; ldr: of 4. */
int seg_dwconv3x3_bwd_fused_add_ok(int dil);
int seg_dwconv3x3_bwd_fused_add(int dtype, const void* dy, long lddy, const void* x, long ldx, int N,
                                int H, int W, int C, const float* w9c, int w_layout, int pro_mode,
                                const float* pro_scale, const float* pro_shift, const void* res,
                                long ldr, void* g, long ldg, float* partial_w, float* partial_bn,
                                int grid_y, void* stream);
/* seg_dwconv3x3_bwd_fused_add with the masked gradient rounded to dtype before res joins: bit for
 * bit seg_sum_n over the stored g of seg_dwconv3x3_bwd_fused and res, in one pass — for a res that
 * used to meet g in that sum (the shortcut conv's data gradient of a conv-skip Xception block).
 * Sliding family only: seg_dwconv3x3_bwd_fused_sum_ok (dilation 1, C a multiple of 4 and of the
 * element type's 16-byte vector), pure host. */
int seg_dwconv3x3_bwd_fused_sum_ok(int dtype, int C, int dil);
int seg_dwconv3x3_bwd_fused_sum(int dtype, const void* dy, long lddy, const void* x, long ldx, int N,
                                int H, int W, int C, const float* w9c, int w_layout, int pro_mode,
                                const float* pro_scale, const float* pro_shift, const void* res,
                                long ldr, void* g, long ldg, float* partial_w, float* partial_bn,
                                int grid_y, void* stream);

/* ---- nn.BatchNorm2d / nn.SyncBatchNorm (train + eval, forward + backward) -------------------
 * Replaces F.batch_norm behind every `bn*` module (segmentron/modules/basic.py:41,43,70;
 * segmentron/modules/module.py:46,54,58; xception.py:22,78,82) and torch's SyncBatchNorm
 * collectives (tools/train.py:76): the caller all-reduces the 2C doubles between seg_colsum
 * and the finalize call.  eps / momentum are read at call time. */
/* out[l] = sum_r in[r][l]  (in: fp32 [R][L]); ws: >= 64*L doubles (needed when R > 128). */
int seg_colsum(const float* in, long R, int L, double* out_d, float* out_f, double* ws,
               void* stream);
/* float64 column sums with the local element count appended (out_d[L] = count): the
 * SyncBatchNorm forward message of one BatchNorm, assembled by one launch. */
int seg_colsum_count(const float* in, long R, int L, double* out_d, double count, double* ws,
                     void* stream);
/* sums = [sum x (C), sum x^2 (C)] over `count` samples.  Writes mean, invstd (biased var),
 * scale = gamma*invstd, shift = beta - mean*scale; updates running stats (nullable) with the
 * unbiased variance and `momentum`.  mean_offset (nullable, [C]) is added to the batch mean for the
 * running_mean update only: the per-channel constant a folded convolution (seg_fold_weights) leaves
 * out of its stored output because the following BatchNorm cancels it.
 * count_dev (nullable, here and in the backward finalizes): a DEVICE double that overrides
 * `count` — the SyncBatchNorm caller all-reduces [sums | local count] as one message and passes
 * &buf[2C], so unequal per-rank shards are exact without a host read-back. */
int seg_bn_finalize(const double* sums, double count, const double* count_dev,
                    const float* gamma, const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                    float* mean, float* invstd, float* scale, float* shift, int C,
                    const float* mean_offset, void* stream);
/* Single-process BatchNorm: the same directly from the [R][2][C] fp32 partial rows the conv /
 * reduce kernels emit (column sum fused in, fp64).  ws: >= 128*C doubles, used when R > 1024. */
int seg_bn_finalize_p(const float* partial, long R, double count, const float* gamma,
                      const float* beta, float eps, float momentum, float* running_mean,
                      float* running_var, float* mean, float* invstd, float* scale, float* shift,
                      int C, const float* mean_offset, double* ws, void* stream);
/* The same for a BatchNorm over FEW samples (M = N*H*W <= 4096 rows of the stored NHWC tensor y,
 * row pitch ldy): two-pass statistics (mean, then sum (x - mean)^2) straight from y — the
 * single-pass partial sums lose mean^2 / var digits, catastrophic for the 2-sample BatchNorm of
 * the ASPP image-pooling branch (module.py:52-64) and PSP's pyramid bins (module.py:89-97). */
int seg_bn_finalize_small(int dtype, const void* y, long ldy, long M, int C, const float* gamma,
                          const float* beta, float eps, float momentum, float* running_mean,
                          float* running_var, float* mean, float* invstd, float* scale,
                          float* shift, const float* mean_offset, void* stream);
/* ... under SyncBatchNorm (torch.nn.SyncBatchNorm / the reference's NaiveSyncBatchNorm,
 * segmentron/modules/batch_norm.py:135-176): every rank takes ITS rows' two-pass moments and the
 * ranks merge them as float64 sums (n*mean_r, M2_r + n*mean_r^2, n).  seg_bn_moments_small writes
 * those 2C + 1 doubles for a torch.distributed all-reduce followed by seg_bn_finalize;
 * seg_bn_finalize_small_sync merges them through the peer mailbox inside the launch (count_out =
 * the global element count, as seg_bn_finalize_p_sync). */
int seg_bn_moments_small(int dtype, const void* y, long ldy, long M, int C, double* moments,
                         void* stream);
int seg_bn_finalize_small_sync(void* p2p, int dtype, const void* y, long ldy, long M, int C,
                               const float* gamma, const float* beta, float eps, float momentum,
                               float* running_mean, float* running_var, float* mean, float* invstd,
                               float* scale, float* shift, const float* mean_offset,
                               double* count_out, void* stream);
/* y = xs[0] + ... + xs[n-1] (2 <= n <= 8 NHWC operands of M rows x C channels, row pitches lds[],
 * host arrays of device pointers / pitches), fp32 accumulation in index order, one rounding: the
 * gradient of an activation with several consumers (torch autograd: n-1 `add` launches). */
int seg_sum_n(int dtype, int n, const void* const* xs, const long* lds, void* y, long ldy, long M,
              int C, void* stream);
/* eval mode: scale/shift from running statistics. */
int seg_bn_eval_affine(const float* gamma, const float* beta, const float* rm, const float* rv,
                       float eps, float* scale, float* shift, int C, void* stream);
/* ... of n BatchNorms at once (host arrays of device pointers; out[j]: 2*C[j] floats = scale row,
 * shift row; C[j] <= 2048; gamma[j] / beta[j] nullable): one launch per 48 jobs instead of one per
 * BatchNorm of an evaluation-mode forward. */
int seg_bn_eval_affine_multi(int n, const float* const* gamma, const float* const* beta,
                             const float* const* rm, const float* const* rv, const float* eps,
                             float* const* out, const int* C, void* stream);
/* Materialise: y = post_relu?( act_x(x) * chan_mul[n][c] + act_r(r) )  (r, chan_mul nullable).
 * Covers BN+ReLU materialisation, the residual adds of xception.py:40,42 / resnet.py:38,78 and
 * nn.Dropout2d (segmentron/modules/module.py:60; chan_mul = mask/(1-p), rows_per_n = H*W) and
 * nn.Dropout (module.py:21, pspnet.py:52; elem_mul = per-element mask/(1-p) of the element type). */
int seg_bn_apply(int dtype, const void* x, long ldx, int mode_x, const float* sx, const float* tx,
                 const void* r, long ldr, int mode_r, const float* sr, const float* tr,
                 const float* chan_mul, long rows_per_n, const void* elem_mul, long ldm,
                 int post_relu, void* y, long ldy, long M, int C, void* stream);
/* Backward of "act(x) consumed with gradient g": g' = g * chan_mul * relu_mask.
 * reduce  : partial[grid_y][2][C] = (sum g', sum g'*x) per block
 * finalize: dgamma, dbeta and the coefficients c0,c1 of  dx = scale*g' - c0 - c1*x
 * apply   : dx (may alias g).  With mode lacking the affine bit: dx = g' (ReLU backward). */
int seg_bn_bwd_grid_y(int dtype, int C, long M);
/* Launch geometry of the row-tile kernels (seg_bn_apply, seg_bn_bwd_reduce, seg_bn_bwd_apply,
 * seg_sum_n), pure host.  what: 0 = lanes (16-byte channel vectors) per row of a block, 1 = rows
 * per block, 2 = threads per block, 3 = gridDim.x, 4 = gridDim.y of the apply kernels and
 * seg_sum_n for M rows (the reduce has seg_bn_bwd_grid_y rows).  -1 on a bad argument. */
int seg_ew_geom_query(int dtype, int C, long M, int what);
int seg_bn_bwd_reduce(int dtype, const void* g, long ldg, const void* x, long ldx, int mode,
                      const float* scale, const float* shift, const float* chan_mul,
                      long rows_per_n, const void* elem_mul, long ldm, long M, int C,
                      float* partial, int grid_y, void* stream);
/* BatchNorm backward of a SMALL tensor (M = N*H*W <= 4096 rows; same layers as
 * seg_bn_finalize_small) in ONE launch with float64 arithmetic: g' = g * chan_mul * elem_mul *
 * relu_mask, dx = gamma*invstd*(g' - mean(g') - xhat*mean(g'*xhat)) (training = 1) or
 * scale*g' (training = 0), dgamma = sum g'*xhat, dbeta = sum g'.  dx may alias g.  Replaces
 * seg_bn_bwd_reduce + seg_bn_bwd_finalize_p + seg_bn_bwd_apply there: with a handful of samples
 * per channel dx is the remainder of cancelling terms, which fp32 `scale*g' - c0 - c1*x` loses. */
int seg_bn_bwd_small(int dtype, const void* g, long ldg, const void* x, long ldx, void* dx,
                     long lddx, long M, int C, int mode, const float* scale, const float* shift,
                     const float* mean, const float* invstd, const float* gamma,
                     const float* chan_mul, long rows_per_n, const void* elem_mul, long ldm,
                     double count, int training, float* dgamma, float* dbeta, void* stream);
int seg_bn_bwd_finalize(const double* sums, double count, const double* count_dev,
                        const float* mean, const float* invstd, const float* gamma, float* dgamma, float* dbeta, float* c0, float* c1,
                        int C, void* stream);
/* seg_bn_bwd_finalize with dgamma / dbeta multiplied by grad_scale (SyncBatchNorm: the sums are
 * global and the data-parallel gradient averaging divides by the world size once more — torch's
 * SyncBatchNorm returns local sums there, torch/nn/modules/_functions.py:150-170). */
int seg_bn_bwd_finalize_s(const double* sums, double count, const double* count_dev,
                          const float* mean, const float* invstd, const float* gamma, float* dgamma,
                          float* dbeta, float* c0, float* c1, int C, double grad_scale, void* stream);
int seg_bn_bwd_finalize_p(const float* partial, long R, double count, const float* mean,
                          const float* invstd, const float* gamma, float* dgamma, float* dbeta,
                          float* c0, float* c1, int C, double* ws, void* stream);
/* Both reductions behind a fused depthwise backward in one launch: seg_bn_bwd_finalize_p on
 * partial_bn [Rb][2][C] (Rb <= 1024) and seg_dwconv3x3_wgrad_finalize on partial_w [Rw][9][C]
 * (replaces two launches per depthwise layer and step; the reference's counterpart is autograd's
 * batch_norm_backward + the depthwise weight-gradient reduction inside cudnn/MIOpen,
 * segmentron/modules/basic.py:38-44). */
int seg_dw_bwd_finalize(const float* partial_bn, int Rb, double count, const float* mean,
                        const float* invstd, const float* gamma, float* dgamma, float* dbeta,
                        float* c0, float* c1, const float* partial_w, int Rw, float* dw_c9, int C,
                        void* stream);
int seg_bn_bwd_apply(int dtype, const void* g, long ldg, const void* x, long ldx, int mode,
                     const float* scale, const float* shift, const float* c0, const float* c1,
                     const float* chan_mul, long rows_per_n, const void* elem_mul, long ldm,
                     void* dx, long lddx, long M, int C, void* stream);
/* dx = round(scale*g' - c0 - c1*x) + round(dx_add): `add` ([M][C] of dtype, pitch ldadd) is the
 * gradient of another consumer of the same raw tensor.  add_mode 0: dx_add = add (already w.r.t.
 * the raw tensor).  Otherwise add is w.r.t. that consumer's activated input (add_mode = its
 * prologue bits on the same scale / shift) and dx_add = scale*mask(add) - add_c0 - add_c1*x with the
 * coefficients of ITS finalize (null: evaluation mode).  Both terms are rounded to dtype first, so
 * the result equals the separate seg_bn_bwd_apply passes + seg_sum_n bit for bit.  Geometry of
 * seg_bn_bwd_apply. */
int seg_bn_bwd_apply_add(int dtype, const void* g, long ldg, const void* x, long ldx, int mode,
                         const float* scale, const float* shift, const float* c0, const float* c1,
                         const void* add, long ldadd, int add_mode, const float* add_c0,
                         const float* add_c1, void* dx, long lddx, long M, int C, void* stream);

/* ---- nn.GroupNorm(min(32, C), C): the 'GN' choice of cfg.MODEL.BN_TYPE -------------------------
 * Replaces the nn.GroupNorm modules segmentron/modules/batch_norm.py:105-108,129 builds (F.group_norm
 * forward + autograd backward).  Group statistics are per SAMPLE: z = x*a[n][c] + b[n][c] — a
 * per-(sample, channel) affine, materialised (it cannot ride in a per-channel prologue).
 *   seg_gn_moments      partial[n][chunk][2][C] = (sum u, sum u*v) over the chunk's pixels; v null:
 *                       v = u (sum x, sum x^2).  chunks = seg_gn_chunks(HW).
 *   seg_gn_fwd_finalize mean_rstd[n][g][2] and coef[n][3][C] = (gamma*rstd, 0, beta - mean*gamma*rstd)
 *                       (gamma / beta nullable: affine=False), float64 sums, biased variance
 *   seg_gn_bwd_finalize from the moments of (u, v) = (dz, x): coef[n][3][C] of
 *                       dx = k1*dz + k2*x + k3, and contrib[n][2][C] = per-sample terms of
 *                       (dgamma, dbeta) — sum over n with seg_colsum
 *   seg_gn_affine       out = coef[n][0][c]*u + coef[n][1][c]*v + coef[n][2][c]   (v nullable) */
int seg_gn_chunks(long HW);
int seg_gn_moments(int dtype, const void* u, long ldu, const void* v, long ldv, int N, long HW,
                   int C, float* partial, void* stream);
int seg_gn_fwd_finalize(const float* partial, int N, long HW, int C, int G, const float* gamma,
                        const float* beta, double eps, float* mean_rstd, float* coef,
                        void* stream);
int seg_gn_bwd_finalize(const float* partial, int N, long HW, int C, int G,
                        const float* mean_rstd, const float* gamma, float* coef, float* contrib,
                        void* stream);
int seg_gn_affine(int dtype, const void* u, long ldu, const void* v, long ldv, const float* coef,
                  void* out, long ldo, int N, long HW, int C, void* stream);

/* ---- linear BatchNorm folded into a 1x1 convolution -------------------------------------------
 * `relu_first` SeparableConv2d (segmentron/modules/basic.py:46-50) has no non-linearity between
 * bn_depth and the pointwise conv: W (s.*x + t) = (W diag(s)) x + W t.
 * fold_weights : Wp[o][c] = W[o][c]*scale[c] (dtype), WpT = its transpose [C][O] (nullable),
 *                bprime[o] = sum_c W[o][c]*shift[c] (nullable).  W is fp32 [O][C].
 * fold_bwd_*   : from dWp = dY^T x_raw (fp32 [O][C]) and db = colsum(dY) (nullable = 0):
 *                dW, then dgamma/dbeta of the folded BatchNorm and the coefficients of
 *                dx_raw = dY Wp - c0 - c1 x_raw.  dsdt = [ds (C), dt (C)] is all-reduced by the
 *                caller between the two calls under SyncBN. */
int seg_fold_weights(int dtype, const float* W, const float* scale, const float* shift, void* Wp,
                     void* WpT, float* bprime, int O, int C, void* stream);
/* dWp: the weight-gradient split partials [splits][O*C] as written by seg_conv_gemm_wgrad (summed
 * here); dsdt: [seg_fold_bwd_rows(O)][2][C] partial (ds, dt) rows, summed by the finalize. */
int seg_fold_bwd_rows(int O);
int seg_fold_bwd_reduce(const float* W, const float* dWp, int splits, const float* scale,
                        const float* shift, const float* db, float* dW, float* dsdt, int O, int C,
                        void* stream);
int seg_fold_bwd_finalize(const float* dsdt, int rows, double count, const double* count_dev,
                          const float* mean, const float* invstd, const float* gamma, const float* scale, float* dgamma, float* dbeta,
                          float* c0, float* c1, int C, void* stream);
/* the same with dgamma / dbeta multiplied by grad_scale (SyncBatchNorm: 1 / world size) */
int seg_fold_bwd_finalize_s(const float* dsdt, int rows, double count, const double* count_dev,
                            const float* mean, const float* invstd, const float* gamma,
                            const float* scale, float* dgamma, float* dbeta, float* c0, float* c1,
                            int C, double grad_scale, void* stream);

/* ---- pooling --------------------------------------------------------------------------------
 * nn.MaxPool2d(k, stride, pad) (segmentron/models/backbones/resnet.py:119) on a deferred
 * activation; idx = one byte per output element (winning tap), consumed by the backward gather. */
int seg_maxpool_fwd(int dtype, const void* x, long ldx, int N, int Hi, int Wi, int C, int k,
                    int stride, int pad, int pro_mode, const float* pro_scale,
                    const float* pro_shift, void* y, long ldy, int Ho, int Wo, void* idx,
                    void* stream);
int seg_maxpool_bwd(int dtype, void* gx, long ldgx, int N, int Hi, int Wi, int C, int k, int stride,
                    int pad, const void* gy, long ldgy, int Ho, int Wo, const void* idx,
                    void* stream);
/* nn.AdaptiveAvgPool2d(o) (segmentron/modules/module.py:52,89), ATen bins
 * [floor(i*H/o), ceil((i+1)*H/o)).  partial: fp32 [chunks][N*o*o][C] bin SUMS (reduce over chunks
 * with seg_colsum, divide by the bin area). */
int seg_adaptive_avgpool_chunks(int H, int W, int o);
int seg_adaptive_avgpool_partial(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                                 int o, float* partial, int chunks, void* stream);
int seg_adaptive_avgpool_bwd(int dtype, void* gx, long ldgx, int N, int H, int W, int C, int o,
                             const void* gy, long ldgy, void* stream);

/* ---- channel attention: squeeze (global average pool) + sigmoid gate (csrc/chan_gate.hip) -----
 * Replaces nn.AdaptiveAvgPool2d(1) -> ... -> nn.Sigmoid() -> `x * attention` of
 * segmentron/models/bisenet.py:106-120,170-186.  NHWC, HW = H*W pixels per image, `chunks` =
 * seg_apply_pool_chunks(N, HW, C) pixel chunks per image; a / radd / v are fp32 [N][C].  Partial
 * rows are fp32, written per (chunk, image) and summed over the chunks in index order: no atomics,
 * bit-identical results on every launch.
 *   seg_apply_pool_fwd   y = act(x) (y nullable: pool only) and partial[chunks][N][C] = sums of the
 *                        fp32 activated values (seg_colsum over the chunks, divide by HW)
 *   seg_chan_gate_fwd    y = x * (identity + sigmoid(a[n][c])) + r + radd[n][c]   (r, radd nullable)
 *   seg_chan_gate_bwd    dx = dy * (identity + sigmoid(a)) (dx nullable) and
 *                        partial[chunks][N][2][C] = (sum_hw dy*x, sum_hw dy)
 *   seg_chan_gate_bwd_finalize   da = s(1-s) * sum dy*x, dradd = sum dy   (either nullable)
 *   seg_bcast_add        y = g + v[n][c] * scale (g nullable: the broadcast alone; y may be g) */
int seg_apply_pool_chunks(int N, long HW, int C);
int seg_apply_pool_fwd(int dtype, const void* x, long ldx, int pro_mode, const float* pro_scale,
                       const float* pro_shift, void* y, long ldy, int N, long HW, int C,
                       float* partial, int chunks, void* stream);
int seg_chan_gate_fwd(int dtype, const void* x, long ldx, const float* a_pre, int identity,
                      const void* r, long ldr, const float* radd, void* y, long ldy, int N, long HW,
                      int C, int chunks, void* stream);
int seg_chan_gate_bwd(int dtype, const void* dy, long lddy, const void* x, long ldx,
                      const float* a_pre, int identity, void* dx, long lddx, int N, long HW, int C,
                      float* partial, int chunks, void* stream);
int seg_chan_gate_bwd_finalize(const float* partial, int chunks, int N, int C, const float* a_pre,
                               float* da, float* dradd, void* stream);
int seg_bcast_add(int dtype, const void* g, long ldg, const float* v, float scale, void* y,
                  long ldy, int N, long HW, int C, int chunks, void* stream);

/* ---- CGNet's ContextGuidedBlock (csrc/cgnet.hip; segmentron/models/cgnet.py:149-181) -----------
 * NHWC; partial rows are fp32, one per (pixel chunk, image), summed in index order: no atomics,
 * bit-identical results on every launch, and no image reaches another image's rows.
 *   seg_cg_joint_fwd   y[..., :C] = depthwise 3x3 (w_loc, pad 1) of x, y[..., C:2C] = depthwise 3x3
 *                      (w_sur, pad = dilation = dil) of the same x, one pass; w_loc / w_sur are the
 *                      [C,1,3,3] parameters as they are; C % 4 == 0, pitches % 4 == 0;
 *                      partial[chunks * N][2][2C] (nullable) = sum | sum of squares of the fp32
 *                      accumulators, chunks = seg_cg_joint_chunks(N, H, W, C) (or any 1..256)
 *   seg_bn_prelu_fwd   y = prelu(x * scale[c] + shift[c], alpha[c]) (scale / shift both null: plain
 *                      PReLU; y nullable: sums only) and partial[chunks][N][C] (nullable) = per-image
 *                      sums of the fp32 activated values, chunks as seg_apply_pool_chunks.  Any
 *                      C >= 1: every pitch holds C rounded up to 8, the parameter arrays have
 *                      exactly C elements, and y's channels [C, round_up(C, 8)) are written as zeros
 *   seg_prelu_bwd      g = g_y + g_pool[n][c] / HW (either nullable), z = x * scale + shift,
 *                      g_z = z > 0 ? g : alpha * g (pad channels: zeros), partial[chunks][N][C] =
 *                      sum over z <= 0 of g * z: dalpha = seg_colsum over the chunks * N rows */
int seg_cg_joint_chunks(int N, int H, int W, int C);
int seg_cg_joint_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                     const float* w_loc, const float* w_sur, int dil, void* y, long ldy,
                     float* partial, int chunks, void* stream);
int seg_bn_prelu_fwd(int dtype, const void* x, long ldx, const float* scale, const float* shift,
                     const float* alpha, void* y, long ldy, int N, long HW, int C, float* partial,
                     int chunks, void* stream);
int seg_prelu_bwd(int dtype, const void* g_y, long ldgy, const float* g_pool, const void* x,
                  long ldx, const float* scale, const float* shift, const float* alpha, void* g_z,
                  long ldgz, int N, long HW, int C, float* partial, int chunks, void* stream);

/* ---- ESPNetv2's EESP unit and DownSampler (csrc/espnetv2.hip; segmentron/modules/module.py:165-207,
 * segmentron/models/backbones/eespnet.py:14-43) ---------------------------------------------------
 * NHWC, fp32 and bf16; every pitch is a multiple of the element type's 16-byte vector (4 / 8).  No
 * atomics, fp32 partial rows summed in index order, bit-identical results on every launch, and no
 * image reaches another image's outputs or rows.
 *   seg_eesp_pyr_fwd     y[..., j*n:(j+1)*n] = sum_{i <= j} depthwise 3x3 (w_i, pad = dilation = d_i,
 *                        stride) of x for j = 0..3, one pass over x, fp32 sums rounded once; w_i are
 *                        the [n,1,3,3] parameters as they are; n a positive multiple of 8, each d_i
 *                        in 1..4 and d0 <= d1 <= d2 <= d3, stride 1 or 2, y has (H-1)/stride + 1
 *                        rows; anything else is an error.  partial[chunks * N][2][4n] (nullable) =
 *                        sum | sum of squares of the fp32 values, chunks = seg_eesp_pyr_chunks(...)
 *                        (or any 1..256)
 *   seg_eesp_suffix_sum  s[..., j*n:(j+1)*n] = sum_{i >= j} g[..., i*n:(i+1)*n] over rows of 4n
 *                        channels (what branch j's backward sees); s may be g
 *   seg_avgpool3x3s2_*   nn.AvgPool2d(3, 2, 1) with count_include_pad: divisor 9 everywhere; C a
 *                        multiple of the vector; the backward writes every gx once (a gather)
 *   seg_bn_add_prelu_fwd y = prelu(a * sa + ta + b * sb + tb, alpha); sa / ta and sb / tb nullable in
 *                        pairs (a plain operand); C a multiple of the vector, chunks as
 *                        seg_apply_pool_chunks
 *   seg_bn_add_prelu_bwd z recomputed, g_z = z > 0 ? g : alpha * g (the gradient of both affine
 *                        operands' outputs), partial[chunks][N][C] = sum over z <= 0 of g * z:
 *                        dalpha = seg_colsum over the chunks * N rows */
int seg_eesp_pyr_chunks(int N, int H, int W, int n, int stride);
int seg_eesp_pyr_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int n,
                     const float* w0, const float* w1, const float* w2, const float* w3, int d0,
                     int d1, int d2, int d3, int stride, void* y, long ldy, float* partial,
                     int chunks, void* stream);
int seg_eesp_suffix_sum(int dtype, const void* g, long ldg, void* s, long lds, long rows, int n,
                        void* stream);
int seg_avgpool3x3s2_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int C, void* y,
                         long ldy, void* stream);
int seg_avgpool3x3s2_bwd(int dtype, const void* gy, long ldgy, int N, int H, int W, int C, void* gx,
                         long ldgx, void* stream);
int seg_bn_add_prelu_fwd(int dtype, const void* a, long lda, const float* sa, const float* ta,
                         const void* b, long ldb, const float* sb, const float* tb,
                         const float* alpha, void* y, long ldy, int N, long HW, int C, int chunks,
                         void* stream);
int seg_bn_add_prelu_bwd(int dtype, const void* g, long ldg, const void* a, long lda,
                         const float* sa, const float* ta, const void* b, long ldb, const float* sb,
                         const float* tb, const float* alpha, void* g_z, long ldgz, int N, long HW,
                         int C, float* partial, int chunks, void* stream);

/* ---- FPENet's FPE block and MEU module (csrc/fpenet.hip; segmentron/models/fpenet.py:150-247) ----
 * NHWC, fp32 and bf16.  The channel vector is 4 elements (16 B of fp32, 8 B of bf16): n, every pitch
 * and every channel offset are multiples of 4, not of 8.  No atomics, fp32 partial rows per (chunk,
 * image) summed in index order, bit-identical results on every launch, and no image reaches another
 * image's outputs or rows.  act(x; s, t) = relu(s[c]*x + t[c]).
 *   seg_fpe_stage_fwd    y = depthwise 3x3 (w the [n,1,3,3] parameter as it is, pad = dilation = dil,
 *                        stride 1) of in = act(a; sa, ta) + act(b; sb, tb), the sum in fp32 and never
 *                        rounded; b (with sb, tb, b_act) nullable: stage 0.  n a positive multiple of
 *                        4 up to 64, dil in 1..8; anything else is an error before any launch.
 *                        b_act (nullable): act(b) at the centre pixel rounded once, written to a slice
 *                        of another buffer (pitch ldo).  partial[rows][2][n] (nullable) = sum | sum of
 *                        squares of the fp32 outputs, rows = seg_fpe_stage_rows(...) (or any
 *                        chunks * N, chunks in 1..256)
 *   seg_fpe_act_fwd      y = act(b; sb, tb) over rows of an n-channel slice (the last stage's slice
 *                        of the concat: seg_bn_apply takes 8-channel vectors in bf16)
 *   seg_fpe_stage_bwd    with t_k = dy[p - d_k] and dgrad = sum_k t_k * w[k]:
 *                          ga = mask(a) * dgrad, gb = mask(b) * (dgrad + res)  (mask: s*x + t > 0),
 *                          pw[rows][9][n] = sum t_k * in[p] (the layout seg_dw_bwd_finalize and
 *                          seg_dwconv3x3_wgrad_finalize take),
 *                          pa[rows][2][pa_pitch] at column pa_col = (sum ga | sum ga*a_raw),
 *                          pb[rows][2][n] = (sum gb | sum gb*b_raw)  (seg_bn_bwd_finalize_p's layout).
 *                        b, res, gb, pb are null together (stage 0).  dy null (then a, ga, pw, pa are
 *                        not read): gb = mask(b) * res and pb alone, the last stage's slice.
 *   seg_fpe_bn_bwd_apply dx = scale*g - c0 - c1*x over rows of an n-channel slice; c0 / c1 null
 *                        together: dx = scale*g (evaluation-mode BatchNorm).  dx may be g.
 *   seg_meu_fwd          out = a[n][c]*(sl*L + tl) + sa[p]*(sh*bilinear(Hraw) + th),
 *                        sa[p] = sigmoid(w_sa[0] * mean_c(sl*L + tl)) also stored as fp32 [N,h,w];
 *                        L [N,h,w,C], Hraw [N,h2,w2,C], 1 <= h2 <= h, 1 <= w2 <= w, align_corners
 *                        taps; a fp32 [N][C]; w_sa a device float; C a multiple of 8 up to 128;
 *                        sl / tl and sh / th nullable in pairs
 *   seg_meu_bwd_low      dL = a*g + w_sa * sa(1-sa)/C * S[p], S[p] = sum_c g*Hup (the gradient at
 *                        bn_low's output); p_a[rows][2][C] = (sum_p g*Lbn | in column 0:
 *                        sum_p sa(1-sa) * mean_c(Lbn) * S), p_bn[rows][2][C] = (sum dL | sum dL*L);
 *                        rows = seg_meu_rows(N, h, w, C, 0), row = chunk * N + image
 *   seg_meu_bwd_high     dH[q][c] = sum_p wgt(p,q) * sa[p] * g[p][c] + dpool[n][c]/(h2*w2) (dpool fp32
 *                        [N][C], nullable), every dH written once; p_bn[rows][2][C] = (sum dH |
 *                        sum dH*Hraw), rows = seg_meu_rows(N, h2, w2, C, 1) */
int seg_fpe_stage_rows(int dtype, int N, int H, int W, int n);
int seg_fpe_stage_fwd(int dtype, const void* a, long lda, const float* sa, const float* ta,
                      const void* b, long ldb, const float* sb, const float* tb, const float* w,
                      int dil, void* y, long ldy, void* b_act, long ldo, int N, int H, int W, int n,
                      float* partial, int rows, void* stream);
int seg_fpe_act_fwd(int dtype, const void* b, long ldb, const float* sb, const float* tb, void* y,
                    long ldy, long rows, int n, void* stream);
int seg_fpe_stage_bwd(int dtype, const void* dy, long lddy, const void* a, long lda, const float* sa,
                      const float* ta, const void* b, long ldb, const float* sb, const float* tb,
                      const void* res, long ldres, const float* w, int dil, void* ga, long ldga,
                      void* gb, long ldgb, int N, int H, int W, int n, float* pw, float* pa,
                      long pa_pitch, int pa_col, float* pb, int rows, void* stream);
int seg_fpe_bn_bwd_apply(int dtype, const void* g, long ldg, const void* x, long ldx,
                         const float* scale, const float* c0, const float* c1, void* dx, long lddx,
                         long rows, int n, void* stream);
int seg_meu_rows(int N, int h, int w, int C, int high);
int seg_meu_fwd(int dtype, const void* L, long ldl, const float* sl, const float* tl, const void* Hr,
                long ldh, const float* sh, const float* th, const float* a, const float* wsa,
                void* out, long ldo, float* sa, int N, int h, int w, int h2, int w2, int C,
                void* stream);
int seg_meu_bwd_low(int dtype, const void* g, long ldg, const void* L, long ldl, const float* sl,
                    const float* tl, const void* Hr, long ldh, const float* sh, const float* th,
                    const float* a, const float* wsa, const float* sa, void* dL, long lddl, int N,
                    int h, int w, int h2, int w2, int C, float* p_a, float* p_bn, int rows,
                    void* stream);
int seg_meu_bwd_high(int dtype, const void* g, long ldg, const float* sa, const void* Hr, long ldh,
                     const float* dpool, void* dH, long lddh, int N, int h, int w, int h2, int w2,
                     int C, float* p_bn, int rows, void* stream);

/* ---- UNet's encoder skips and padded upsampling (csrc/unet.hip; segmentron/models/unet.py:81-121) --
 * NHWC, fp32 and bf16, a channel pitch per operand, C a multiple of the 16-byte vector (4 / 8).
 * No atomics: bit-identical results on every launch.  act = the seg_maxpool_fwd prologue
 * (pro_mode / scale / shift; the model uses affine + ReLU).
 *   seg_skip_pool_fwd     one pass over the raw y [N,H,W,C]: skip = act(y) (a slice of a wider
 *                         buffer) and pooled [N,H/2,W/2,C] (floor) = the 2x2 / stride-2 max of the
 *                         stored values, i.e. of act(y) rounded to the activation dtype.  A trailing
 *                         odd row or column goes to skip only; no index tensor.  H, W >= 2.
 *   seg_skip_pool_bwd     g' = relu_mask * (g_skip + scatter(g_pool)) written densely, the activation
 *                         recomputed from y; the winner of a window is the first maximum of the
 *                         rounded activations in row-major order (ATen's max_pool2d rule).
 *                         partial[rows][2][C] = (sum g' | sum g'*y) of the unrounded fp32 g', the
 *                         layout seg_bn_bwd_finalize_p takes; rows = seg_skip_pool_bwd_rows(...) (or
 *                         any 1..65535).  g_skip and g_pool are nullable (a zero gradient).
 *   seg_bilinear_pad_fwd  seg_bilinear_fwd with a destination window: the resized Ho x Wo map lands at
 *                         (top, left) of the Hd x Wd map y (a pitched channel slice), the rest of that
 *                         slice is set to zero: F.pad(F.interpolate(act(x), (Ho, Wo), 'bilinear'))
 *   seg_bilinear_pad_bwd  gx [N,Hi,Wi,C] gathered from the window of gy [N,Hd,Wd,C] alone */
int seg_skip_pool_fwd(int dtype, const void* y, long ldy, int N, int H, int W, int C, int pro_mode,
                      const float* pro_scale, const float* pro_shift, void* skip, long ldskip,
                      void* pooled, long ldpool, void* stream);
int seg_skip_pool_bwd_rows(int dtype, int N, int H, int W, int C);
int seg_skip_pool_bwd(int dtype, const void* g_skip, long ldgs, const void* g_pool, long ldgp,
                      const void* y, long ldy, int N, int H, int W, int C, int pro_mode,
                      const float* pro_scale, const float* pro_shift, void* gx, long ldgx,
                      float* partial, int rows, void* stream);
int seg_bilinear_pad_fwd(int dtype, const void* x, long ldx, int N, int Hi, int Wi, int C,
                         int pro_mode, const float* pro_scale, const float* pro_shift, void* y,
                         long ldy, int Ho, int Wo, int Hd, int Wd, int top, int left,
                         int align_corners, void* stream);
int seg_bilinear_pad_bwd(int dtype, void* gx, long ldgx, int N, int Hi, int Wi, int C, const void* gy,
                         long ldgy, int Ho, int Wo, int Hd, int Wd, int top, int left,
                         int align_corners, void* stream);

/* ---- ContextNet's fusion: bilinear resize + depthwise 3x3 without the upsampled map ------------
 * (csrc/contextnet.hip; segmentron/models/contextnet.py:180-183)
 * NHWC, fp32 and bf16, a channel pitch per operand, C a multiple of the 16-byte vector (4 / 8).
 * No atomics: bit-identical results on every launch.  Any h, w, H, W >= 1 (h == 1 or w == 1: scale
 * 0 on that axis).  U = F.interpolate(act(lo), (H, W), 'bilinear', align_corners) of lo [N,h,w,C],
 * act = the seg_bilinear_fwd prologue (pro_mode / scale / shift) applied to each source tap before
 * the blend; U is ZERO outside [0,H) x [0,W) (the padding belongs to the upsampled map), lives in
 * registers and LDS in fp32 and is never rounded to the activation dtype.  w9c: fp32 [9][C]
 * tap-major.
 *   seg_up_dw_rows   partial rows of a launch (pure host; 0: bad arguments).  kind 0: the forward's
 *                    statistics rows, kind 1: the backward's weight-gradient rows.  The launchers
 *                    take exactly this many.
 *   seg_up_dw_fwd    y[n,Y,X,c] = sum_{i,j in -1..1} w9c[(i+1)*3+(j+1)][c] * U[n,Y+i,X+j,c].
 *                    stat_partial (nullable): [rows][2][C] = sum | sum of squares of the fp32
 *                    outputs, what seg_dwconv3x3 hands to seg_bn_finalize_p.
 *   seg_up_dw_bwd    one pass over dy [N,H,W,C] and lo: d_up [N,H,W,C] = the correlation of dy with
 *                    the flipped taps, in the activation dtype (no mask: nothing stands between the
 *                    resize and the convolution; seg_bilinear_bwd takes it next), and
 *                    partial_w [rows][9][C] = sum dy[Y,X] * U[Y+i,X+j] with U recomputed from lo
 *                    (reduce with seg_dwconv3x3_wgrad_finalize). */
int seg_up_dw_rows(int dtype, int N, int H, int W, int C, int kind);
int seg_up_dw_fwd(int dtype, const void* lo, long ldlo, int N, int h, int w, int C, int pro_mode,
                  const float* pro_scale, const float* pro_shift, const float* w9c, void* y,
                  long ldy, int H, int W, int align_corners, float* stat_partial, int rows,
                  void* stream);
int seg_up_dw_bwd(int dtype, const void* dy, long lddy, const void* lo, long ldlo, int N, int h,
                  int w, int C, int pro_mode, const float* pro_scale, const float* pro_shift,
                  const float* w9c, void* d_up, long ldd, int H, int W, int align_corners,
                  float* partial_w, int rows, void* stream);

/* ---- F.interpolate(mode='bilinear') ---------------------------------------------------------
 * Replaces segmentron/models/deeplabv3_plus.py:39,44,71; segmentron/modules/module.py:64,96;
 * segmentron/models/segbase.py:83.  NHWC -> NHWC with optional prologue and per-(n,c) multiplier. */
int seg_bilinear_fwd(int dtype, const void* x, long ldx, int N, int Hi, int Wi, int C,
                     int pro_mode, const float* pro_scale, const float* pro_shift,
                     const float* chan_mul, void* y, long ldy, int Ho, int Wo, int align_corners,
                     void* stream);
int seg_bilinear_bwd(int dtype, void* gx, long ldgx, int N, int Hi, int Wi, int C, const void* gy,
                     long ldgy, int Ho, int Wo, int align_corners, void* stream);
/* nn.Upsample(scale_factor=2^shift, mode='nearest') fused with the running sum of HRNet's
 * cross-resolution fuse (segmentron/models/backbones/hrnet.py:186,215-229):
 * y = post_relu?( act_x(x) + act_r(r[n, h>>shift, w>>shift]) ); backward of r = block sums. */
int seg_nearest_add(int dtype, const void* x, long ldx, int mode_x, const float* sx,
                    const float* tx, const void* r, long ldr, int mode_r, const float* sr,
                    const float* tr, int shift, int post_relu, void* y, long ldy, int N, int H,
                    int W, int C, void* stream);
int seg_nearest_sum_bwd(int dtype, const void* g, long ldg, int N, int H, int W, int C, int shift,
                        void* gr, long ldgr, void* stream);
/* Model boundary: NHWC logits (C valid channels, pitch ldx) -> NCHW float32 [N,C,Ho,Wo] and back. */
int seg_upsample_to_nchw(int dtype, const void* x, long ldx, int N, int Hi, int Wi, int C,
                         float* out, int Ho, int Wo, int align_corners, void* stream);
int seg_upsample_to_nchw_bwd(int dtype, void* gx, long ldgx, int N, int Hi, int Wi, int C,
                             const float* gy, int Ho, int Wo, int align_corners, void* stream);
/* Input boundary: NCHW float32 image [N,Cin,H,W] -> NHWC [N,H,W,16/sizeof(elem)] zero-padded. */
int seg_nchw_to_nhwc_pad(int dtype, const float* x, int N, int Cin, int H, int W, void* y,
                         void* stream);

/* ---- fused bilinear upsample -> log-softmax -> NLL (ignore_index), mean over valid pixels ------
 * Replaces F.interpolate(mode='bilinear', align_corners) of the head's logits
 * (segmentron/models/deeplabv3_plus.py:44, pspnet.py:34, fcn.py:28) + F.cross_entropy
 * (segmentron/solver/loss.py:16-46: nn.CrossEntropyLoss(ignore_index=-1)) without materialising
 * the [N, C, H, W] float32 logits.  lo: [N, Hi, Wi, ld] logits in `dtype` (C <= 32 classes, ld a
 * vector-padded pitch); target: int64 [N, H, W]; loss_out: float32[2] = (mean loss, 1 / number
 * of valid pixels); ws: >= 2 * seg_upsample_ce_blocks(N, H, W) doubles.  Backward: dlo
 * [N, Hi, Wi, lddlo] in `dtype` (channels >= C written as zeros) = grad_out[0] * dLoss/dlo,
 * up-sampling factors up to 16.1 (output-stride-4, -8 and -16 heads).  It runs as a row pass and a
 * column pass around a float32 workspace [N, H, Wi, C] that the caller provides (the entry point
 * does not allocate): ws of ws_bytes >= seg_upsample_ce_bwd_ws_bytes(N, H, Wi, C) bytes (that
 * query returns -1 where an int cannot hold the size).  Deterministic (fixed-order float64 /
 * gather reductions, no atomics). */
int seg_upsample_ce_blocks(int N, int H, int W);
int seg_upsample_ce_bwd_ws_bytes(int N, int H, int Wi, int C);
int seg_upsample_ce_fwd(int dtype, const void* lo, long ld, int N, int Hi, int Wi, int C,
                        const long* target, int H, int W, long ignore_index, int align_corners,
                        double* ws, float* loss_out, void* stream);
int seg_upsample_ce_bwd(int dtype, const void* lo, long ld, int N, int Hi, int Wi, int C,
                        const long* target, int H, int W, long ignore_index, int align_corners,
                        const float* loss_out, const float* grad_out, void* dlo, long lddlo,
                        float* ws, long ws_bytes, void* stream);

/* ---- DUpsampling (segmentron/models/dunet.py:90-117) on the low-resolution NHWC tensor ---------
 * lo: [N, h, w, ld] output of the module's 1x1 convolution in `dtype`, s*s*C valid channels
 * (1 <= C <= 32 classes, s >= 1, ld >= s*s*C and a multiple of the 16-byte vector).  The
 * reference's three permute / view rounds amount to
 *     out[n, k, hh*s + a, ww*s + b] = lo[n, hh, ww, (a*s + b)*C + k]
 * seg_dup_ce_fwd/bwd: F.cross_entropy(out, target, ignore_index), mean over valid pixels, on lo
 * itself; target int64 [N, h*s, w*s] read in place; loss_out float32[2] = (mean loss, 1 / valid
 * count), NaN and 0 when no pixel is valid; labels outside [0, C) are ignored too; ws >= 2 *
 * seg_dup_ce_blocks(...) doubles (-1: bad geometry).  dlo [N, h, w, lddlo] in `dtype` =
 * grad_out[0] * loss_out[1] * (softmax - onehot), zeros for invalid pixels and for channels >=
 * s*s*C.  Arithmetic of seg_point_ce_fwd/bwd; deterministic, no atomics.
 * seg_dup_to_nchw: the materialised float32 [N, C, h*s, w*s]; seg_dup_to_nchw_bwd: its inverse,
 * float32 NCHW gradient gy -> gx [N, h, w, ldgx] in `dtype` (pad channels zero). */
int seg_dup_ce_blocks(int dtype, long ld, int N, int h, int w, int s, int C);
int seg_dup_ce_fwd(int dtype, const void* lo, long ld, int N, int h, int w, int s, int C,
                   const long* target, long ignore_index, double* ws, float* loss_out,
                   void* stream);
int seg_dup_ce_bwd(int dtype, const void* lo, long ld, int N, int h, int w, int s, int C,
                   const long* target, long ignore_index, const float* loss_out,
                   const float* grad_out, void* dlo, long lddlo, void* stream);
int seg_dup_to_nchw(int dtype, const void* lo, long ld, int N, int h, int w, int s, int C,
                    float* out, void* stream);
int seg_dup_to_nchw_bwd(int dtype, void* gx, long ldgx, int N, int h, int w, int s, int C,
                        const float* gy, void* stream);

/* ---- PointRend point head (segmentron/models/pointrend.py:32-195, csrc/pointrend.hip) ---------
 * Maps are addressed through strides: element (n, pixel h*W + w, channel c) at
 * x + n*sn + (h*W + w)*sp + c*sc (NHWC activation: sn = H*W*ld, sp = ld, sc = 1; NCHW float32:
 * sn = C*H*W, sp = 1, sc = H*W).  pts: fp32 [N][P][2] (width, height) in [0, 1].  Point rows:
 * [N*P][ld] in their own dtype.  Deterministic: no float atomics.
 *   seg_point_sample      rows y[n*P + p][col + c] = F.grid_sample(x, 2p - 1, align_corners=False,
 *                         padding 'zeros'), bilinear or (nearest = 1) std::nearbyint taps; the
 *                         coarse and fine features of pointrend.py:63-66 land side by side
 *   seg_point_sample_bwd  dx NHWC [N,H,W,lddx] channels [0, C) (every pixel written) = the
 *                         bilinear backward of rows g[.][col + c]; ws: seg_point_sample_bwd_ws ints
 *                         (points bucketed by cell, each pixel sums its points in a fixed order)
 *   seg_point_uncertainty u = -(top1 - top2) of the C channels: per pixel (pts = NULL, u [N][H*W])
 *                         or of the rank-0 / rank-1 planes interpolated at the points (u [N][P])
 *   seg_point_topk        idx int64 [N][K] = the K largest of keys [N][L], ties to the lower
 *                         index, ascending; ws: seg_point_topk_ws ints (radix select)
 *   seg_point_coords      over != NULL: pts[n] = (over[n][idx[n][j]] for j < K, then cover[n]);
 *                         over == NULL: pixel centres of idx on an H x W grid (pointrend.py:170-172)
 *   seg_point_scatter     y[n, idx[n][p], c] = rend[n*P + p][c] (float32 map, strides as above)
 *   seg_point_resize      F.interpolate(x, (Ho, Wo), 'bilinear', align_corners) -> float32 NCHW
 *   seg_point_ce_fwd/bwd  mean NLL of log_softmax over the C columns of rows x against target
 *                         int64 [R] (ignore_index; targets outside [0, C) are ignored too);
 *                         loss_out float32[2] = (loss, 1 / valid rows), NaN when none is valid;
 *                         ws >= 2 * seg_point_ce_blocks(R) doubles */
int seg_point_sample(int dtype_x, const void* x, long sn, long sp, long sc, int N, int H, int W,
                     int C, const float* pts, int P, int nearest, int dtype_y, void* y, long ldy,
                     int col, void* stream);
int seg_point_sample_bwd_ws(int N, int H, int W, int P);
int seg_point_sample_bwd(int dtype_g, const void* g, long ldg, int col, const float* pts, int N,
                         int P, int H, int W, int C, int dtype_x, void* dx, long lddx, int* ws,
                         void* stream);
int seg_point_uncertainty(int dtype, const void* x, long sn, long sp, long sc, int N, int H, int W,
                          int C, const float* pts, int P, float* u, void* stream);
int seg_point_topk_ws(int N, long L);
int seg_point_topk(const float* keys, int N, long L, int K, long* idx, int* ws, void* stream);
int seg_point_coords(const float* over, const long* idx, int N, int L, int K, const float* cover,
                     int P, int H, int W, float* pts, void* stream);
int seg_point_scatter(int dtype_r, const void* rend, long ldr, const long* idx, int N, int P,
                      int C, float* y, long sn, long sp, long sc, void* stream);
int seg_point_resize(int dtype, const void* x, long sn, long sp, long sc, int N, int Hi, int Wi,
                     int C, float* y, int Ho, int Wo, int align_corners, void* stream);
int seg_point_ce_blocks(long R);
int seg_point_ce_fwd(int dtype, const void* x, long ldx, long R, int C, const long* target,
                     long ignore_index, double* ws, float* loss_out, void* stream);
int seg_point_ce_bwd(int dtype, const void* x, long ldx, long R, int C, const long* target,
                     long ignore_index, const float* loss_out, const float* grad_out, void* dx,
                     long lddx, void* stream);

/* ---- stride-2 depthwise 3x3 (padding 1, dilation 1): fused backward --------------------------
 * One pass over dy [N,(H+1)/2,(W+1)/2,C] and x [N,H,W,C] (+ prologue): g = masked data gradient,
 * partial_w [grid_y][9][C] (reduce with seg_dwconv3x3_wgrad_finalize), partial_bn [grid_y][2][C]
 * (nullable) = (sum g, sum g*x_raw).  w_c9: torch's [C,1,3,3] fp32.  grid_y from
 * seg_dwconv3x3_s2_grid_y (-1: a non-positive size, or C not a positive multiple of 4). */
int seg_dwconv3x3_s2_grid_y(int C, int N, int H, int W);
int seg_dwconv3x3_s2_bwd_fused(int dtype, const void* dy, long lddy, const void* x, long ldx, int N,
                               int H, int W, int C, const float* w_c9, int pro_mode,
                               const float* pro_scale, const float* pro_shift, void* g, long ldg,
                               float* partial_w, float* partial_bn, int grid_y, void* stream);

/* ---- torch.optim.SGD(momentum, weight_decay) step over many tensors -------------------------
 * Replaces the optimizer the reference builds in segmentron/solver/optimizer.py:45-50 (dampening
 * 0, no Nesterov): d = g + wd*p; m = first ? d : momentum*m + d; p -= lr*m, fp32.
 * params / grads / bufs: HOST arrays of ntensors device pointers; numel / group: host arrays;
 * lr_dev / wd_dev: DEVICE float arrays indexed by parameter group (a captured graph of the step
 * follows the LR schedule: the host rewrites these floats between replays). */
int seg_sgd_multi_tensor(int ntensors, const void* const* params, const void* const* grads,
                         const void* const* bufs, const long* numel, const int* group,
                         const float* lr_dev, const float* wd_dev, float momentum, int first,
                         void* stream);
/* Multi-tensor weight packing (r04): njobs jobs "fp32 [O][C] contiguous -> dtype [O][C]
 * (transpose = 0) or [C][O] (transpose = 1)" in as few launches as the 32-job / 1024-tile
 * argument block allows: the GEMM operands of the non-folded 1x1 convolutions, re-made once per
 * optimizer step (torch: one cast / transposing copy per tensor and direction).  srcs / dsts / O /
 * C / transpose: HOST arrays. */
int seg_pack_multi(int dtype, int njobs, const void* const* srcs, const void* const* dsts,
                   const int* O, const int* C, const int* transpose, void* stream);

/* ---- pixAcc / mIoU counters ------------------------------------------------------------------
 * Replaces segmentron/utils/score.py:83-113 (batch_pix_accuracy: argmax of the logits TRUNCATED
 * to integers; batch_intersection_union: argmax + three torch.histc on the CPU).  counters:
 * int64 [2 + 3*nclass] = correct, labelled, inter[nclass], pred[nclass], lab[nclass], ACCUMULATED
 * (zero them to start an evaluation).  _nchw takes fp32 NCHW logits; _upsample takes the
 * network's low-resolution NHWC logits and applies the final bilinear resize on the fly with
 * seg_upsample_to_nchw's arithmetic. */
int seg_metric_update_nchw(const float* logits, int N, int C, int H, int W, const long* target,
                           int nclass, long* counters, void* stream);
int seg_metric_update_upsample(int dtype, const void* lo, long ld, int N, int Hi, int Wi, int C,
                               const long* target, int H, int W, int align_corners, int nclass,
                               long* counters, void* stream);

/* ---- criss-cross attention (CCNet) ------------------------------------------------------------
 * Replaces the reference's CUDA extension segmentron/modules/csrc/criss_cross_attention/
 * ca_cuda.cu:8-177 (+ the softmax of cc_attention.py:66), NHWC.  Entry z of pixel (y, x):
 * z < W -> (y, z); else i = z - W, (i < y ? i : i + 1, x).  L = W + H - 1 <= 512.
 * att / de: fp32 [N, H, W, L].
 *   seg_cca_attention     : att = softmax_z(q[p] . k[partner(p, z)])
 *   seg_cca_map           : out = gamma * sum_z w b[partner] (+ res); transposed = 1 sums over
 *                           the pixels attending TO p (dv, dk); raw (nullable) = the plain sum
 *   seg_cca_attention_bwd : de = softmax backward of dA = scale * dout[p] . v[partner(p, z)] */
int seg_cca_attention(int dtype, const void* q, long ldq, const void* k, long ldk, int N, int H,
                      int W, int C, float* att, void* stream);
int seg_cca_attention_bwd(int dtype, const void* dout, long lddo, const void* v, long ldv, int N,
                          int H, int W, int C, const float* att, const float* scale, float* de,
                          void* stream);
int seg_cca_map(int dtype, const float* wt, const void* b, long ldb, int N, int H, int W, int C,
                int transposed, const float* gamma, const void* res, long ldres, void* out,
                long ldo, void* raw, long ldraw, void* stream);

/* ---- DANet position / channel attention (segmentron/modules/module.py:100-162).  The two
 * torch.bmm of each module are GEMMs on the convolution entry points (seg_conv_gemm_fwd = NT,
 * seg_conv_gemm_wgrad = TN); the softmax between them (nn.Softmax(dim=-1), module.py:110,141):
 *   seg_row_softmax     : a[r][j] = softmax_j(sign * e[r][j]) for j < L, 0 for L <= j < Lp
 *   seg_row_softmax_bwd : de[r][j] = sign * a[r][j] * (g[r][j] - sum_j a[r][j] g[r][j])
 * e / a / g / de: row-major [R][pitch], element type DT_F32 (0) or DT_BF16 (1) given per operand;
 * sign = -1 is CAM's softmax(max(energy) - energy) (shift invariance). */
int seg_row_softmax(const void* e, int dt_in, long lde, void* a, int dt_out, long lda, long R,
                    int L, int Lp, float sign, void* stream);
int seg_row_softmax_bwd(const void* a, int dt_a, long lda, const void* g, int dt_g, long ldg,
                        void* de, int dt_out, long ldde, long R, int L, int Lp, float sign,
                        void* stream);
/* ---- SyncBatchNorm statistics exchange: one-hop xGMI peer writes ----------------------------
 * Replaces, for the data-parallel path of tools/train.py:73-79 (convert_sync_batchnorm +
 * DistributedDataParallel), the two collectives per BatchNorm that torch's SyncBatchNorm issues
 * (torch/nn/modules/_functions.py:49-74 all_gather of mean/invstd/count, :140 all_reduce of the
 * backward sums): an in-place float64 SUM over the ranks of one node, every rank writing its
 * vector into a mailbox on each peer (csrc/p2p.hip).  One process per GPU.
 *   seg_p2p_create       : this rank's mailbox (uncached device memory), slot_bytes % 128 == 0
 *                          bounds one message; *handle_out is an opaque object of THIS process
 *   seg_p2p_ipc_handle   : the 64-byte hipIpcMemHandle_t of the mailbox, to be sent to the peers
 *   seg_p2p_connect      : handles = [world][64] bytes in rank order (own entry ignored)
 *   seg_p2p_all_reduce_f64 / _f32: buf[n] <- sum over ranks (added in rank order: bit-identical
 *                          on every rank), on `stream` (capturable); every rank must issue the
 *                          same sequence of calls
 *   seg_p2p_status       : synchronises; 3 = a peer failed to publish within the time limit (the
 *                          kernel stops waiting instead of hanging, and this and every later
 *                          exchange returns NaN — the error word is never reset)
 *   seg_p2p_set_timeout  : bound of one in-kernel wait in seconds (default 600)                 */
int seg_p2p_create(int rank, int world, long slot_bytes, void** handle_out);
int seg_p2p_ipc_handle(void* handle, void* out64);
int seg_p2p_connect(void* handle, const void* handles);
int seg_p2p_all_reduce_f64(void* handle, void* buf, int n, void* stream);
int seg_p2p_all_reduce_f32(void* handle, void* buf, int n, void* stream);
int seg_p2p_status(void* handle);
int seg_p2p_set_timeout(void* handle, double seconds);
int seg_p2p_destroy(void* handle);
/* The BatchNorm finalize steps with the exchange INSIDE the kernel (column sums of this rank's
 * partial rows -> peer writes -> finalize): a SyncBatchNorm then costs the same single launch per
 * direction as a plain BatchNorm.  p2p = handle of seg_p2p_create; Rb <= 1024; ws (>= 128 C
 * doubles) is needed for R > 1024 as in seg_bn_finalize_p; count_out /
 * count_dev: the GLOBAL element count (float64, device) produced by the forward step and read by
 * the backward ones; grad_scale multiplies dgamma / dbeta (1 / world, see seg_bn_bwd_finalize_s). */
int seg_bn_finalize_p_sync(void* p2p, const float* partial, long R, double local_count,
                           const float* gamma, const float* beta, float eps, float momentum,
                           float* running_mean, float* running_var, float* mean, float* invstd,
                           float* scale, float* shift, int C, const float* mean_offset,
                           double* count_out, double* ws, void* stream);
int seg_bn_bwd_finalize_p_sync(void* p2p, const float* partial, long R, const double* count_dev,
                               const float* mean, const float* invstd, const float* gamma,
                               float* dgamma, float* dbeta, float* c0, float* c1, int C,
                               double grad_scale, double* ws, void* stream);
int seg_dw_bwd_finalize_sync(void* p2p, const float* partial_bn, int Rb, const double* count_dev,
                             const float* mean, const float* invstd, const float* gamma,
                             float* dgamma, float* dbeta, float* c0, float* c1,
                             const float* partial_w, int Rw, float* dw_c9, int C,
                             double grad_scale, void* stream);
int seg_fold_bwd_finalize_sync(void* p2p, const float* dsdt, int rows, const double* count_dev,
                               const float* mean, const float* invstd, const float* gamma,
                               const float* scale, float* dgamma, float* dbeta, float* c0,
                               float* c1, int C, double grad_scale, void* stream);

/* ---- LEDNet: dense 3-tap line convolutions and the split-shuffle tail (csrc/conv_line.hip) ----
 * Replace the nn.Conv2d (3,1) / (1,3) layers of SSnbt.branch1 / branch2
 * (segmentron/models/lednet.py:76-102: stride 1, padding = dilation along ONE axis, no bias):
 *   y[n,h,w,o] = sum_t sum_c act(x[n, h + (t-1)*dil*[axis==0], w + (t-1)*dil*[axis==1], c])
 *                            * wp[o][t][c]  (+ add[n,h,w,o])
 * NHWC, C == O in {16, 32, 64}, axis 0 = H (a [O,C,3,1] parameter), 1 = W ([O,C,1,3]); wp is the
 * [O][3*C] packing seg_conv_gemm_fwd takes, in `dtype`.  x, y and add have their own row pitches
 * (channel slices of wider buffers); channels outside the slice are never touched.  The prologue
 * is applied in float32 and, for bf16, rounded once before the MFMA; a tap outside its own image
 * (axis 0) or row (axis 1) is zero AFTER the prologue.  add (nullable): y = acc + add, rounded
 * once.  stat_partial (nullable): fp32 [rows][2][C], rows = seg_conv_line_geom(.., 1), sums and
 * sums of squares of the values AS STORED (after add and rounding), for seg_bn_finalize_p.
 * The data gradient is the same call on dy with the weights repacked as [C][2-t][O].
 *   seg_conv_line_ok   : 1 if the kernels serve (dtype, C, axis, dil); pure host query
 *   seg_conv_line_geom : what = 0 pixels per tile, 1 grid (= partial rows), 2 tiles per block,
 *                        3 pixels per staging trip of the weight gradient; -1 on bad input
 *   seg_conv_line_wgrad: partial fp32 [splits][O][C][3] (splits from seg_conv_line_wgrad_splits;
 *                        the memory layout of the [O,C,3,1] / [O,C,1,3] parameter itself),
 *                        dW[o][c][t] = sum_p dy[p][o] * act(x)[p + tap t][c]; sum with seg_colsum.
 * No atomics, fixed summation order: every launch is bit-identical.
 * C == O == 40 (EDANet's EDABlock, segmentron/models/edanet.py:107-116) is served on packed or
 * pitched 40-channel tensors (no padding: in bf16 the void upper half of the third 16-channel
 * k-step is masked in registers; the weight packing stays [O][3*C] with C = 40) by the
 * seg_conv_line_bias_* entries and the weight gradient.  seg_conv_line_ok / _geom / _fwd keep the
 * classes they have always had and refuse C = 40.
 *   seg_conv_line_bias_ok / _geom: the queries above for C in {16, 32, 40, 64}
 *   seg_conv_line_bias_fwd: seg_conv_line_fwd with a per-channel float32 bias [C] (nullable),
 *                        added to the accumulators BEFORE add, the rounding and the statistics;
 *                        the zero padding of a consumer applies after it.  With the data
 *                        gradient's weights and stat_partial, row sums [.][0][c] are the
 *                        per-channel sums of dx as stored: the bias gradient of a biased
 *                        producer convolution that feeds x directly.
 *                        For C in {16, 32, 64} seg_conv_line_fwd is this call with bias = NULL.  */
int seg_conv_line_ok(int dtype, int C, int axis, int dil);
int seg_conv_line_geom(int dtype, int N, int H, int W, int C, int what);
int seg_conv_line_wgrad_splits(int dtype, int N, int H, int W, int C);
int seg_conv_line_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                      const void* wp, int axis, int dil, int pro_mode, const float* pro_scale,
                      const float* pro_shift, void* y, long ldy, const void* add, long ldadd,
                      float* stat_partial, void* stream);
int seg_conv_line_bias_ok(int dtype, int C, int axis, int dil);
int seg_conv_line_bias_geom(int dtype, int N, int H, int W, int C, int what);
int seg_conv_line_bias_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                           const void* wp, const float* bias, int axis, int dil, int pro_mode,
                           const float* pro_scale, const float* pro_shift, void* y, long ldy,
                           const void* add, long ldadd, float* stat_partial, void* stream);
int seg_conv_line_wgrad(int dtype, const void* x, long ldx, const void* dy, long lddy, int N,
                        int H, int W, int C, int axis, int dil, int pro_mode,
                        const float* pro_scale, const float* pro_shift, float* partial, int splits,
                        void* stream);
/* SSnbt.forward's tail (lednet.py:117-128: the two branches' last BatchNorm + ReLU, torch.cat,
 * + x, ReLU, channel_shuffle(groups=2)) in one pass over P = N*H*W pixels, C in {32, 64, 128}:
 *   out[p][2i + g] = relu(relu(y_g[p][i]*s_g[i] + t_g[i]) + x[p][g*C/2 + i]),  g < 2, i < C/2
 * and its backward, unshuffled:  gm[p][g*C/2 + i] = gout[p][2i + g] * (out[p][2i + g] > 0).
 *   seg_ssnbt_tail_geom: what = 0 threads, 1 grid, 2 loop trips; -1 on bad input                */
int seg_ssnbt_tail_geom(int dtype, long P, int C, int what);
int seg_ssnbt_tail_fwd(int dtype, const void* y0, long ldy0, const float* s0, const float* t0,
                       const void* y1, long ldy1, const float* s1, const float* t1, const void* x,
                       long ldx, void* out, long ldout, long P, int C, void* stream);
int seg_ssnbt_tail_bwd(int dtype, const void* gout, long ldgout, const void* out, long ldout,
                       void* gm, long ldgm, long P, int C, void* stream);

/* ---- EDANet: a pair of line convolutions in one launch (csrc/conv_line_pair.hip) ---------------
 * EDABlock runs its line convolutions as conv3x1 -> conv1x3 with only the first bias in between
 * (segmentron/models/edanet.py:127-128, 132-133).  C == O == 40, one dilation for both:
 *   mid = lineA(act(x)) + bias_a  (rounded to `dtype` as a store rounds it)
 *   y   = lineB(mid) + bias_b (+ add)
 * order 0: (A, B) = (H, W), order 1: (W, H).  One block owns one whole line along B (a row / a
 * column) and keeps its `mid` in LDS; a tap of stage B outside the line is zero AFTER bias_a.
 * wa / wb: the [O][3*C] packings of seg_conv_line_fwd.  mid (nullable): also stored to global
 * memory.  stat_partial (nullable): fp32 [rows][2][C] of y as stored; mid_sums (nullable): fp32
 * [rows][C] per-channel sums of mid as stored; rows = seg_conv_line_pair_rows.  y and mid are
 * bit-identical to two seg_conv_line_bias_fwd launches; no atomics, fixed summation order.
 * The data gradient of an order-0 pair is the order-1 pair on dy with the weights repacked
 * [C][2-t][O] (B's first) and no biases: its mid is d mid, its mid_sums are d bias_a.
 *   seg_conv_line_pair_ok  : 1 if (dtype, C, line length L along B, dil) is served: C == 40 and
 *                            the weights of both convolutions + L * (C * sizeof + 16) bytes of
 *                            `mid` fit 64 KB of LDS (L <= 436 in bf16, 136 in float32); pure
 *                            host query
 *   seg_conv_line_pair_rows: blocks = rows of stat_partial / mid_sums; -1 on bad input          */
int seg_conv_line_pair_ok(int dtype, int C, int L, int dil);
int seg_conv_line_pair_rows(int N, int H, int W, int order);
int seg_conv_line_pair_fwd(int dtype, const void* x, long ldx, int N, int H, int W, int C,
                           const void* wa, const float* bias_a, const void* wb,
                           const float* bias_b, int order, int dil, int pro_mode,
                           const float* pro_scale, const float* pro_shift, void* mid, long ldmid,
                           void* y, long ldy, const void* add, long ldadd, float* stat_partial,
                           float* mid_sums, void* stream);

/* ---- EDANet: channel placement for the down-sampler's concat (csrc/edanet.hip) ----------------
 * DownsamplerBlock (segmentron/models/edanet.py:90-97) concatenates a stride-2 convolution with a
 * 2x2 max-pool of its input at channel offsets (12, 45) that are no whole 16-byte vector.
 *   dst[p][c] = c < C ? src[p][c] : 0   for p < P, c < Cz  (C <= Cz <= 4096)
 * element-wise, any channel alignment; src and dst are already offset to their first channel and
 * have their own row pitches (lds >= C, ldd >= Cz).  Forward: the pooled channels into their
 * slice of the concat buffer (Cz = C); backward: that slice of the gradient into an aligned
 * tensor of the pool's width with zeros in its pad channels (Cz > C).                          */
int seg_chan_copy(int dtype, const void* src, long lds, void* dst, long ldd, long P, int C,
                  int Cz, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEGMENTRON_HIP_H */
