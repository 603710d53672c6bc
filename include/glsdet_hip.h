/* glsdet_hip.h -- C ABI of libglsdet_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for ONE path of WUTCM-Lab/GLSDet: the detection forward pass
 * (backbone -> PAFPN / GL-fusion neck -> decoupled head -> decode -> NMS).  The reference
 * is pure Python; the native kernels it reaches live in torch ATen/cuDNN and
 * torchvision.  Each entry point below replaces one such call site (reference file:line
 * given per function, paths relative to the reference root, drone/ = yolox-drone/).
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless it says host.
 *  - activations are NHWC "views": base pointer + element strides for n/h/w, channels
 *    contiguous.  A view can therefore be a quadrant, a channel slice of a concat buffer
 *    or a row band of a larger tensor without any copy.
 *  - dtype: GLSDET_F16 (fp16 storage, fp32 accumulate) or GLSDET_F32 (exact-f32 MFMA).
 *  - `stream` is a hipStream_t passed as void*.  All entry points are asynchronous on
 *    that stream, never synchronise, never allocate, and may be stream-captured.
 *  - return value: 0 = ok, negative = GLSDET_E_* (nothing was launched); the text of
 *    the last error of the calling thread is available from glsdet_last_error().
 *  - every view carries the bounds of the allocation it lives in; each launch checks on
 *    the host that the extreme addresses it can touch lie inside (a kernel is never
 *    launched on operands that do not fit).
 */
#ifndef GLSDET_HIP_H
#define GLSDET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLSDET_ABI_VERSION 17

enum { GLSDET_F16 = 0, GLSDET_F32 = 1 };
enum { GLSDET_ACT_NONE = 0, GLSDET_ACT_SILU = 1, GLSDET_ACT_RELU = 2, GLSDET_ACT_LRELU = 3,
       GLSDET_ACT_GELU = 4 /* exact erf form, nn.GELU() */, GLSDET_ACT_SIGMOID = 5,
       /* OR-ed into `act`: the residual is added BEFORE the activation, act(conv*scale+bias+res)
        * (ResNet Bottleneck: `out += identity; out = relu(out)`, ufp/mmdet/models/backbones/
        * resnet.py:292-301).  Without the flag the order is act(conv*scale+bias) + res
        * (YOLOX Bottleneck, drone/models/base/darknet.py:61-63).                            */
       GLSDET_ACT_RES_FIRST = 0x100 };
/* Accuracy of the activation epilogues (tests/act_reference.py derives each bound, tests/test_act_exact.py enforces it on
 * every kernel variant).  v = the fp32 pre-activation conv*scale+bias (+ res with GLSDET_ACT_RES_FIRST), y the float64
 * value of the activation at v, u = 2^-24.  The result is the rounding (nearest even; fp16 overflows to inf) to the output
 * type of a value within tol of y:
 *     NONE, RELU   tol = 0 (the one rounding to the output type)
 *     LRELU        v > 0 ? v : 0.1f * v.  F32: exactly float(0.1f * v); F16: tol = u |y| (the fp32 product, rounded again)
 *     SILU         F16: v * rcp(1 + exp2(v * -log2e)), v_exp_f32 / v_rcp_f32:  tol = (8 + 2 |v| sigmoid(-v)) u |y| + 2^-120
 *                  F32, and glsdet_dwconv2d in both dtypes: v / (1 + expf(-v)):  tol = 6 u |y| + 2^-120
 *     SIGMOID      1 / (1 + expf(-v)).  F32: tol = 6 u |y| + 2^-120; F16: tol = 4 u (|y| + |v| / 2)
 *     GELU         0.5f * v * (1 + erff(v * 0.70710678f)): tol = 4 u (|y| + |v| / 2) -- 1 + erff cancels for negative v
 * With a residual added after the activation one more fp32 rounding of the sum: tol + u |y + res|.  An fp16 output with a
 * residual is rounded ONCE, from the fp32 sum.  Every kernel variant (tile_hint) gives the same bits for the same problem,
 * and the vector epilogue (no residual) the same bits as the scalar one (GLSDET_ACT_RES_FIRST), zeros compared as zeros.
 * Special values: +-0 keep their sign through NONE, LRELU, SILU and GELU; a NaN pre-activation gives NaN EXCEPT under RELU,
 * where relu(NaN) = 0 (fmaxf / v_max semantics; torch.relu gives NaN); +inf gives +inf (SIGMOID: 1); -inf gives -inf under
 * NONE and LRELU, 0 under RELU and SIGMOID, and NaN under SILU and GELU (-inf * 0).
 * glsdet_dwconv2d / glsdet_dwconv2d_dilated accept NONE, SILU, RELU and LRELU only; glsdet_csp_fused SILU only;
 * glsdet_resnet_stem_pool has RELU compiled in; every other entry point with an `act` takes all six codes. */
enum {
  GLSDET_OK = 0,
  GLSDET_E_ARG = -1,      /* inconsistent shapes / unsupported parameter            */
  GLSDET_E_BOUNDS = -2,   /* a view reaches outside its allocation                  */
  GLSDET_E_ALIGN = -3,    /* pointer / stride not 16-byte compatible                */
  GLSDET_E_HIP = -4,      /* HIP runtime error (text in glsdet_last_error)          */
  GLSDET_E_CAPACITY = -5  /* workspace too small                                    */
};

/* NHWC view.  Strides in ELEMENTS of `dtype`; channel stride is 1.
 * Addressing range.  Strides are 64-bit and every entry point addresses through them at full width: a view may lie, and
 * its images may be, more than 2^31 (and 2^32) bytes away from alloc_lo and from each other (tests/test_far_addresses.py).
 * The exceptions, all refused on the host before any launch:
 *   - the INPUT of the conv family (glsdet_conv2d, _multi, _chain, glsdet_bottleneck, glsdet_conv2d_gnstats,
 *     glsdet_csp_fused) is read through 32-bit buffer-descriptor offsets counted from alloc_lo: its ALLOCATION
 *     (alloc_hi - alloc_lo) must be below 2^31 - 1 bytes, else GLSDET_E_ARG "... exceeds the 2 GiB descriptor range".
 *     The limit is counted on the allocation, not on the view: one image sliced out of a batch tensor of 2 GiB or more is
 *     refused although the view is small.  glsdet_csp_fused applies the same limit to the allocation of y.
 *   - the persistent 1x1 variants (tile_hint 16 .. 31) read res, and 16 .. 28 also store y, through 32-bit offsets from
 *     the view's base (29 .. 31 store y through 64-bit ones, but the family keeps ONE limit): the SPAN of y and of res
 *     (bytes from the first to the last element of the view) must be below 2^31 - 1, else the hint "does not apply";
 *     tile_hint 0 then chooses another kernel, 1 is the generic kernel, both take any span.
 *   - glsdet_conv2d_grouped, glsdet_csp_fused, glsdet_bottleneck, glsdet_layernorm, glsdet_patch_merge and
 *     glsdet_window_attention decide "y overlaps x" on the spans of the two views, so two views whose images interleave
 *     (image strides far larger than an image) are refused as overlapping.                                          */
typedef struct glsdet_view {
  void*   base;            /* address of element (n=0,h=0,w=0,c=0)                    */
  int64_t sn, sh, sw;      /* element strides                                         */
  int32_t n, h, w, c;      /* logical extent                                          */
  int32_t dtype;           /* GLSDET_F16 / GLSDET_F32                                 */
  int32_t _pad;
  void*   alloc_lo;        /* [alloc_lo, alloc_hi) = allocation the view lives in     */
  void*   alloc_hi;
} glsdet_view;

/* ---------------------------------------------------------------------------------
 * conv2d + folded BatchNorm + activation (+ residual add)          reference call sites:
 *   drone/models/base/baseConv.py:15-16   act(bn(conv(x)))            (BaseConv)
 *   drone/models/base/darknet.py:61-62    y = conv2(conv1(x)) + x     (Bottleneck add)
 *   drone/models/base/yolox.py:31-44      predictors, Conv2d + bias
 *   drone/models/block/non_local/Identity_Conv.py:27-84   dense kxk conv + bias
 *   (mmdet twin: mmcv ConvModule at ufp/mmdet/models/backbones/csp_darknet.py:39-47)
 * y[n,ho,wo,co] = act( scale[co] * sum_{r,s,ci} x[n,ho*stride-pad+r,wo*stride-pad+s,ci]
 *                                              * w[co,r,s,ci] + bias[co] ) (+ res[n,ho,wo,co])
 * Implicit GEMM on MFMA, NHWC, LDS-staged weight and im2col tiles, fused epilogue.
 *  w      : packed [cout_pad][kpad] elements of x.dtype, k = (r*S + s)*x.c + ci,
 *           kpad = round_up(R*S*x.c, 64 bytes worth of elements), cout_pad = round_up(y.c, 32),
 *           zero filled (see glsdet_conv_weight_elems).
 *  scale/bias : fp32 [cout_pad]  (BN folded: scale = gamma/sqrt(var+eps), bias = beta-mean*scale;
 *           plain conv: scale = 1, bias = conv bias)
 *  res    : optional (base == NULL for none), same dtype/extent as y.
 *  x.c, y.c must be multiples of 8; y.dtype may be F32 while x.dtype is F16 (predictors).
 */
typedef struct glsdet_conv_desc {
  glsdet_view x, y, res;
  const void*  w;
  const float* scale;
  const float* bias;
  int32_t R, S, stride, pad, act;
  int32_t tile_hint;       /* which kernel runs the conv.  This table is the authority: csrc/conv_common.h decodes it once
                            * (decode_tile_hint) and every entry point refuses, with GLSDET_E_ARG when the op is built, a
                            * value that is not listed here -- nothing is recorded that could only fail at launch.
                            *   family   0 automatic | 1 generic kernel, tile chosen by the library | 2 halo kernel (stride-1
                            *            k x k) | 3 weight-stationary 1x1 | 4 halo, wave-private weight staging | 5 halo,
                            *            64-row cout tiles also for wide layers | 8..11 halo with the weight tiles in an
                            *            LDS-DMA ring | 12 / 13 its 8-wave form: 128 cout rows x 8 x 32 pixels per 512-thread
                            *            workgroup (no residual) | 16..31 the persistent LDS-DMA 1x1 kernel
                            *            (6 / 7, a persistent halo kernel, no longer exist)
                            *   cout tile  8, 10: 64 rows | 9, 11: 128 rows
                            *   k64      10, 11, 13: 64-byte channel chunks (8, 9, 12: 128-byte)
                            *   geometry 0x100 | h, 0x200 | h (h = 8..11, 13 only): ring kernel h on 10 x 12 resp. 6 x 21
                            *            pixel tiles (h = 13: 10 x 24 resp. 6 x 42) instead of 8 x 16 (8 x 32) -- fewer
                            *            wasted lanes on 50 x 84 / 25 x 42 maps
                            *   variant  16 + v, v = 0..15: row v of the table in csrc/conv_gemm.hip (tile, ring depth,
                            *            K panel, weight-resident, single shot); variant 19 (128 x 128 tile, three stages of
                            *            128-byte panels) takes no residual with an fp32 output: ring + fp32 residual tile
                            *            exceed the 160 KiB of LDS
                            *   tile     co << 16 | px: the generic kernel on a co x px tile -- 128x128, 64x128, 32x128,
                            *            64x64, and 128 << 16 | 0 = the 8-wave 128 x 256 tile (Cin a whole number of K
                            *            steps, no chained conv); glsdet_conv2d_multi has 128x128, 64x128, 64x64 only
                            *            (32x128 runs as 64x64; its batched form also 128x256 as 128x128)
                            *   kb64     bit 15 of a tile: 64-byte K steps
                            *   dbg      bits 8..10 of a tile: diagnostic switches (timing experiments; results invalid) */
} glsdet_conv_desc;

int     glsdet_conv2d(const glsdet_conv_desc* d, void* stream);
/* Up to 8 independent convolutions of ONE shape class (same R, S, stride, pad, Cin, Cout and
 * dtypes; extents, strides, weights, residuals may differ) as one launch of the generic kernel:
 * the four quadrant convs of Patch_Conv (drone/models/block/non_local/Identity_Conv.py:298-301),
 * the cls / reg tower convs of one head level (base/yolox.py:62-75).  Each alone is too small
 * to fill the chip.  tile_hint of d[0] applies (0 = auto; 8..11 = the grouped LDS-DMA ring kernel for 3x3 problems, meaning
 * as for glsdet_conv2d, refused with GLSDET_E_ARG where it does not apply).  Results are those of n glsdet_conv2d.
 * `w` may point at an ACTIVATION matrix (rows of x.c elements at a pitch of glsdet_conv_kpad elements, zero padded):
 * the batched products of the non-local block at ResNet widths are such 1x1 "convs" with per-image weights.
 * n = 9 .. 32 (round 3): the BATCHED form -- all descriptors must describe ONE geometry (extents, strides, epilogue, residual
 * or not: they may differ in the operand addresses only; the 8 images x 4 quadrants of a plug-in level), the generic
 * tiles only (tile_hint 0 or co << 16 | px); anything else is refused with GLSDET_E_ARG. */
int     glsdet_conv2d_multi(const glsdet_conv_desc* d, int32_t n, void* stream);
/* as glsdet_conv2d_tune, for the group: fastest tile_hint of the one-launch form and its time */
int     glsdet_conv2d_multi_tune(const glsdet_conv_desc* d, int32_t n, void* stream, int32_t* best_hint, float* best_us);
/* Build-time autotune: times every kernel / tile variant that applies to exactly this
 * problem on the device (synchronises; never recorded into a plan) and returns the fastest
 * tile_hint.  The output view is written with the conv result. */
int     glsdet_conv2d_tune(const glsdet_conv_desc* d, void* stream, int32_t* best_hint, float* best_us);
/* A conv (exactly as glsdet_conv2d, residual included) followed IN THE SAME LAUNCH by a 1x1 conv + folded BN + act on a
 * channel range of its result -- the two back-to-back BaseConvs of a CSPLayer / Bottleneck chain
 * (drone/models/base/darknet.py:58-63: `y = conv2(conv1(x))`; :96-107: conv1 -> m[0].conv1):
 *     y  = glsdet_conv2d(d)
 *     y2 = act2( scale2 * sum_{c < cin2} y[.., c0 + c] * w2[co2][c] + bias2 )          (w2 packed as for a 1x1 conv)
 * The workgroup that produced a tile multiplies it from LDS while it is still there: the 1x1 costs no launch and no
 * re-read of y.  It consumes the STORED (rounded) values in the k order of the stand-alone kernels, so y2 equals what
 * glsdet_conv2d on y would give, bit for bit.  Limits: x, y, y2 one dtype; y2.c <= 128; the channels [c0, c0+cin2) must
 * lie inside one cout tile of the kernel that runs d (else GLSDET_E_ARG: callers fall back to two launches).          */
typedef struct glsdet_conv_chain {
  glsdet_view y2;          /* y's n, h, w                                                        */
  const void*  w2;         /* [cout_pad(y2.c)][kpad(1,1,cin2)] elements of y.dtype               */
  const float* scale2;
  const float* bias2;
  int32_t act2, c0, cin2;
  int32_t flags;           /* 0 or GLSDET_CHAIN_SKIP_Y (ABI 13; the field was padding before)      */
} glsdet_conv_chain;
/* y is read by nothing but the chained conv: it is not stored (its view is still validated).  Needs c0 == 0, cin2 == y.c,
 * no residual.  The stride-2 BaseConv in front of a CSPLayer (drone/models/base/darknet.py:174-195: `dark3 = Sequential(
 * Conv(.., 3, 2), CSPLayer(..))`) + the layer's conv1 | conv2 then move the 3x3's output through LDS only.          */
#define GLSDET_CHAIN_SKIP_Y 1
int     glsdet_conv2d_chain(const glsdet_conv_desc* d, const glsdet_conv_chain* c, void* stream);
int     glsdet_conv2d_chain_tune(const glsdet_conv_desc* d, const glsdet_conv_chain* c, void* stream, int32_t* best_hint,
                                 float* best_us);
/* Bottleneck front in ONE launch (drone/models/base/darknet.py:61-64 `y = self.conv2(self.conv1(x)); if self.use_add:
 * y = y + x`): c1 = the 1x1 (c1->y describes the hidden tensor; its base is not touched), c2 = the 3x3 stride 1 pad 1 on
 * that hidden tensor (c2->x must equal c1->y in extent and dtype), with c2's residual / activation as for glsdet_conv2d.
 * The workgroup of an 8 x 16 output tile recomputes the 1x1 on the tile's halo into LDS; the hidden values are rounded
 * to the storage dtype there, so y equals the two-launch form bit for bit.  Limits: hidden channels 32, 64 or 128 ==
 * c2->y.c; one dtype; y must not overlap x other than as a disjoint channel slice of the same pixel-interleaved buffer
 * (the fused form cannot run in place: GLSDET_E_ARG).  hint 0 / 1: 128- / 64-byte channel chunks.                      */
int     glsdet_bottleneck(const glsdet_conv_desc* c1, const glsdet_conv_desc* c2, int32_t hint, void* stream);
int     glsdet_bottleneck_tune(const glsdet_conv_desc* c1, const glsdet_conv_desc* c2, void* stream, int32_t* best_hint,
                               float* best_us);
/* A whole CSPLayer in ONE launch (drone/models/base/darknet.py:66-112, `x_1 = self.conv1(x); x_2 = self.conv2(x);
 * x_1 = self.m(x_1); x = torch.cat((x_1, x_2), dim=1); return self.conv3(x)` with the Bottleneck of :61-64), ABI 14:
 *     main  = act(bn(conv1(x)))   short = act(bn(conv2(x)))         w12 = ONE packed 1x1 conv 64 -> 64, rows [conv1 | conv2]
 *     h     = act(bn(m.0.conv1(main)))                              wm1: 1x1 32 -> 32
 *     main' = act(bn(m.0.conv2(h))) (+ main when shortcut)          wm2: 3x3 32 -> 32, stride 1, pad 1
 *     y     = act(bn(conv3([main' | short])))                       w3:  1x1 64 -> 64
 * Weights / scale / bias packed as for glsdet_conv2d (cin 64, 32, 32, 64).  A workgroup keeps all 18.4 K weights resident
 * and walks a strip of pixel tiles; main, short, h and main' live in LDS only, each rounded to fp16 exactly where the
 * four-launch form stores it, every product in the k order of the stand-alone kernels: y equals four glsdet_conv2d bit
 * for bit.  Limits: fp16 x and y, x.c == y.c == 64 (hidden 32, ONE Bottleneck), any n / h / w and view strides; y must
 * not overlap x other than as a disjoint channel slice of the same pixel-interleaved buffer.  Anything else is refused
 * with a negative code before any launch (callers fall back to the separate launches).  x AND y are addressed through
 * 32-bit descriptor offsets: the allocation of each (alloc_hi - alloc_lo, not the view) must be below 2^31 - 1 bytes.
 * hint 0 / 1: 8 x 16 / 4 x 16 pixel tiles.                                                                              */
typedef struct glsdet_csp_desc {
  glsdet_view x, y;
  const void*  w12;  const float* scale12; const float* bias12;
  const void*  wm1;  const float* scalem1; const float* biasm1;
  const void*  wm2;  const float* scalem2; const float* biasm2;
  const void*  w3;   const float* scale3;  const float* bias3;
  int32_t act;             /* of all five BaseConvs: GLSDET_ACT_SILU (the only one compiled)      */
  int32_t shortcut;        /* 1: main' += main (Bottleneck.use_add)                             */
} glsdet_csp_desc;
int     glsdet_csp_fused(const glsdet_csp_desc* d, int32_t hint, void* stream);
/* times both tile heights on the device (synchronises; never recorded into a plan); y is written with the result */
int     glsdet_csp_fused_tune(const glsdet_csp_desc* d, void* stream, int32_t* best_hint, float* best_us);
/* Depthwise k x k conv + folded BN + act (`dconv` of DWConv, drone/models/base/baseConv.py:22-30;
 * mmcv DepthwiseSeparableConvModule).  Same descriptor; x.c == y.c; w = [R*S][x.c] elements of
 * x.dtype (tap-major), scale/bias fp32 [x.c]; res must be empty; act: GLSDET_ACT_NONE / SILU / RELU / LRELU (codes 0..3;
 * GELU, SIGMOID and GLSDET_ACT_RES_FIRST are refused with GLSDET_E_ARG before anything is launched). */
int     glsdet_dwconv2d(const glsdet_conv_desc* d, void* stream);
/* the same with a dilation (LSKblock.conv_spatial: 7x7, dilation 3, padding 9, groups = dim; drone/models/lsk/LSK.py:31);
 * y extent = floor((x + 2 pad - dilation (k - 1) - 1) / stride) + 1.                                                  */
int     glsdet_dwconv2d_dilated(const glsdet_conv_desc* d, int32_t dilation, void* stream);
/* Grouped 3x3 conv + folded BN + act: conv2 of the ResNeXt Bottleneck (ufp/mmdet/models/backbones/resnext.py:55-64,
 * `groups` = 32 / 64 groups of Cg = 4 / 8 / 16 / 32 channels).  Same descriptor:
 *     y[n,ho,wo,co] = act( scale[co] * sum_{r,s,j<Cg} x[n, ho*stride-1+r, wo*stride-1+s, (co/Cg)*Cg + j] * weight[co][j][r][s]
 *                          + bias[co] )
 * fp32 accumulation in any order, one rounding to y.dtype; out-of-map taps are zeros.  x.c == y.c == groups * Cg (a
 * multiple of 8), Cg in {4, 8, 16, 32}; R = S = 3, pad = 1, stride 1 or 2; x.dtype == y.dtype (F16 or F32); res empty;
 * tile_hint 0; x and y may be strided views (y a channel slice of a wider buffer) but must not overlap other than as
 * disjoint channel slices of one pixel-interleaved buffer.  Anything else: GLSDET_E_ARG (views: their own codes), nothing
 * launched.
 *  w      : zero-filled block-diagonal tiles over channel blocks of 32, [ceil(C/32)][9][32][32] elements of x.dtype:
 *           w[b][r*3+s][co_l][ci_l] = weight[co][ci - (co/Cg)*Cg][r][s] with co = 32 b + co_l, ci = 32 b + ci_l, where
 *           co < C and ci lies in the group of co; 0 elsewhere.  glsdet_conv_grouped_weight_elems(groups, Cg) elements
 *           (0 for a group width the kernel refuses).
 *  scale/bias : fp32 [ceil(C/32) * 32].
 * On the matrix cores (one K step = one tap of one 32-channel block): 32 / Cg <= 8 times the layer's own multiplies,
 * where the block-diagonal dense conv over all C channels costs C / Cg times.                                          */
int     glsdet_conv2d_grouped(const glsdet_conv_desc* d, int32_t groups, void* stream);
int64_t glsdet_conv_grouped_weight_elems(int32_t groups, int32_t cg);
/* its time on the device (one kernel: *best_hint = 0), for comparisons by the caller's tuner; synchronises, y is written */
int     glsdet_conv2d_grouped_tune(const glsdet_conv_desc* d, int32_t groups, void* stream, int32_t* best_hint, float* best_us);
/* number of ELEMENTS of the packed weight buffer for (cout, R, S, cin, dtype)           */
int64_t glsdet_conv_weight_elems(int32_t cout, int32_t R, int32_t S, int32_t cin, int32_t dtype);
int32_t glsdet_conv_kpad(int32_t R, int32_t S, int32_t cin, int32_t dtype);
int32_t glsdet_conv_cout_pad(int32_t cout);

/* ---------------------------------------------------------------------------------
 * Focus space-to-depth + layout change      drone/models/base/darknet.py:15-21
 * img: NCHW fp32 [n,3,H,W] (contiguous)  ->  y: NHWC view [n,H/2,W/2,16]:
 * channels 0..11 = (TL, BL, TR, BR) x (c0,c1,c2), 12..15 = 0.
 */
int glsdet_focus_pack(const float* img, int32_t n, int32_t cin, int32_t H, int32_t W,
                      const glsdet_view* y, void* stream);

/* Focus AND its 3x3 BaseConv in one launch (drone/models/base/darknet.py:10-21: `self.conv(cat(TL, BL, TR, BR))`): the
 * fp32 NCHW image is read directly, the packed tensor never exists.  w / scale / bias: as glsdet_conv2d for a 3x3 conv
 * over 16 input channels (12 real), packed for y's dtype.  y: NHWC view [n, H/2, W/2, <= 64 channels].                */
int glsdet_focus_conv(const float* img, int32_t n, int32_t cin, int32_t H, int32_t W, const void* w, const float* scale,
                      const float* bias, int32_t act, const glsdet_view* y, void* stream);
/* Focus, its 3x3 BaseConv AND the first downsampling conv (CSPDarknet.stem -> dark2[0], drone/models/base/darknet.py:117-121,
 * 3x3 stride 2) in one launch: the stem's output tensor -- the largest of the network -- is neither written nor read; the
 * workgroup of an output tile computes the stem on the tile's halo into LDS.  w1 / scale1 / bias1: the stem (c1 = 32
 * output channels, packed as for glsdet_focus_conv); w2 / scale2 / bias2: a 3x3 conv over 32 channels; y: NHWC view
 * [n, (H/2 + 1) / 2, (W/2 + 1) / 2, <= 64 channels].  Equals glsdet_focus_conv + glsdet_conv2d(stride 2) bit for bit.     */
int glsdet_focus_conv_down(const float* img, int32_t n, int32_t cin, int32_t H, int32_t W, const void* w1, const float* scale1,
                           const float* bias1, int32_t act1, int32_t c1, const void* w2, const float* scale2,
                           const float* bias2, int32_t act2, const glsdet_view* y, void* stream);

/* max pool k x k, stride 1, pad k/2 (-inf padding)   drone/models/base/darknet.py:29,35 */
int glsdet_maxpool2d(const glsdet_view* x, const glsdet_view* y, int32_t k, void* stream);

/* The three pools of SPPBottleneck (darknet.py:29,35: kernel sizes 5, 9, 13, stride 1, pad k/2) in one launch: x is read once,
 * pool9 = pool5(pool5), pool13 = pool5(pool9) are formed in LDS.  y5 / y9 / y13: x's extent and dtype, one common set of
 * strides (the channel slices of the concat buffer the SPP conv2 reads).                                                */
int glsdet_spp_pools(const glsdet_view* x, const glsdet_view* y5, const glsdet_view* y9, const glsdet_view* y13, void* stream);

/* SpatialAttention front half (drone/models/new/Non_local_family.py:429-432): per pixel the max
 * and the mean over channels.  y: view [n,h,w,8] of x.dtype, channel 0 = max, 1 = mean, 2..7 = 0
 * (the 7x7 2->1 conv + sigmoid that follows is a glsdet_conv2d with GLSDET_ACT_SIGMOID).     */
int glsdet_channel_maxmean(const glsdet_view* x, const glsdet_view* y, void* stream);

/* nearest-neighbour resample by an integer factor (1 = strided copy, 2 = nn.Upsample(2))
 * drone/models/base/yolox.py:103,181,198 ; torch.cat is realised by views, not copies.   */
int glsdet_resample_copy(const glsdet_view* x, const glsdet_view* y, int32_t factor, void* stream);

/* `count` strided copies x[i] -> y[i] (same extents per pair, one dtype and channel count per call) in one launch per 32
 * pairs: the per-(image, quadrant) `.view(b, c, -1)` / `.permute().contiguous()` operand copies of the non-local block
 * (drone/models/new/Non_local_family.py:32-41) when it runs on a ResNet stage, where every product is a GEMM whose
 * second operand must be a dense matrix.                                                                    */
int glsdet_copy_many(const glsdet_view* x, const glsdet_view* y, int32_t count, void* stream);

/* The transposed form: x[i] is ONE image window [1,h,w,C], y[i] a dense matrix view [1,1,rows >= C, cols >= ceil8(h*w)]
 * (row pitch y[i].sw); y[i][c][p] = x[i][p / w][p % w][c].  This is `x.view(b, c, -1)` (Non_local_family.py:33-39) for
 * NHWC storage: the operand of the products that contract over the pixels (X^T X).  Columns beyond the pixels, rows
 * beyond C are left as they are.                                                                            */
int glsdet_transpose_many(const glsdet_view* x, const glsdet_view* y, int32_t count, void* stream);

/* ---------------------------------------------------------------------------------
 * Non-local block, dot-product form       drone/models/block/non_local/Identity_Conv.py:152-173
 *   out = x + Wout * ( (theta^T phi / N) g^T ) + bout      (NO softmax, divide by N)
 * `tpg` holds the three 1x1 projections [theta | phi | g] (each ci channels) of x, produced
 * by glsdet_conv2d with concatenated weights.  Evaluated in the re-associated order
 *   G = sum_j phi_j (x) g_j   [ci x ci],  out_i = x_i + (Wout G^T / N) theta_i + bout
 * which is the same bilinear form at O(N ci^2) instead of O(N^2 ci).
 *  wout : fp32 [cx][ci] row-major, bout: fp32 [cx];
 *  gram : fp32 workspace of n*(8*ci*ci + cx*ci) floats (partial Gram slices + folded matrix).
 */
int glsdet_nonlocal(const glsdet_view* x, const glsdet_view* tpg, int32_t ci,
                    const float* wout, const float* bout, float* gram,
                    const glsdet_view* out, void* stream);
/* 1..4 independent non-local blocks with the same n, channel counts and dtype (the four
 * quadrants of Patch_Conv_NonLocal, Identity_Conv.py:361-364) in one set of three launches.
 * x, tpg, out: arrays of n_sets views; wout, bout: arrays of n_sets device pointers;
 * gram: n_sets times the single-block workspace.                                           */
int glsdet_nonlocal_multi(const glsdet_view* x, const glsdet_view* tpg, int32_t n_sets, int32_t ci,
                          const float* const* wout, const float* const* bout, float* gram,
                          const glsdet_view* out, void* stream);
/* The same 1..4 blocks on the matrix cores (additive exports of ABI 17), for the wide blocks of new/yolox10.py:236-266:
 * Patch_Conv_NonLocal_new on dark3 / dark4 / dark5 with inter_channels = C (Non_local_family.py:32-48), i.e. ci = cx =
 * 128 .. 1280 at the input resolution.  Semantics, association (Gram per pixel slice with the slicing rule of
 * glsdet_nonlocal_multi, a fold that adds the slices in a fixed order, apply), workspace layout and determinism are those
 * of glsdet_nonlocal_multi; no rounding is added (theta / phi / g in the storage type, G, P, wout, bout fp32; the fp16 Gram
 * on v_mfma_f32_32x32x16_f16, everything else on v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain): only the order of the
 * sums differs.  out[q] may equal x[q].  Refused (negative code, nothing launched) unless: n_sets in 1..4; the sets agree
 * in n and channels; ci and x.c multiples of 32, at most 1280; tpg.c >= 3 ci; every base and stride (a window's offset is
 * part of its base), wout[q] and bout[q] multiples of 16 bytes; one dtype (f16 / f32) for x, tpg and out; ws 256-byte
 * aligned with ws_bytes >= glsdet_nonlocal_mfma_workspace_bytes(n, n_sets, ci, x.c) (0 for arguments out of range).  */
int64_t glsdet_nonlocal_mfma_workspace_bytes(int32_t n, int32_t n_sets, int32_t ci, int32_t cx);
int glsdet_nonlocal_mfma(const glsdet_view* x, const glsdet_view* tpg, int32_t n_sets, int32_t ci,
                         const float* const* wout, const float* const* bout, void* ws, int64_t ws_bytes,
                         const glsdet_view* out, void* stream);

/* ---------------------------------------------------------------------------------
 * EVCBlock of the "centralized feature pyramid" (models/cfp/evc_blocks.py:214-308; additive exports of ABI 17).
 *
 * glsdet_lvc_encode: the codebook Encoding layer (models/cfp/Functions.py:25-84, 64 codewords) of every image of x:
 *     A[n][k] = softmax_k( s_k |x_n - c_k|^2 ),   E[b][k][:] = sum_n A[n][k] (x_n - c_k)          n over the h * w pixels
 *   x: NHWC view [n, h, w, C], f16 or f32, converted exactly; codewords fp32 [64][C]; scale fp32 [64]; E fp32 [n][64][C].
 *   Evaluated in the expanded form, everything in fp32, the two products on v_mfma_f32_32x32x2_f32:
 *     D = s_k * (fmaf(-2, x_n . c_k, |x_n|^2) + |c_k|^2),  A = expf(D - max_k D) / sum_k,  E = A^T X - (sum_n A) c.
 *   A never reaches memory.  The pixels of an image are cut into slices of chunk = 128 * max(1, ceil(h w / 8192)) pixels
 *   (a function of h * w only, at most 64 slices); every slice writes its partial A^T X and sum_n A to the workspace and a
 *   second kernel adds the slices in ascending order: no atomics, the same bits on every run.
 *   Refused (negative code, nothing launched) unless: C a multiple of 32 in [32, 640]; base and strides of x (a window's
 *   offset is part of its base), codewords, scale and E multiples of 16 bytes; ws 256-byte aligned with ws_bytes >=
 *   glsdet_lvc_encode_workspace_bytes(n, h, w, C) (0 for arguments out of range); h * w <= 2^24 and n <= 65535 (the grid
 *   is (slices <= 64, n, ceil(C / 64))).
 *
 * glsdet_lvc_gate: LVCBlock.forward from the encoding to the gate (evc_blocks.py:223-238): BatchNorm1d(64) over [n, 64, C]
 *   (per CODE; folded on the host to a_k, b_k), ReLU, the mean over the codes, fc, sigmoid.  fp32, in this order:
 *     m = 0; for k = 0..63: m += fmaxf(fmaf(a_k, E[b][k][c], b_k), 0);   en[c] = m * (1 / 64)
 *     v = fc_b[co]; for c = 0..C-1: v = fmaf(fc_w[co][c], en[c], v);     gam[b][co] = 1 / (1 + expf(-v))    (SIGMOID above)
 *   E fp32 [n][64][C], fc_w fp32 [C][C] row-major, gam fp32 [n][C].  C as for glsdet_lvc_encode; E, fc_w, gam 16-byte aligned.
 *
 * glsdet_channel_fuse: NHWC views of one dtype and extent, 16 bytes per lane, fp32 arithmetic, one rounding; y may alias a.
 *   mode 0: y = relu(fmaf(a, v[img][c], a))     v fp32 [n][C]   (`relu_(x + x * y)`, evc_blocks.py:239; t is not read)
 *   mode 1: y = fmaf(v[c], t, a)                v fp32 [C]      (`x + layer_scale_1 * dw(norm1(x))`, evc_blocks.py:272)      */
int64_t glsdet_lvc_encode_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t C);
int glsdet_lvc_encode(const glsdet_view* x, const float* codewords, const float* scale, void* ws, int64_t ws_bytes,
                      float* E, void* stream);
int glsdet_lvc_gate(const float* E, int32_t n, int32_t C, const float* a_k, const float* b_k, const float* fc_w,
                    const float* fc_b, float* gam, void* stream);
int glsdet_channel_fuse(const glsdet_view* a, const glsdet_view* t, const glsdet_view* y, const float* v, int32_t mode,
                        void* stream);

/* ---------------------------------------------------------------------------------
 * Patch_Conv_NonLocal_adapt_new: the data-dependent quadrant split (drone/models/new/Non_local_family.py:272-357)
 * The reference thresholds its SpatialAttention map (values under min + 0.75 (max - min) -> 0) and walks columns / rows in
 * Python until the running sum passes half of the total (`get_centroid`, :298-321: one device sync per step).  Here:
 *   glsdet_attn_split   att = [n,h,w,>=1] view whose channel 0 is the map (n <= 16, one split for the whole batch as in the
 *                       reference) -> split = DEVICE int32[4] {row split, column split above it, column split from it on, 0}
 *   glsdet_nonlocal_split  the four Non_local_Blocks (sets lt, lb, rt, rb) on the windows `split` describes: x / out full
 *                       maps, tpg[q] = [theta|phi|g] of the full map with quadrant q's weights, gram = 4 x the workspace of
 *                       glsdet_nonlocal
 *   glsdet_rowsplit     mode 0 / 1: y = a above / from the row split, zero elsewhere (the zero padding the top / bottom 3x3
 *                       convs see at the split); mode 2: y = row < split ? a : b (`torch.cat((t, b), dim=2)`);
 *                       mode 3 | q << 4: y = a inside quadrant q (0 lt, 1 lb, 2 rt, 3 rb), zero outside; mode 4 | q << 4: y = a
 *                       inside quadrant q, y untouched outside; | 1 << 8: the split indices halved (regions of the stride-2
 *                       map of Patch_Conv_NonLocal_adapt, :112-206, whose quadrant convs have stride 2)
 *   glsdet_scale_by_map y[..,c] = map[..,0] * x[..,c]                                  (:355-356)
 * Nothing returns to the host: the block is recordable / capturable like any other op sequence.                       */
int glsdet_attn_split(const glsdet_view* att, int32_t* split, void* stream);
int glsdet_nonlocal_split(const glsdet_view* x, const glsdet_view* tpg /*[4]*/, int32_t ci, const float* const* wout /*[4]*/,
                          const float* const* bout /*[4]*/, float* gram, const glsdet_view* out, const int32_t* split,
                          int32_t split_shift /* 0, or 1: windows on the stride-2 map */, void* stream);
int glsdet_rowsplit(const glsdet_view* a, const glsdet_view* b /*mode 2*/, const glsdet_view* y, const int32_t* split, int32_t mode,
                    void* stream);
int glsdet_scale_by_map(const glsdet_view* x, const glsdet_view* map, const glsdet_view* y, void* stream);

/* ---------------------------------------------------------------------------------
 * YOLOX decode        drone/models/core/utils_bbox.py:254-306  (mode 0, normalised cxcywh)
 *                     ufp/mmdet/models/dense_heads/yolox_head.py:298-308 (mode 1, xyxy px)
 * levels: fp32 views [n,H_l,W_l,>=5+nc] (channel order reg4, obj, cls..).
 * out: fp32 [n][A][5+nc] contiguous, A = sum H_l*W_l, level-major then row-major.
 * mode 0: sigmoid(obj,cls); cx=(x+gx)*s/in_w, cy=(y+gy)*s/in_h, w=exp()*s/in_w, h=exp()*s/in_h,
 *         s = in_h / H_l for both axes (reference quirk, utils_bbox.py:285).
 * mode 1: sigmoid(obj,cls); x1,y1,x2,y2 in input pixels, s_l = strides[l]; if scale_factors
 *         (device fp32 [n][4], may be NULL) is given the box is divided by it per image
 *         (mmdet `rescale=True`, yolox_head.py:283-285).
 * glsdet_yolox_decode_ex (ABI 15): the same with a choice of the score channels that go through the sigmoid --
 *   sigmoid_mask bit 0 = objectness (channel 4), bit 1 = the classes (channels 5 .. 5+nc); a channel outside the mask
 *   is copied through as the raw fp32 logit, bit for bit; 3 = glsdet_yolox_decode; outside 0..3: GLSDET_E_ARG.  The
 *   box arithmetic does not depend on the mask.  The decode variants of drone/models/core/utils_bbox.py:36-253 that
 *   the harness picks by `decode_mode` (drone/yolo.py:75-82):
 *     decode_outputs_cls_sigmoid     mode 0, mask 2        decode_outputs_no_sigmoid   mode 0, mask 1
 *     decode_outputs_no_sigmoid_all  mode 0, mask 0        decode_outputs_xyxy         mode 1, mask 0, strides = NULL,
 *                                                                                      scale_factors = NULL
 */
int glsdet_yolox_decode(const glsdet_view* levels, int32_t n_levels, int32_t num_classes,
                        int32_t in_h, int32_t in_w, const int32_t* strides /*host, may be NULL*/,
                        int32_t mode, float* out, int64_t out_elems,
                        const float* scale_factors, void* stream);
int glsdet_yolox_decode_ex(const glsdet_view* levels, int32_t n_levels, int32_t num_classes,
                           int32_t in_h, int32_t in_w, const int32_t* strides /*host, may be NULL*/,
                           int32_t mode, int32_t sigmoid_mask, float* out, int64_t out_elems,
                           const float* scale_factors, void* stream);

/* ---------------------------------------------------------------------------------
 * class-max + score threshold + batched (per-class) NMS
 *   drone/models/core/utils_bbox.py:375-419  (torchvision.ops.boxes.batched_nms)
 *   ufp/mmdet/models/dense_heads/yolox_head.py:310-322 (mmcv.ops.batched_nms)
 * pred: fp32 [n][A][5+nc] as produced by glsdet_yolox_decode (either mode; mode 0 boxes
 *       are converted cxcywh->xyxy first, utils_bbox.py:380-385).
 * keep score = obj * max_c cls_c >= conf_thres; candidates visited by descending score
 * (ties: lower anchor index first); a candidate is dropped if an already kept one of the
 * SAME class has IoU > nms_thres (areas without +1).
 * dets : fp32 [n][max_det][7] = x1,y1,x2,y2,obj,cls_conf,cls_id in score order
 * count: int32 [2n]: [0,n) kept per image clamped to max_det, [n,2n) unclamped
 * ws   : workspace of glsdet_nms_workspace_bytes(n, A, max_cand) bytes
 * status: int32[1], bit0 set if some image had more than max_cand candidates (results for
 *         that image are then NOT the reference's: callers must treat it as an error).
 */
int64_t glsdet_nms_workspace_bytes(int32_t n, int32_t A, int32_t max_cand);
int glsdet_nms(const float* pred, int32_t n, int32_t A, int32_t num_classes, int32_t box_mode,
               float conf_thres, float nms_thres, int32_t max_cand, int32_t max_det,
               float* dets, int32_t* count, int32_t* status,
               void* ws, int64_t ws_bytes, void* stream);

/* The exchange record of the multi-GPU path: replaces the pickled result list that
 * collect_results_gpu pads and all_gathers (ufp/mmdet/apis/test.py:161-191).
 *   dets [n][max_det][7], count int32 [2n] as glsdet_nms / glsdet_gfl_detect leave them
 *   out  fp32 [n][cap+1][7]: rows 0..cap-1 = the first min(count, cap) detections in score order (zero rows
 *        behind them), row cap = (rows kept here, detections before any cap, 0, 0, 0, 0, 0).
 * One launch, recordable / capturable like every other op: the record is complete when the plan is.  */
int glsdet_pack_detections(const float* dets, const int32_t* count, int32_t n, int32_t max_det, int32_t cap,
                           float* out, void* stream);

/* ---------------------------------------------------------------------------------
 * ResNet-50 / FPN / GFL / MPHead helpers
 * --------------------------------------------------------------------------------- */
/* fp32 NCHW image -> NHWC view of the engine dtype, channels zero padded to y.c (>= cin,
 * multiple of 8): the input of the 7x7 s2 stem conv (ufp/mmdet/models/backbones/resnet.py:634). */
int glsdet_nchw_pack(const float* img, int32_t n, int32_t cin, int32_t H, int32_t W,
                     const glsdet_view* y, void* stream);

/* ResNet stem in one launch: y = act(scale * conv7x7 stride 2 pad 3 (img) + bias) straight from the fp32 NCHW image
 * (ufp/mmdet/models/backbones/resnet.py:634-636 `x = self.relu(self.norm1(self.conv1(x)))`), replacing glsdet_nchw_pack +
 * glsdet_conv2d over 3 channels padded to 8.  w: [64][7][8][4] elements of y's dtype = conv1.weight[co][c][r][s] at
 * [co][r][s][c], zero for s = 7 and c = 3 (glsdet_resnet_stem_weight_elems elements); scale / bias: folded BN, fp32 [64];
 * y: NHWC view [n, (H + 1) / 2, (W + 1) / 2, 64].  Same k order as the generic kernel minus its zero-padded channels:
 * results agree to fp32 summation-order noise.                                                                          */
int64_t glsdet_resnet_stem_weight_elems(void);
/* ... and with `x = self.maxpool(x)` (resnet.py:637: MaxPool2d(3, stride 2, padding 1)) in the epilogue: the stem's output
 * is never written; act is ReLU (a zero stands in for the pool's -inf padding).  y: [n, ((H+1)/2 + 1) / 2, ((W+1)/2 + 1) / 2, 64].
 * Equals glsdet_resnet_stem + glsdet_pool2d bit for bit.                                                                */
int glsdet_resnet_stem_pool(const float* img, int32_t n, int32_t cin, int32_t H, int32_t W, const void* w, const float* scale,
                            const float* bias, const glsdet_view* y, void* stream);
int glsdet_resnet_stem(const float* img, int32_t n, int32_t cin, int32_t H, int32_t W, const void* w, const float* scale,
                       const float* bias, int32_t act, const glsdet_view* y, void* stream);

/* nn.MaxPool2d(k, stride, pad) (resnet.py:598: k3 s2 p1), floor mode, -inf padding.
 * y extent must be floor((x + 2*pad - k)/stride) + 1.                                      */
int glsdet_pool2d(const glsdet_view* x, const glsdet_view* y, int32_t k, int32_t stride, int32_t pad,
                  void* stream);

/* FPN top-down step (ufp/mmdet/models/necks/fpn.py:165-175):
 *   fine += F.interpolate(coarse, size=fine.shape[2:], mode='nearest')
 * source index = min(floor(dst * (float)in/out), in-1) as torch computes it.  In place on fine. */
int glsdet_upsample_add(const glsdet_view* coarse, const glsdet_view* fine, void* stream);

/* nn.GroupNorm(groups, C) (+ optional ReLU) on an NHWC view, two kernels: fp64 partial sums
 * per (image, pixel slice, group) into `stats` (caller owned, glsdet_groupnorm_workspace_bytes
 * bytes, 8-byte aligned), then the fold + affine normalisation.  The conv towers of GFLHead /
 * MPHead: mmcv ConvModule(norm_cfg=GN32) = conv -> GN -> ReLU (gfl_head.py:128-152).
 * y may alias x.  gamma, beta: fp32 [C].  act: GLSDET_ACT_NONE or GLSDET_ACT_RELU.          */
int64_t glsdet_groupnorm_workspace_bytes(int32_t n, int32_t groups);
int glsdet_groupnorm(const glsdet_view* x, const glsdet_view* y, int32_t groups, const float* gamma,
                     const float* beta, float eps, int32_t act, void* stats, void* stream);
/* 1..16 tensors of the same n / C / groups in one launch pair (cls and reg tower outputs of all
 * pyramid levels); stats = n_sets times the single-tensor workspace. */
int glsdet_groupnorm_multi(const glsdet_view* x, const glsdet_view* y, int32_t n_sets, int32_t groups,
                           const float* const* gamma, const float* const* beta, float eps, int32_t act,
                           void* stats, void* stream);

/* The same, with the statistics of some sets already produced by the conv that wrote them: pre_stats[q] != NULL names
 * the partials glsdet_conv2d_gnstats wrote for x[q] (one slice per 8 x 16 pixel tile); those sets skip the statistics
 * pass (one read of the tensor less).  pre_stats == NULL or all NULL: glsdet_groupnorm_multi.                          */
int glsdet_groupnorm_multi_pre(const glsdet_view* x, const glsdet_view* y, int32_t n_sets, int32_t groups,
                               const float* const* gamma, const float* const* beta, float eps, int32_t act,
                               void* stats, void* const* pre_stats, void* stream);
/* glsdet_conv2d that ALSO writes the GroupNorm partial sums of the tensor it stores (gfl_head.py:128-152: every tower
 * conv is followed by GN(32) + ReLU): per (image, 8 x 16 pixel tile, group) the fp64 sum and sum of squares of the
 * stored values, summed in a fixed order.  3x3 stride 1, no residual, x.dtype == y.dtype, halo ring kernels only
 * (tile_hint 8..11, 0 = 8); anything else is GLSDET_E_ARG and the caller runs glsdet_conv2d + the two-pass GN.
 * stats: glsdet_conv2d_gnstats_bytes(n, ho, wo, groups) bytes, 8-byte aligned.                                         */
int64_t glsdet_conv2d_gnstats_bytes(int32_t n, int32_t ho, int32_t wo, int32_t groups);
int     glsdet_conv2d_gnstats(const glsdet_conv_desc* d, int32_t groups, void* stats, void* stream);
int     glsdet_conv2d_gnstats_tune(const glsdet_conv_desc* d, int32_t groups, void* stats, void* stream, int32_t* best_hint,
                                   float* best_us);

/* The two elementwise steps of LSKblock.forward (drone/models/lsk/LSK.py:46-48) on NHWC views of one dtype:
 *   mode 0: y[.., c] = a[.., c] * map[.., 0] + b[.., c] * map[.., 1]     (`attn1 * sig[:, 0] + attn2 * sig[:, 1]`)
 *   mode 1: y = a * b                                                     (`x * attn`; map may be NULL)
 * fp32 arithmetic, one rounding.  y may alias a or b.                                                                 */
int glsdet_gate(const glsdet_view* a, const glsdet_view* b, const glsdet_view* map, const glsdet_view* y, int32_t mode,
                void* stream);

/* MPHead.forward_proxy (ufp/mmdet/models/dense_heads/mp_head.py:105-121).
 *   feat : view [n,h,w,C] (the gfl_cls_conv output), engine dtype
 *   dots : fp32 view [n,h,w,>=P], feat . (proxy_k / max(|proxy_k|, 1e-12)) for the P proxies
 *          (a glsdet_conv2d with the normalised proxies as a 1x1 weight)
 *   counts: host int32 [nc], proxies per class (sum = P <= 64 per class and P <= 256 in all)
 *   out  : fp32 view [n,h,w,>=nc]:  gamma * sum_k softmax_k(gamma*s_k) * s_k  per class,
 *          s_k = dots_k / max(|feat|, 1e-12)                                              */
int glsdet_proxy_scores(const glsdet_view* feat, const glsdet_view* dots, const int32_t* counts,
                        int32_t num_classes, float gamma, const glsdet_view* out, void* stream);

/* GFL post-processing: gfl_head.py:380-471 (_get_bboxes_single) + base_dense_head.py:226-301
 * (_bbox_post_process) + core/utils/misc.py:119-165 (filter_scores_and_topk).
 *   cls : fp32 views [n,H_l,W_l,>=nc] raw class logits;  reg: fp32 views [n,H_l,W_l,>=4*(reg_max+1)]
 *   per level: score = sigmoid(cls) ; (position, class) pairs with score > score_thr ; the
 *   nms_pre best (ties: lower position*nc+class first) ; distances = Integral(reg) * stride ;
 *   box = (x*s - l, y*s - t, x*s + r, y*s + b) clamped to [0,img_w] x [0,img_h]
 *   (img_hw: device fp32 [n][2] = h,w per image, NULL = in_h,in_w) ; levels concatenated ;
 *   divided by scale_factors (device fp32 [n][4], may be NULL) ; per-class NMS (IoU > iou_thr
 *   suppresses) ; the first max_det in descending score order.
 *   dets : fp32 [n][max_det][7] = x1,y1,x2,y2,score,score,label ; count: int32 [2n] as glsdet_nms
 *   status bit0: a level held more than max_cand passing pairs (results invalid for that image)
 *   ws   : glsdet_gfl_workspace_bytes(n, n_levels, max_cand, nms_pre) bytes, 256-byte aligned   */
int64_t glsdet_gfl_workspace_bytes(int32_t n, int32_t n_levels, int32_t max_cand, int32_t nms_pre);
int glsdet_gfl_detect(const glsdet_view* cls, const glsdet_view* reg, int32_t n_levels,
                      const int32_t* strides /*host*/, int32_t num_classes, int32_t reg_max,
                      int32_t in_h, int32_t in_w, const float* img_hw, const float* scale_factors,
                      float score_thr, int32_t nms_pre, float iou_thr, int32_t max_cand, int32_t max_det,
                      float* dets, int32_t* count, int32_t* status,
                      void* ws, int64_t ws_bytes, void* stream);
/* ABI 16: the reference's get_bboxes(..., rescale=False, with_nms=False) -- glsdet_gfl_detect up to and including the
 * level concatenation, without the division by the scale factors and without the NMS.
 *   cand       : fp32 [n][cap][8] = x1,y1,x2,y2,score,label,0,0, 16-byte aligned.  Rows are level-major and inside a level
 *                by descending score, ties by lower position*nc+class first: the order of torch.cat(mlvl_*).  Rows at and
 *                beyond the count are not written.
 *   cap        : >= sum over levels of min(nms_pre, H_l*W_l*nc)
 *   cand_count : int32 [n];  status bit0 as in glsdet_gfl_detect
 *   ws         : glsdet_gfl_candidates_workspace_bytes(n, n_levels, max_cand) bytes, 256-byte aligned                      */
int64_t glsdet_gfl_candidates_workspace_bytes(int32_t n, int32_t n_levels, int32_t max_cand);
int glsdet_gfl_candidates(const glsdet_view* cls, const glsdet_view* reg, int32_t n_levels,
                          const int32_t* strides /*host*/, int32_t num_classes, int32_t reg_max,
                          int32_t in_h, int32_t in_w, const float* img_hw, float score_thr, int32_t nms_pre,
                          int32_t max_cand, float* cand, int32_t cap, int32_t* cand_count, int32_t* status,
                          void* ws, int64_t ws_bytes, void* stream);

/* ABI 16: test-time augmentation, the cross-augmentation step of BBoxTestMixin.aug_test_bboxes
 * (dense_heads/dense_test_mixins.py:41-114): merge_aug_bboxes (:179-206) with bbox_mapping_back
 * (core/bbox/transforms.py:22-72), one per-class NMS over the union, the first max_det.
 *   cands / cand_counts / caps : host arrays of n_augs entries (1 <= n_augs <= GLSDET_MAX_AUGS), read when the call is made
 *                (or recorded) and carried in the kernel arguments: device rows [n][cap_k][8] as glsdet_gfl_candidates
 *                writes them, device int32 counts [n], capacities.  The capacities may sum to 32768 at the most.
 *   aug_meta : device fp32 [n_augs][n][8] = img_h, img_w, sf0, sf1, sf2, sf3, flip code (0 none, 1 horizontal, 2 vertical,
 *              3 diagonal), 0.  Horizontal: x1' = img_w - x2, x2' = img_w - x1; vertical likewise with img_h; then every
 *              coordinate is divided by its scale factor -- one fp32 operation each.
 *   The lists are concatenated in augmentation order; greedy per-class NMS in (score descending, concatenation index
 *   ascending) order, IoU > iou_thr suppresses, areas without +1; the first max_det; the four coordinates are then
 *   multiplied by out_scale (device fp32 [n][4]) unless it is NULL (`rescale=False`, dense_test_mixins.py:108-110).
 *   dets / count / status as glsdet_gfl_detect;  ws: glsdet_aug_merge_workspace_bytes(n, caps, n_augs), 256-byte aligned.  */
#define GLSDET_MAX_AUGS 12
int64_t glsdet_aug_merge_workspace_bytes(int32_t n, const int32_t* caps /*host*/, int32_t n_augs);
int glsdet_aug_merge_nms(const float* const* cands /*host*/, const int32_t* const* cand_counts /*host*/,
                         const int32_t* caps /*host*/, int32_t n_augs, int32_t n, const float* aug_meta, float iou_thr,
                         int32_t max_det, const float* out_scale, float* dets, int32_t* count, int32_t* status,
                         void* ws, int64_t ws_bytes, void* stream);

/* ABI 17: Soft-NMS of merged result rows, drone/merge_results.py:41-130 (py_cpu_softnms, batched_soft_nms) with the call
 * of :159-163 taken (the reference ships with that call commented out and batched_nms live).
 *   cand / cand_count : the candidate rows of glsdet_gfl_candidates: fp32 [n][cap][8] = x1,y1,x2,y2,score,label,(2 columns
 *              that are not read), 16-byte aligned, and int32 [n] counts on the device; a count is clamped to [0, cap]
 *              before any loop uses it.  cap <= 32768.  Scores must be finite and >= 0, boxes x2 >= x1 and y2 >= y1,
 *              labels integer-valued.
 *   Per image and per class present, the class's rows in ascending original index form a segment of N positions
 *   (box, score, original index), and for i = 0 .. N-1:
 *     selection : if i != N-1, m = the FIRST position of the maximum of score[i+1:]; if score[i] < score[m] (strict: a tie
 *                 leaves the order alone) positions i and m are SWAPPED (box, score, index -- a swap, not a rotation).
 *     overlap   : for every k > i, in fp64 on the fp32 coordinates, every operation rounded on its own:
 *                 w = max(0, min(x2) - max(x1) + 1), h alike, inter = w * h, ovr = inter / (area_i + area_k - inter),
 *                 area = (x2 - x1 + 1) * (y2 - y1 + 1).
 *     weight    : method 1 (linear)   1 - ovr if ovr > iou_thr, else 1
 *                 method 2 (gaussian) exp(-(ovr * ovr) / sigma), fp64
 *                 method 3 (hard)     0 if ovr > iou_thr, else 1
 *     update    : score[k] = fp32(weight * fp64(score[k])), one rounding to fp32 per update.
 *   A row survives when its decayed score > min_score (strict, compared in fp32).  The reference's values are
 *   iou_thr (Nt) 0.3, sigma 0.5, min_score (thresh) 1e-4, method 2.  iou_thr and sigma are doubles because the
 *   reference compares and divides in fp64.  The loop stops once the largest remaining score is <= min_score: weights lie
 *   in [0, 1] and scores are >= 0, so nothing behind that point can survive.
 *   The survivors of an image are sorted by ORIGINAL score descending (batched_soft_nms: the decay works on a copy), with
 *   rescore != 0 by decayed score descending; ties go to the lower original index (the reference's torch.sort leaves them
 *   unspecified).  The first max_det are written.
 *   dets   : fp32 [n][max_det][7] = x1,y1,x2,y2, original score, decayed score, label; rows at and beyond the count are
 *            not written.   count: int32 [2n], survivors clamped to max_det, then unclamped.
 *   status : int32 [1]; bit0: a count exceeds cap; bit1: a class segment is longer than
 *            glsdet_soft_nms_segment_limit() or a label lies outside [0, num_classes).  With either bit set the results
 *            are invalid (every loop stays clamped; rows of an over-long segment or with a bad label are dropped).
 *   glsdet_soft_nms_segment_limit() = 6784: a segment stays in LDS as fp32 box (16 bytes) + fp32 score + int32 index
 *            = 24 bytes per row behind 1024 bytes of reduction slots; (160 KiB - 1 KiB) / 24 = 6784.
 *   ws     : glsdet_soft_nms_workspace_bytes(n, cap) bytes, 256-byte aligned (0 for n < 1 or cap outside 1 .. 32768).
 *   Refused on the host: n < 1, cap > 32768, method outside 1..3, sigma <= 0 with method 2, min_score negative or not
 *   finite (dropped rows carry a decayed score of 0, which must not pass), misaligned buffers, a short workspace.                                                                                                           */
int64_t glsdet_soft_nms_workspace_bytes(int32_t n, int32_t cap);
int32_t glsdet_soft_nms_segment_limit(void);
int glsdet_soft_nms(const float* cand, const int32_t* cand_count, int32_t n, int32_t cap, int32_t num_classes,
                    int32_t method, double iou_thr, double sigma, float min_score, int32_t rescore, int32_t max_det,
                    float* dets, int32_t* count, int32_t* status, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Image preprocessing, drone flavour:
 *   PIL `image.resize(size, Image.BICUBIC)` + `preprocess_input` + HWC->CHW
 *   (drone/models/core/utils.py:21-34,46-50; yolo.py:130-134), bit-identical to Pillow:
 *   two passes with uint8 intermediate and 22-bit fixed-point coefficients.
 * src : device uint8 [in_h][in_w][3] (RGB);  tmp: device uint8 [in_h][out_w][3] scratch
 * x/y bounds: device int32 [out][2] = (first source index, tap count); x/y kk: device int32
 *   [out][ksize] coefficients * 2^22 as Pillow's precompute_coeffs + normalize_coeffs_8bpc give
 *   them (glsdet_amd/preprocess.py computes the tables on the host)
 * dst : device fp32 image [3][dst_h][dst_w] (one image of an NCHW batch); the resized picture
 *   lands at (off_y, off_x) (letterbox paste), the rest of the canvas is the caller's.
 * mean3 / std3: host double[3]; value = f32(f64(f32(v/255f)) - mean) then f32(f64(.) / std), the
 *   mixed float32/float64 in-place arithmetic numpy performs in preprocess_input.          */
int glsdet_pil_resize_normalize(const unsigned char* src, int32_t in_h, int32_t in_w,
                                const int32_t* xbounds, const int32_t* xkk, int32_t xksize, int32_t out_w,
                                const int32_t* ybounds, const int32_t* ykk, int32_t yksize, int32_t out_h,
                                unsigned char* tmp, float* dst, int32_t dst_h, int32_t dst_w,
                                int32_t off_y, int32_t off_x, const double* mean3, const double* std3,
                                void* stream);

/* ---------------------------------------------------------------------------------
 * UFPMP-Det second stage (ufp/ufpmp_det_eval.py)
 * --------------------------------------------------------------------------------- */
/* display_merge_result (:182-193): chips = device fp32 [n_chips][7] = src_x, src_y, w, h, canvas_x,
 * canvas_y, magnification (floored like the reference); img: device uint8 [H][W][3] (BGR as cv2 reads
 * it); canvas: device fp32 [ch][cw][3], zero outside the chips.  Crops are magnified with cv2.resize's
 * uint8 INTER_LINEAR arithmetic (11-bit fixed point), restated -- cv2 is not available to pin it. */
int glsdet_ufp_mosaic(const unsigned char* img, int32_t H, int32_t W, const float* chips, int32_t n_chips,
                      float* canvas, int32_t ch, int32_t cw, void* stream);
/* mmdet test pipeline on an fp32 HWC BGR image: bilinear resize to nh x nw (half-pixel centres, edge
 * clamp), BGR->RGB, (v - mean) * (1/std), zero padding to ph x pw, HWC->CHW
 * (mmdet/datasets/pipelines/transforms.py:30,671,572).  mean/std: host double[3], RGB order.      */
int glsdet_resize_normalize_pad(const float* src, int32_t h, int32_t w, int32_t nh, int32_t nw, float* dst,
                                int32_t ph, int32_t pw, const double* mean_rgb, const double* std_rgb, void* stream);
/* the same on a uint8 HWC BGR frame (the first stage: cv2.imread -> mmcv.imresize): cv2.resize's uint8
 * INTER_LINEAR (11-bit fixed point, rounded to uint8) before Normalize.  An exact 2x downscale, which
 * OpenCV silently turns into INTER_AREA, is NOT special-cased. */
int glsdet_resize_normalize_pad_u8(const unsigned char* src, int32_t h, int32_t w, int32_t nh, int32_t nw, float* dst,
                                   int32_t ph, int32_t pw, const double* mean_rgb, const double* std_rgb,
                                   void* stream);
/* ABI 16: the two calls above followed by mmcv.imflip of the resized nh x nw picture (RandomFlip runs between Resize and
 * Normalize / Pad, transforms.py:457-461).  flip: 0 none (= the calls above), 1 horizontal, 2 vertical, 3 diagonal.
 * Destination pixel (y, x) inside nh x nw holds what the unflipped call writes at (nh-1-y if vertical, nw-1-x if
 * horizontal); the zero padding stays at the right and the bottom.                                                       */
int glsdet_resize_normalize_pad_ex(const float* src, int32_t h, int32_t w, int32_t nh, int32_t nw, float* dst,
                                   int32_t ph, int32_t pw, const double* mean_rgb, const double* std_rgb, int32_t flip,
                                   void* stream);
int glsdet_resize_normalize_pad_u8_ex(const unsigned char* src, int32_t h, int32_t w, int32_t nh, int32_t nw, float* dst,
                                      int32_t ph, int32_t pw, const double* mean_rgb, const double* std_rgb, int32_t flip,
                                      void* stream);
/* back-mapping + merge NMS (:282-300): dets = the fine detector's rows [max_det][7] (x1,y1,x2,y2,
 * score,score,label) with their count on the device; a row inside a chip's mosaic rectangle (IoF >
 * iof_thr) is mapped to source-image coordinates; per class greedy NMS with '+1' areas, a box
 * survives while IoU <= nms_thr (py_cpu_nms :149-178).  out: [max_out][7] in descending score
 * order, out_count int32[2] (kept clamped / unclamped), status bit0 = more than max_cand matches. */
int64_t glsdet_ufp_merge_workspace_bytes(int32_t max_cand);
int glsdet_ufp_backmap_merge(const float* dets, const int32_t* count, int32_t max_det, const float* chips,
                             int32_t n_chips, float iof_thr, float nms_thr, int32_t max_cand, int32_t max_out,
                             float* out, int32_t* out_count, int32_t* status, void* ws, int64_t ws_bytes,
                             void* stream);

/* Unified foreground packing on the device (an additive export of ABI 17): ufp/UFPMP-Det-Tools/ufp/unified_foreground_packing.py:6-197
 * (scale_boxes :6-32, ForegroundRegionGeneration :54-87, Packing :125-164) and spp.py:77-168 (phsppog sorted by height,
 * recursive_packing) on the coarse detector's own buffers, so that only `header` crosses the bus between the two stages.
 * One wave per image; no host synchronisation and no allocation inside the call: legal under stream capture.
 *   dets / count : fp32 [n_img][max_det][7] rows x1,y1,x2,y2,score,score,label in the detector's NMS order and int32
 *                  [n_img] (glsdet_gfl_detect's buffers).  Rows at and beyond the count are not read.
 *   The result is that of UnifiedForegroundPacking(boxes_class_major_float32, expand, [img_w, img_h]) under numpy 2
 *   (NEP 50), where a float32 input makes the computation mixed precision:
 *     order     : class-major, stable (np.argsort(labels, kind="stable")); within a class the detector's order.
 *     enlarge   : float32, each operation rounded once: half_w = ((x2-x1)*0.5f)*expand (expand rounded to float32 first),
 *                 cx = (x2+x1)*0.5f, clip of cx -/+ half_w to [0, img_w-1] (ties give the bound), y alike.  The object
 *                 area (x2-x1+1)*(y2-y1+1) is float32 and is accumulated in float32.
 *     merge     : float32.  For i ascending, if alive, for j ascending over every alive j != i (earlier j included): the
 *                 union box by min / max; merge iff (ux1-ux0)*(uy1-uy0) < (r2-r0)*(r3-r1) + (o2-o0)*(o3-o1), each product and
 *                 the sum rounded on their own (no fused multiply-add).  The region grows as soon as a j merges: later j see
 *                 the grown region, earlier j are not revisited.
 *     magnify   : (double)area_sum / (double)count, an IEEE float64 division; < 1024 -> 4, < 9216 -> 2, else 1.
 *     sizes     : (double)(float)(r2-r0) * magnification; from here on everything is float64 (strip width, width - w,
 *                 top + h, x + rw and the equality tests).
 *     strip     : rectangles by decreasing height, stable.  The first unplaced one opens a shelf at (0, top) and leaves the
 *                 slot (w, top, width - w, h); a slot takes the FIRST rectangle of the lowest class among 1 exact fit,
 *                 2 exact width, 3 exact height, 4 strictly smaller both ways, else it dies.  Class 2 leaves the slot above,
 *                 class 3 the slot to the right; class 4 compares with `smallest`, the least side of the rectangles still
 *                 unplaced AFTER the pick (infinity when none): w-rw < smallest: above (full width); h-rh < smallest: right
 *                 (full height); rw < smallest: right (height rh), then above (full width); else above (width rw), then right
 *                 (full height).  The first slot is filled completely before the second.
 *     bisection : lo = 300, hi = 2666, mid = (lo+hi)/2, lo = mid+1 when the packed height > mid else hi = mid-1, while
 *                 lo <= hi: 11 probes.  The layout of the LAST probe is used, feasible or not.
 *     claim     : placed rectangles in region order; each claims every still-pending region of exactly equal magnified
 *                 size, in ascending region order, at its own position (equal-sized regions share one position).
 *   chips       : fp64 [n_img][max_det][7] = src_x, src_y, w, h, canvas_x, canvas_y, magnification, in claim order; rows at
 *                 and beyond n_chips are not written.
 *   chips_floor : fp32, (float)floor(chips): what glsdet_ufp_mosaic / glsdet_ufp_backmap_merge take.
 *   header      : fp64 [n_img][4] = n_boxes, n_chips, canvas_w, canvas_h (max of x+w / y+h over the placed rectangles).
 *   status      : int32 [n_img], written for every image; bit0 = count outside [0, max_det]: then the header row is
 *                 count, 0, 0, 0 (n_boxes holds the count as it was read) and no chip is written.
 *   glsdet_ufp_pack_max_boxes() = (160 KiB - 32) / 104 = 1575: per box the LDS holds the region (16 bytes), four doubles
 *                 (size and position, 32), a stack slot (32, plus one slot of 32 bytes per image), area sum and count (8)
 *                 and four int32 maps and flags (16).
 *   Refused on the host: null or misaligned pointers (4 bytes; chips / header 8), n_img < 1, max_det outside
 *   1 .. glsdet_ufp_pack_max_boxes(), expand not finite or <= 0, img_w < 1 or img_h < 1.                                   */
int32_t glsdet_ufp_pack_max_boxes(void);
int glsdet_ufp_pack(const float* dets, const int32_t* count, int32_t n_img, int32_t max_det, float expand,
                    int32_t img_w, int32_t img_h, double* chips, float* chips_floor, double* header, int32_t* status,
                    void* stream);

/* ---------------------------------------------------------------------------------
 * bbox COCOeval: COCOeval.computeIoU + evaluateImg
 * (drone/models/core/cocoeval.py:163-190, 235-313; the protocol ufp/ufpmp_det_eval.py:333-338 runs
 * through pycocotools) for n_pairs (image, category) pairs in one call, all in fp64.
 *   dt_box [n_dt][4] x,y,w,h / dt_area [n_dt]: the pair's detections contiguous, in descending
 *       score order (stable), cut to the largest maxDets; dt_off int32 [n_pairs+1]
 *   gt_box [n_gt][4] / gt_area [n_gt] / gt_flags u8 [n_gt] (bit0 iscrowd, bit1 ignore, bit2 the
 *       annotation id is 0 -- the reference tests `dtm == 0` on stored ids); gt_off [n_pairs+1]
 *   iou_off int64 [n_pairs+1]: start of the pair's [D][G] block in `ious` (cumulative D*G)
 *   area_rng fp64 [n_area][2]; iou_thr fp64 [n_thr]
 * out (device, caller allocated; nothing needs clearing):
 *   ious       fp64 [iou_off[n_pairs]]   IoU, ground truths in annotation order (computeIoU)
 *   gt_order   int32 [n_area][n_gt]      position -> index inside the pair, ignored last (stable)
 *   gt_ignore  u8    [n_area][n_gt]      gtIgnore by position
 *   n_regular  int32 [n_area][n_pairs]   ground truths not ignored
 *   dt_match   int32 [n_area][n_thr][n_dt]  index inside the pair of the matched ground truth, -1
 *   dt_ignore  u8    [n_area][n_thr][n_dt]  dtIgnore (match ignored, or unmatched outside the range)
 *   gt_match   int32 [n_area][n_thr][n_gt]  by position: index of the matching detection, -1 */
int glsdet_coco_match(const double* dt_box, const double* dt_area, const int32_t* dt_off, const double* gt_box,
                      const double* gt_area, const unsigned char* gt_flags, const int32_t* gt_off,
                      const int64_t* iou_off, int32_t n_pairs, int32_t n_dt, int32_t n_gt,
                      const double* area_rng, int32_t n_area, const double* iou_thr, int32_t n_thr,
                      double* ious, int32_t* gt_order, unsigned char* gt_ignore, int32_t* n_regular,
                      int32_t* dt_match, unsigned char* dt_ignore, int32_t* gt_match, void* stream);

/* ---------------------------------------------------------------------------------
 * VOC-style mAP (an additive export of ABI 17): the score the drone harness reports, get_map of
 * drone/models/core/utils_map.py:294-813 as called at get_map.py:121-124 -- the matching of :474-512, the curves of
 * :570-617, voc_ap :99-140 and the nine picked miss rates of log_average_miss_rate :26-62 -- for every class and
 * n_thr overlap thresholds in one call, all in fp64, no product fused into a sum.
 *   dt_box [n_dt][4] left, top, right, bottom / score [n_dt]: class-major, inside a class in the reference's rank
 *       order (float(confidence) descending, stable over sorted-file then line order); cls_off int32 [n_cls+1]
 *   the n_pairs (class, image) pairs that own at least one detection:
 *       pair_off int32 [n_pairs+1] into pair_det int32 [n_dt]: the pair's detection indices, ascending (every
 *       detection belongs to exactly one pair); gt_off int32 [n_pairs+1] into gt_box fp64 [n_gt_boxes][4] /
 *       gt_difficult u8 [n_gt_boxes]: the pair's ground truths in file order (a pair may have none)
 *   n_gt int32 [n_cls] non-difficult ground truths of the class; n_img int32 [n_cls] images that hold one
 *   min_overlap fp64 [n_thr]; fppi_ref fp64 [9]: the host's np.logspace(-2, 0, 9)
 * Matching: iw = min(right) - max(left) + 1 (ih alike); a ground truth is a candidate iff iw > 0 and ih > 0;
 *   ov = iw*ih / ((bb area with +1) + (gt area with +1) - iw*ih); ovmax starts at -1 and is replaced on strict >, so
 *   the first ground truth in file order keeps a tie; difficult ones are candidates.  ovmax >= min_overlap: a difficult
 *   match is neither tp nor fp and is not marked used, a used match is fp, otherwise tp; no match is fp.
 * out (device, caller allocated; nothing needs clearing):
 *   tp, fp   int32 [n_thr][n_dt]  cumulative counts in rank order per class
 *   rec      fp64  [n_thr][n_dt]  tp / max(n_gt, 1)        prec  fp64 [n_thr][n_dt]  tp / max(fp + tp, 1)
 *   mpre     fp64  [n_thr][n_dt]  voc_ap's mpre[1 .. n]: the suffix maximum of [prec..., 0]
 *   cls_out  fp64  [n_thr][n_cls][16] = ap (terms (mrec[i]-mrec[i-1])*mpre[i] over the i where mrec changes, added one
 *            at a time in ascending i from 0.0), n_tp, score05_idx (last index with score > 0.5, else 0), F1 / recall /
 *            precision there (F1 = rec*prec*2 / where(prec+rec == 0, 1, prec+rec); zeros for a class without
 *            detections), mr9[9]: for each fppi_ref[k] the last j of [-1, fp / float(n_img)...] that is <= it, picked
 *            from [1, 1 - rec...] (the reference hands `rec` to the parameter it calls `precision`, :617; 1 for a class
 *            without detections, whose lamr the reference sets to 0), and the final fp count.
 *   ws : glsdet_voc_ap_workspace_bytes(n_gt_boxes, n_thr) bytes (the `used` flags; 0 for a negative size or n_thr < 1),
 *        contents irrelevant.
 * Refused on the host: null or misaligned pointers, negative sizes, n_thr < 1, n_pairs > n_dt, a short workspace.  The
 * offset arrays live on the device and are not read back here: glsdet_amd/eval/voc.py checks on the host that they are
 * monotone and that pair_det is a permutation before it uploads them; the kernels clamp every offset to its array, so
 * malformed offsets give wrong numbers and no fault.                                                                    */
int64_t glsdet_voc_ap_workspace_bytes(int32_t n_gt_boxes, int32_t n_thr);
int glsdet_voc_ap(const double* dt_box, const double* score, const int32_t* cls_off, int32_t n_dt, int32_t n_cls,
                  const int32_t* pair_off, const int32_t* pair_det, const int32_t* gt_off, int32_t n_pairs,
                  const double* gt_box, const unsigned char* gt_difficult, int32_t n_gt_boxes,
                  const int32_t* n_gt, const int32_t* n_img, const double* min_overlap, int32_t n_thr,
                  const double* fppi_ref, int32_t* tp, int32_t* fp, double* rec, double* prec, double* mpre,
                  double* cls_out, void* ws, int64_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Baseline JPEG decoding (additive exports of ABI 17): the reference's `Image.open(path)` / `cv2.imread(path)`
 * (drone/yolo.py, get_map*.py, ufpmp_det_eval.py:93), bit for bit what Pillow (libjpeg-turbo, JDCT_ISLOW, fancy
 * upsampling) gives for the same bytes.  The serial part -- markers and Huffman -- runs on the host
 * (csrc/jpeg_host.h, no HIP call: both host functions work without a GPU); everything at pixel rate runs on the device.
 * Accepted streams: SOF0 (baseline, 8 bit, Huffman) with ONE interleaved scan; DQT with 8-bit entries, DHT, DRI, RSTn,
 *   APPn, COM; grayscale (one 1x1 component) or three YCbCr components with luma 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0)
 *   and 1x1 chroma.
 * Refused, with a negative code and a message that names the reason: SOF1 / SOF2 / every other SOFn, arithmetic coding,
 *   12-bit samples, 2 or 4 components, an Adobe APP14 marker whose transform is not 1 (or component ids 'R','G','B')
 *   on a stream without a JFIF marker, other sampling factors, a scan that does not hold every component in frame order
 *   or a marker other than EOI after it (several scans), 16-bit DQT entries, DNL or height 0, a table selector without
 *   a table, a Huffman code that is in no table, a zero run past coefficient 63, a quantised coefficient outside
 *   [-2048, 2047], a missing or out-of-order RSTn, data that ends before the last MCU or before EOI, and
 *   width * height > 2^28.  Every read of `data` is checked against nbytes first.
 * glsdet_jpeg_desc is plain data.  glsdet_jpeg_parse fills all of it; the entropy decoder parses the stream again and
 *   refuses a descriptor that differs from its own; glsdet_jpeg_reconstruct recomputes mcus_*, blocks_* and n_blocks
 *   from width, height, ncomp, hs, vs and refuses a descriptor that differs (they size every device index).
 * glsdet_jpeg_entropy_decode (host buffers): coef = n_blocks * 64 int16, component by component, block raster inside a
 *   component (blocks_x[c] per row), natural (row-major, de-zigzagged) order, NOT dequantised; qtab = [3][64] uint16,
 *   row c = the table of component c in natural order, rows of absent components zero.
 * glsdet_jpeg_reconstruct (device buffers coef, qtab, ws, dst): two kernels,
 *   1. dequantise d = coef * q, libjpeg's jidctint.c (CONST_BITS 13, PASS1_BITS 2: pass 1 down the columns with
 *      descale 11, pass 2 along the rows with descale 18, all in 64-bit integers like libjpeg's `long`), + 128,
 *      saturated to 0..255 -> uint8 component planes of blocks_x*8 by blocks_y*8 in ws, one after the other;
 *   2. jdsample.c's fancy upsampling of the chroma planes' REAL samples (dw = ceil(W*h_c/h_max) by dh alike; triangle
 *      filters h2v1 / h2v2 with the edge samples replicated; plain replication where dw <= 2), jdcolor.c's 16-bit
 *      fixed-point YCbCr -> RGB, each channel clamped, interleaved into rows 0..height-1 of dst, 3*width bytes each at
 *      stride dst_row_bytes >= 3*width (the bytes of a row past 3*width are not written).  order 0 = RGB, 1 = BGR;
 *      grayscale writes Y to all three.
 *   ws: glsdet_jpeg_workspace_bytes(d) bytes (0 for a descriptor reconstruct would refuse), 16-byte aligned, contents
 *   irrelevant.  Refused on the host, nothing launched: null pointers, a short or misaligned workspace,
 *   dst_row_bytes < 3*width, order outside 0..1, an inconsistent descriptor.                                         */
typedef struct glsdet_jpeg_desc {
  int32_t width, height, ncomp;      /* ncomp 1 or 3 */
  int32_t hs[3], vs[3];              /* sampling factors (0 for absent components) */
  int32_t mcus_x, mcus_y, restart_interval;
  int32_t blocks_x[3], blocks_y[3];  /* per component, padded to whole MCUs */
  int64_t n_blocks;                  /* sum over components */
  int64_t scan_offset;               /* first byte of the entropy-coded data */
  int32_t tq[3], td[3], ta[3];       /* quantisation / DC / AC table selectors per component */
  int32_t reserved;                  /* 0 */
} glsdet_jpeg_desc;
int glsdet_jpeg_parse(const unsigned char* data, int64_t nbytes, glsdet_jpeg_desc* d);
int glsdet_jpeg_entropy_decode(const unsigned char* data, int64_t nbytes, const glsdet_jpeg_desc* d, int16_t* coef,
                               uint16_t* qtab);
int64_t glsdet_jpeg_workspace_bytes(const glsdet_jpeg_desc* d);
int glsdet_jpeg_reconstruct(const glsdet_jpeg_desc* d, const int16_t* coef, const uint16_t* qtab, void* ws,
                            int64_t ws_bytes, unsigned char* dst, int64_t dst_row_bytes, int32_t order /* 0 RGB, 1 BGR */,
                            void* stream);

/* ---------------------------------------------------------------------------------
 * Swin trunk (additive exports of ABI 17): the steps of ufp/mmdet/models/backbones/swin.py and of PatchMerging in
 * ufp/mmdet/models/utils/transformer.py that are no convolution (csrc/swin.hip).  The linears around them (qkv, proj,
 * the FFN, reduction) are 1x1 glsdet_conv2d calls.  All three record into a plan and replay from a captured graph;
 * every refusal below happens on the host, before any launch.
 *
 * glsdet_layernorm: nn.LayerNorm over the channels of every token of an NHWC view (norm1 / norm2 of swin.py:361-367,
 *   norm{i} of SwinTransformer.forward, the norms of PatchEmbed and of PatchMerging, transformer.py:383):
 *     y[n,h,w,c] = (x[n,h,w,c] - mean) / sqrt(var + eps) * gamma[c] + beta[c],  var the biased variance over c.
 *   fp32 statistics in TWO passes (mean first, then the sum of squared deviations -- never E[x^2] - mean^2), one wave
 *   per token; the summation order is stated in csrc/swin.hip.  x and y have the same extent and may be strided views;
 *   their dtypes may differ (an fp32 residual stream normalised into the fp16 operand of the next linear).
 *   Refused: C no multiple of 32 or outside [32, 4096] (4096 covers the 4C of every merge up to Swin-L), extents that
 *   differ, a negative or non-finite eps, gamma / beta (fp32 [C]) not 16-byte aligned, a y that overlaps x without being
 *   the very same view (same base, strides and dtype: in place is allowed).
 *
 * glsdet_window_attention: ShiftWindowMSA.forward + WindowMSA.forward (swin.py:80-118, 179-253) WITHOUT the qkv and
 *   proj linears.  qkv [n,H,W,3C] is the output of the qkv linear on the UNPADDED map, channel = which * C + head * 32 + d
 *   (which = 0 q, 1 k, 2 v: the order of the reference's reshape to (3, heads, head_dim), swin.py:89-90); y [n,H,W,C]
 *   receives softmax(q * scale . k^T + bias + mask) . v per window and head, channel = head * 32 + d, in UNSHIFTED
 *   coordinates (swin.py:115, 237-248).  Padding to a multiple of ws (swin.py:186-188), the roll by -shift (:193-196),
 *   window_partition / window_reverse and the roll back are index arithmetic in the kernel: nothing is copied.
 *    (a) padding happens after norm1 and before qkv, so a padded token's q, k, v are qkv_bias (fp32 [3C], rounded to
 *        the storage type as the linear would have stored it; NULL = no bias = zeros).  It takes full part in the
 *        softmax of its window; its output row is dropped.
 *    (b) the shift mask is -100 (not -inf) between tokens of different regions; the nine regions are those of
 *        swin.py:199-219, taken on the PADDED map in SHIFTED coordinates, and are computed from coordinates.
 *    (c) q is scaled before the product (swin.py:94).  bias_table is the module's relative_position_bias_table, fp32
 *        [(2 ws - 1)^2][heads]; the kernel RESTATES relative_position_index (double_step_seq + transpose + flip,
 *        swin.py:64-68): entry (i, j) = (ty_i - ty_j + ws - 1) * (2 ws - 1) + (tx_i - tx_j + ws - 1).  No index tensor
 *        and no gathered [heads, N, N] table is passed.
 *   S = q k^T and O = P v run on v_mfma_f32_32x32x2_f32 in both dtypes (fp32 images of q, k, v in LDS, P stays fp32);
 *   N = ws^2 <= 64 tokens sit in a 64-wide tile whose columns past N are excluded from the softmax.  One workgroup per
 *   (image, window, head), at most 4096 workgroups, each striding over the items.
 *   Refused: head_dim other than 32 (heads * 32 != C), C no multiple of 32 or above 1024, ws outside 2..8, shift
 *   outside 0..ws-1, qkv not [n,H,W,3C] of y's dtype, a non-finite scale, misaligned tables, a y whose span overlaps qkv's.
 *
 * glsdet_patch_merge: PatchMerging.forward up to, not including, norm and reduction (transformer.py:363-382): the
 *   AdaptivePadding('corner') zero fill of an odd H / W (transformer.py:121-125) and nn.Unfold(kernel 2, stride 2), whose
 *   channel order is channel-major:  y[n,oh,ow, 4 c + 2 kh + kw] = x[n, 2 oh + kh, 2 ow + kw, c] (0 past H / W).
 *   The zeros take part in the LayerNorm that follows (a glsdet_layernorm call on y).
 *   Refused: y not [n, ceil(H/2), ceil(W/2), 4C] of x's dtype, C no multiple of 8, a y whose span overlaps x's.      */
int glsdet_layernorm(const glsdet_view* x, const glsdet_view* y, const float* gamma, const float* beta, float eps, void* stream);
int glsdet_window_attention(const glsdet_view* qkv, const glsdet_view* y, const float* bias_table, const float* qkv_bias,
                            int32_t heads, int32_t ws, int32_t shift, float scale, void* stream);
int glsdet_patch_merge(const glsdet_view* x, const glsdet_view* y, void* stream);

/* ---------------------------------------------------------------------------------
 * Plan: a recorded sequence of the calls above, replayed without Python in the loop and
 * capturable into one hipGraph (HIP streams + graphs instead of a tracing compiler).
 * Recording: glsdet_plan_begin(plan) makes every following entry-point call on this
 * thread append to the plan instead of launching; glsdet_plan_end() stops recording.
 */
typedef struct glsdet_plan glsdet_plan;
glsdet_plan* glsdet_plan_create(void);
void    glsdet_plan_destroy(glsdet_plan*);
int     glsdet_plan_begin(glsdet_plan*);
int     glsdet_plan_end(glsdet_plan*);
/* While recording: ops submitted under different non-zero branch ids (1..8) between two
 * branch-0 ops are declared independent of each other; replay runs them on side streams
 * forked from / joined into the main stream (parallel nodes of the captured hipGraph). */
int     glsdet_plan_set_branch(int32_t branch);
int32_t glsdet_plan_num_ops(const glsdet_plan*);
/* kind: 0 conv, 1 focus/pack, 2 pool, 3 resample/upsample-add, 4 nonlocal, 5 decode, 6 nms,
 * 7 groupnorm, 8 proxy scores; flops = 2*MACs */
int     glsdet_plan_op_info(const glsdet_plan*, int32_t i, int32_t* kind, double* flops,
                            double* bytes, char* name, int32_t name_cap);
int     glsdet_plan_run(glsdet_plan*, void* stream);               /* eager replay        */
int     glsdet_plan_capture(glsdet_plan*, void* stream);           /* build the hipGraph  */
int     glsdet_plan_launch(glsdet_plan*, void* stream);            /* hipGraphLaunch      */
/* eager replay with a hipEvent pair around every op; ms[i] accumulates milliseconds      */
int     glsdet_plan_run_timed(glsdet_plan*, void* stream, float* ms /*host, num_ops*/);

const char* glsdet_last_error(void);
int32_t     glsdet_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GLSDET_HIP_H */
