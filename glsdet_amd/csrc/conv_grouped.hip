// Grouped 3x3 convolution + folded BN + activation: conv2 of the ResNeXt Bottleneck (ufp/mmdet/models/backbones/
// resnext.py:55-64; 32 or 64 groups of Cg = 4 / 8 / 16 / 32 channels).  x.c == y.c == groups * Cg, pad 1, stride 1 or 2.
//
// The channels are cut into BLOCKS of 32: output channels [32 b, 32 b + 32) depend on input channels of the same range
// only (Cg divides 32, so a block holds 32 / Cg whole groups).  The host packs the weights as zero-filled block-diagonal
// 32 x 32 tiles, one per (block, tap):
//     w[b][t = r * 3 + s][co_l][ci_l],  co = 32 b + co_l, ci = 32 b + ci_l:
//         weight[co][ci - (co / Cg) * Cg][r][s]   where ci lies in the group of co (and co, ci < C),   0 elsewhere
// in elements of x.dtype -- glsdet_conv_grouped_weight_elems(groups, Cg) = ceil(C / 32) * 9 * 32 * 32 of them.  scale / bias:
// fp32 [ceil(C / 32) * 32].  One K step is one tap of one block: the multiplies wasted on the zero fill are 32 / Cg <= 8x;
// the block-diagonal conv over all C channels wastes C / Cg (up to 64x).  Measured (the conv2 shapes
// of X-101 at 8 x 800 x 1344): 2.2x .. 2.7x the layer's HBM time at stride 2, 3.3x .. 4.3x at stride 1 -- the arithmetic is
// not what bounds it, the re-read of the taps is.
//
// A wave owns one block's weights in registers (9 taps x 32 rows x 32 channels = 18 chunks of 8 channels per lane) and
// walks 16-pixel groups of the flat output pixel range.  fp16: v_mfma_f32_16x16x32_f16, A = weights (lane -> row lane % 16,
// channels 8 (lane / 16) .. + 7), B = pixels (lane -> pixel lane % 16, the same 8 channels: ONE 16-byte load per tap),
// D: lane -> pixel lane % 16, rows 4 (lane / 16) .. + 3.  Two products per tap, over the cout rows 8 j + {0..3} and
// 8 j + {4..7} (j = row / 4): a lane then holds the 8 CONSECUTIVE output channels 32 b + 8 (lane / 16) .. + 7 of its pixel
// -- the channels it also loads -- and stores them as one 16-byte chunk.  fp32: v_mfma_f32_16x16x4f32 (exact fp32 products,
// A / B lane -> k = lane / 16) on the same fragments; step e takes element e of every lane's 8 channels, which is a
// permutation of K that both operands share.  The taps come straight from global memory (L1 / L2 serve the 9-fold
// re-read); out-of-map taps, pixels past the end and channels past C are ZERO fragments, never loads.
#include <vector>

#include "conv_common.h"

namespace glsdet {

struct GroupedArgs {
  const unsigned char* x;
  const unsigned char* w;
  const float* scale;
  const float* bias;
  unsigned char* y;
  long x_sn, x_sh, x_sw, y_sn, y_sh, y_sw;
  int H, W, C, Ho, Wo, stride, act;
  int M;                    // N * Ho * Wo
  int ngroups;              // 16-pixel groups
  unsigned howo_mul, wo_mul;  // p / (Ho * Wo), rem / Wo without a division (gls_fastdiv)
  int howo_sh, wo_sh;
};

// Workgroups of a launch (grid-stride over the pixel groups beyond).  768 = 256 CUs x 3: what the fp16 kernel (146 VGPRs)
// holds resident at once; the fp32 kernel (250 VGPRs) holds fewer and runs them in rounds.  Measured: 1024 and 768 give
// the same times within 2 % on the large maps (64 x 4 at 200 x 336: 360.1 and 359.7 us) -- the cap is not what bounds the kernel.
#define GLS_GROUPED_MAX_WG 768

template <typename T>
__global__ __launch_bounds__(256) void conv_grouped_kernel(const GroupedArgs a) {
  constexpr int ES = (int)sizeof(T), NV = 8 * ES / 16;      // 16-byte chunks of a lane's 8 channels: 1 (f16), 2 (f32)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int blk = blockIdx.x;
  const int c0 = blk * 32 + q * 8;                          // this lane's 8 channels, as input and as output
  const bool c_ok = c0 < a.C;                               // (C % 8 == 0: a chunk is inside or outside as a whole)
  const u32x4 zero = {0u, 0u, 0u, 0u};

  u32x4 wf[9][2][NV];
  const unsigned char* wb = a.w + (long)blk * (9 * 32 * 32 * ES);
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = 8 * (r >> 2) + 4 * h + (r & 3);
#pragma unroll
      for (int v = 0; v < NV; ++v)
        wf[t][h][v] = *reinterpret_cast<const u32x4*>(wb + ((t * 32 + row) * 32 + q * 8) * ES + v * 16);
    }
  f32x4 sc[2], bi[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    sc[h] = *reinterpret_cast<const f32x4*>(a.scale + blk * 32 + q * 8 + 4 * h);
    bi[h] = *reinterpret_cast<const f32x4*>(a.bias + blk * 32 + q * 8 + 4 * h);
  }

  const int HoWo = a.Ho * a.Wo;
  for (int g = blockIdx.y * 4 + wave; g < a.ngroups; g += gridDim.y * 4) {     // wave-uniform trip count
    const long pl = (long)g * 16 + r;
    const bool p_ok = pl < (long)a.M;
    const int p = p_ok ? (int)pl : 0;
    const int n = gls_div(p, a.howo_mul, a.howo_sh), rem = p - n * HoWo;
    const int ho = gls_div(rem, a.wo_mul, a.wo_sh), wo = rem - ho * a.Wo;
    const bool live = p_ok && c_ok;
    const long xbase = (long)n * a.x_sn + c0;
    u32x4 bx[9][NV];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int hi = ho * a.stride - 1 + t / 3, wi = wo * a.stride - 1 + t % 3;
      const bool ok = live && hi >= 0 && hi < a.H && wi >= 0 && wi < a.W;
      const unsigned char* px = a.x + (xbase + (long)hi * a.x_sh + (long)wi * a.x_sw) * ES;
#pragma unroll
      for (int v = 0; v < NV; ++v) bx[t][v] = ok ? *reinterpret_cast<const u32x4*>(px + v * 16) : zero;
    }
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if constexpr (ES == 2) {
          mma16(wf[t][h][0], bx[t][0], acc[h]);
        } else {
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            const f32x4 af = __builtin_bit_cast(f32x4, wf[t][h][v]), bf = __builtin_bit_cast(f32x4, bx[t][v]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[e], bf[e], acc[h], 0, 0, 0);
          }
        }
      }
    if (live) {
      const f32x4 o0 = scale_bias_act4<T>(acc[0], sc[0], bi[0], a.act);
      const f32x4 o1 = scale_bias_act4<T>(acc[1], sc[1], bi[1], a.act);
      unsigned char* py = a.y + ((long)n * a.y_sn + (long)ho * a.y_sh + (long)wo * a.y_sw + c0) * ES;
      if constexpr (ES == 2) {
        const f16x8 o = {(f16)o0[0], (f16)o0[1], (f16)o0[2], (f16)o0[3], (f16)o1[0], (f16)o1[1], (f16)o1[2], (f16)o1[3]};
        *reinterpret_cast<f16x8*>(py) = o;
      } else {
        *reinterpret_cast<f32x4*>(py) = o0;
        *reinterpret_cast<f32x4*>(py + 16) = o1;
      }
    }
  }
}

static bool grouped_width_ok(int cg) { return cg == 4 || cg == 8 || cg == 16 || cg == 32; }

// validate the descriptor, fill the argument block and the op
static int build_grouped_op(const glsdet_conv_desc* d, int32_t groups, OpRecord& op) {
  if (!d) GLS_FAIL(GLSDET_E_ARG, "conv2d_grouped: null descriptor");
  const glsdet_view &x = d->x, &y = d->y;
  int rc;
  if ((rc = check_view(x, "conv2d_grouped.x"))) return rc;
  if ((rc = check_view(y, "conv2d_grouped.y"))) return rc;
  if (x.dtype != y.dtype) GLS_FAIL(GLSDET_E_ARG, "conv2d_grouped: x and y must share one dtype");
  if (groups < 1 || x.c != y.c || x.c % groups || !grouped_width_ok(x.c / groups))
    GLS_FAIL(GLSDET_E_ARG, "conv2d_grouped: x.c == y.c == groups * Cg with Cg in {4, 8, 16, 32} (x.c %d, y.c %d, groups %d)", x.c,
             y.c, groups);
  if (x.c % 8) GLS_FAIL(GLSDET_E_ARG, "conv2d_grouped: channels must be a multiple of 8 (%d)", x.c);
  if (d->R != 3 || d->S != 3 || d->pad != 1 || (d->stride != 1 && d->stride != 2))
    GLS_FAIL(GLSDET_E_ARG, "conv2d_grouped: 3x3, pad 1, stride 1 or 2 only (R %d S %d pad %d stride %d)", d->R, d->S, d->pad, d->stride);
  if (d->res.base) GLS_FAIL(GLSDET_E_ARG, "conv2d_grouped: residual not supported");
  const int Ho = (x.h - 1) / d->stride + 1, Wo = (x.w - 1) / d->stride + 1;
  if (y.n != x.n || y.h != Ho || y.w != Wo)
    GLS_FAIL(GLSDET_E_ARG, "conv2d_grouped: output extent [%d,%d,%d] != expected [%d,%d,%d]", y.n, y.h, y.w, x.n, Ho, Wo);
  if (!d->w || !d->scale || !d->bias) GLS_FAIL(GLSDET_E_ARG, "conv2d_grouped: null weight/scale/bias");
  if (((uintptr_t)d->w | (uintptr_t)d->scale | (uintptr_t)d->bias) & 15)
    GLS_FAIL(GLSDET_E_ALIGN, "conv2d_grouped: weight/scale/bias must be 16-byte aligned");
  if (d->act < 0 || d->act > 5) GLS_FAIL(GLSDET_E_ARG, "conv2d_grouped: bad act %d", d->act);
  if (d->tile_hint != 0) GLS_FAIL(GLSDET_E_ARG, "conv2d_grouped: tile_hint must be 0 (one kernel)");
  const long M = (long)x.n * Ho * Wo;
  if (M <= 0 || M > 0x7fffffffL - 16) GLS_FAIL(GLSDET_E_ARG, "conv2d_grouped: pixel count %ld out of range", M);
  // the kernel keeps no copy of x: a workgroup must not store where another still reads
  const int es = dtype_size(x.dtype);
  if (views_overlap(x, y) && !channel_slices_disjoint(x, y)) GLS_FAIL(GLSDET_E_ARG, "conv2d_grouped: y overlaps x (the conv cannot run in place)");

  GroupedArgs a;
  a.x = (const unsigned char*)x.base;
  a.w = (const unsigned char*)d->w;
  a.scale = d->scale;
  a.bias = d->bias;
  a.y = (unsigned char*)y.base;
  a.x_sn = x.sn; a.x_sh = x.sh; a.x_sw = x.sw;
  a.y_sn = y.sn; a.y_sh = y.sh; a.y_sw = y.sw;
  a.H = x.h; a.W = x.w; a.C = x.c; a.Ho = Ho; a.Wo = Wo;
  a.stride = d->stride; a.act = d->act;
  a.M = (int)M;
  a.ngroups = (int)((M + 15) / 16);
  gls_fastdiv(Ho * Wo, &a.howo_mul, &a.howo_sh);
  gls_fastdiv(Wo, &a.wo_mul, &a.wo_sh);
  const int dt = x.dtype, nblk = (x.c + 31) / 32, cg = x.c / groups;
  char nm[112];
  snprintf(nm, sizeof nm, "conv_grouped<%s> 3x3 s%d g%d cg%d blk32x%d", dt ? "f32" : "f16", d->stride, groups, cg, nblk);
  op = make_op(0, 2.0 * (double)M * x.c * 9 * cg, ((double)x.n * x.h * x.w + (double)M) * x.c * es + (double)nblk * 9 * 32 * 32 * es, nm);
  op.launch = [a, dt, nblk](hipStream_t st) -> int {
    int gy = (a.ngroups + 3) / 4;
    const int cap = GLS_GROUPED_MAX_WG / nblk > 1 ? GLS_GROUPED_MAX_WG / nblk : 1;
    if (gy > cap) gy = cap;
    const dim3 grid((unsigned)nblk, (unsigned)gy);
    with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(conv_grouped_kernel<decltype(t)>, grid, dim3(256), 0, st, a); });
    GLS_HIP(hipGetLastError());
    return 0;
  };
  return 0;
}

}  // namespace glsdet

using namespace glsdet;

extern "C" int64_t glsdet_conv_grouped_weight_elems(int32_t groups, int32_t cg) {
  if (groups < 1 || !grouped_width_ok(cg) || (int64_t)groups * cg > 0x7fffffffLL / 512) return 0;
  return (int64_t)((groups * cg + 31) / 32) * 9 * 32 * 32;
}

extern "C" int glsdet_conv2d_grouped(const glsdet_conv_desc* d, int32_t groups, void* stream) {
  OpRecord op;
  int rc = build_grouped_op(d, groups, op);
  if (rc) return rc;
  return submit(std::move(op), stream);
}

extern "C" int glsdet_conv2d_grouped_tune(const glsdet_conv_desc* d, int32_t groups, void* stream, int32_t* best_hint,
                                          float* best_us) {
  if (!best_hint) GLS_FAIL(GLSDET_E_ARG, "conv2d_grouped_tune: null argument");
  std::vector<OpRecord> ops(1);
  int rc = build_grouped_op(d, groups, ops[0]);
  if (rc) return rc;
  return tune_report(ops, {0}, stream, "conv2d_grouped_tune: the kernel failed to launch", best_hint, best_us);
}
