// A whole CSPLayer (64 -> 64 channels, hidden 32, one Bottleneck) in ONE launch
// (drone/models/base/darknet.py:66-112):
//   main  = act(bn(conv1(x)))            64 -> 32, 1x1        |  packed as ONE conv, [conv1 | conv2]
//   short = act(bn(conv2(x)))            64 -> 32, 1x1        |
//   h     = act(bn(m.0.conv1(main)))     32 -> 32, 1x1
//   main' = act(bn(m.0.conv2(h))) [+ main]                    32 -> 32, 3x3 pad 1
//   y     = act(bn(conv3([main' | short])))                   64 -> 64, 1x1
//
// As four launches (conv1|conv2, m.0.conv1, m.0.conv2, conv3) the layer moved 447 MB at 8 x 200 x 336 of which 310 MB
// were three intermediates written once and read once or twice; all four are short-lived-workgroup bound.  The layer has
// 18.4 K weights, so a workgroup keeps ALL of them (the two 64 x 64 1x1s as register-resident A fragments, the Bottleneck's
// 1x1 and 3x3 in LDS) and walks a strip of TH x 16 pixel tiles along x (focus_stem_kernel recipe, stem.hip): per tile
//   load     the x patch of the tile's halo ((TH + 2) x 18 pixels x 128 B) -- requested while the PREVIOUS tile was
//            computed, held in registers -- -> LDS;
//   stage 1  [main | short] on the halo -> patch MS (fp16, all 64 channels of a pixel);
//   stage 2  h on the halo from MS[.., 0:32] -> patch H, ZERO outside the image (the 3x3 pads its INPUT with zeros, not
//            with act(bias)); H takes the bytes of the dead x patch;
//   stage 3  the 3x3 over H for the TH x 16 interior; act, + main (read from MS, one rounding: act(..) + res, then round)
//            -> written over main in MS, which is then [main' | short] = the reference's torch.cat;
//   stage 4  conv3 on the interior of MS -> staged output tile (again over the x patch) -> whole 128-byte pixel runs.
// Every intermediate is rounded to fp16 exactly where the four-launch form stores it, and every product is
// v_mfma_f32_32x32x16_f16 in the k order of the stand-alone kernels (channel-ascending; k = (r * 3 + s) * 32 + ci for
// the 3x3): the result equals the four launches bit for bit (tests/test_csp_fused.py).
// LDS: W(m.0.conv1) 2.5 KB + W(m.0.conv2) 18.5 KB + scale / bias 1.5 KB + [x | H | out] + MS:
//   TH 8: 76.5 KB, TH 4: 58.5 KB -> 2 workgroups / CU either way.
#include "conv_common.h"

namespace glsdet {

struct CspArgs {
  const unsigned char* x_lo;   // allocation of x (buffer descriptor: out-of-image loads return zeros)
  unsigned x_off, x_bytes;
  long x_sn, x_sh, x_sw;       // element strides
  unsigned char* y_lo;         // allocation of y (buffer stores: every lane always issues one, pixels outside the map out of range)
  unsigned y_off, y_bytes;
  long y_sn, y_sh, y_sw;
  const unsigned char *w12, *wm1, *wm2, *w3;
  const float *s12, *b12, *sm1, *bm1, *sm2, *bm2, *s3, *b3;
  int N, H, W, shortcut;
  int kp12, kpm1, kpm2, kp3;   // packed row pitches, elements
  int tiles_x, tiles_y, strips_x, strip;
};

template <int TH>
struct CspGeom {
  static constexpr int PW = 18, PH = TH + 2, NSLOT = PH * PW;
  static constexpr int NHB = (NSLOT + 31) / 32, NS32 = NHB * 32;   // halo pixel blocks of 32
  static constexpr int NPX = TH * 16, NIB = NPX / 32;              // interior pixels / pixel blocks
  static constexpr int RS = 64 * 2 + 16;                           // rows of 64 channels: x, MS, out
  static constexpr int RSH = 32 * 2 + 16;                          // rows of 32 channels: H, W(m.0.conv1)
  static constexpr int RSW = 9 * 32 * 2 + 16;                      // W(m.0.conv2) rows: 288 k + 16 B
  static constexpr int WM1_OFF = 0, WM2_OFF = WM1_OFF + 32 * RSH, SB_OFF = WM2_OFF + 32 * RSW;
  static constexpr int R1_OFF = SB_OFF + 384 * 4;                  // x patch, then H, then the staged output tile
  static constexpr int R2_OFF = R1_OFF + NS32 * RS;                // MS
  static constexpr int LDS = R2_OFF + NS32 * RS;
  // scale / bias in LDS, float offsets
  static constexpr int S12 = 0, B12 = 64, S3 = 128, B3 = 192, SM1 = 256, BM1 = 288, SM2 = 320, BM2 = 352;
};

template <int TH>
__global__ __launch_bounds__(256, 2) void csp_fused_kernel(const CspArgs a) {
  using G = CspGeom<TH>;
  using T = f16;
  constexpr int PW = G::PW, NSLOT = G::NSLOT, NHB = G::NHB, NIB = G::NIB, RS = G::RS, RSH = G::RSH, RSW = G::RSW;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sWm1 = smem + G::WM1_OFF;
  unsigned char* sWm2 = smem + G::WM2_OFF;
  const float* sSB = reinterpret_cast<const float*>(smem + G::SB_OFF);
  unsigned char* sR1 = smem + G::R1_OFF;
  unsigned char* sMS = smem + G::R2_OFF;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  int t;                                           // strip index, XCD-contiguous (conv_bneck.hip)
  {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, local = bid >> 3;
    t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
  }
  const int sx = t % a.strips_x;
  t /= a.strips_x;
  const int ty = t % a.tiles_y, img = t / a.tiles_y;
  const int ty0 = ty * TH;

  // x patch of one tile: thread -> 16-byte chunk tid % 8 of halo slots tid / 8 + 32 i, in registers so that the NEXT
  // tile's loads are in flight while the current tile is multiplied and stored
  const auto xrs = gls_make_rsrc(a.x_lo, a.x_bytes);
  const auto yrs = gls_make_rsrc(a.y_lo, a.y_bytes);
  constexpr int NP = G::NS32 / 32;
  const int kc = tid & 7, slot0 = tid >> 3;
  u32x4 pre[NP];
  auto issue_loads = [&](int tx0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int slot = slot0 + i * 32;
      const int py = slot / PW, px = slot - py * PW;
      const int hi = ty0 - 1 + py, wi = tx0 - 1 + px;
      const bool ok = slot < NSLOT && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
      const unsigned off = ok ? a.x_off + (unsigned)(((long)img * a.x_sn + (long)hi * a.x_sh + (long)wi * a.x_sw + kc * 8) * 2L) : GLS_OOB;
      pre[i] = gls_buf_load16(xrs, off);
    }
  };
  issue_loads(sx * a.strip * 16);

  // resident weights: the Bottleneck's two convs -> LDS, scale / bias of all four -> LDS
  for (int q = tid; q < 32 * 4; q += 256) {
    const int row = q >> 2, c = q & 3;
    *reinterpret_cast<u32x4*>(sWm1 + row * RSH + c * 16) = *reinterpret_cast<const u32x4*>(a.wm1 + (long)row * a.kpm1 * 2 + c * 16);
  }
  for (int q = tid; q < 32 * 36; q += 256) {
    const int row = q / 36, c = q - row * 36;
    *reinterpret_cast<u32x4*>(sWm2 + row * RSW + c * 16) = *reinterpret_cast<const u32x4*>(a.wm2 + (long)row * a.kpm2 * 2 + c * 16);
  }
  if (tid < 96) {
    const float* src;
    int j;
    if (tid < 64) {
      j = tid & 15;
      src = tid < 16 ? a.s12 : (tid < 32 ? a.b12 : (tid < 48 ? a.s3 : a.b3));
    } else {
      j = tid & 7;
      const int k = (tid - 64) >> 3;
      src = k == 0 ? a.sm1 : (k == 1 ? a.bm1 : (k == 2 ? a.sm2 : a.bm2));
    }
    *reinterpret_cast<f32x4*>(smem + G::SB_OFF + tid * 16) = *reinterpret_cast<const f32x4*>(src + j * 4);
  }
  // ... the two 64 x 64 1x1s as A fragments in registers: stage 1 gives a wave ONE cout block (wave & 1) of several pixel
  // blocks, stage 4 unit u = wave + 4 i is (cout block u / NIB, pixel block u % NIB)
  constexpr int NI1 = 2 * NHB / 4, NI4 = 2 * NIB / 4;
  static_assert((2 * NHB) % 4 == 0 && (2 * NIB) % 4 == 0, "units per wave");
  u32x4 a12[4], a3[NI4][4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
    a12[kk] = *reinterpret_cast<const u32x4*>(a.w12 + (long)((wave & 1) * 32 + l31) * a.kp12 * 2 + kk * 32 + lh * 16);
#pragma unroll
  for (int i = 0; i < NI4; ++i)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      a3[i][kk] = *reinterpret_cast<const u32x4*>(a.w3 + (long)(((wave + 4 * i) / NIB) * 32 + l31) * a.kp3 * 2 + kk * 32 + lh * 16);
  // (consumed here so that the wait for these loads sits in front of the tile loop, not inside it where it would also
  // drain the next tile's x loads)
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) asm volatile("" ::"v"(a12[kk]));
#pragma unroll
  for (int i = 0; i < NI4; ++i)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) asm volatile("" ::"v"(a3[i][kk]));

  for (int s = 0; s < a.strip; ++s) {
    const int tx = sx * a.strip + s;
    if (tx >= a.tiles_x) break;                    // uniform
    const int tx0 = tx * 16;
    __syncthreads();                               // the previous tile's store phase is done with R1
#pragma unroll
    for (int i = 0; i < NP; ++i) *reinterpret_cast<u32x4*>(sR1 + (slot0 + i * 32) * RS + kc * 16) = pre[i];
    if (s + 1 < a.strip && tx + 1 < a.tiles_x) issue_loads(tx0 + 16);
    __syncthreads();

    // ---- stage 1: [main | short] = act(bn(W12 . x)) on the halo -> MS
    {
      f32x16 acc[NI1];
#pragma unroll
      for (int i = 0; i < NI1; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;
      const int cb = wave & 1, pb0 = wave >> 1;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int i = 0; i < NI1; ++i) {
          const u32x4 bf = *reinterpret_cast<const u32x4*>(sR1 + ((pb0 + 2 * i) * 32 + l31) * RS + kk * 32 + lh * 16);
          MMA<T>::run(a12[kk], bf, acc[i]);
        }
#pragma unroll
      for (int i = 0; i < NI1; ++i) {
        const int p = (pb0 + 2 * i) * 32 + l31;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int co = cb * 32 + 8 * g + 4 * lh;
          const f32x4 sc = *reinterpret_cast<const f32x4*>(sSB + G::S12 + co), bi = *reinterpret_cast<const f32x4*>(sSB + G::B12 + co);
          const f32x4 xv = {acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
          const f32x4 yv = scale_bias_act4<T>(xv, sc, bi, GLSDET_ACT_SILU);
          const float v[4] = {yv[0], yv[1], yv[2], yv[3]};
          store4(sMS + p * RS + co * 2, v, (T*)nullptr);
        }
      }
    }
    __syncthreads();                               // MS is complete; the x patch is dead: its bytes become H

    // ---- stage 2: h = act(bn(Wm1 . main)) on the halo, zero outside the image -> H
#pragma unroll
    for (int i = 0; i < (NHB + 3) / 4; ++i) {
      const int pb = wave + 4 * i;
      if (pb < NHB) {                              // uniform
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        const int p = pb * 32 + l31;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const u32x4 af = *reinterpret_cast<const u32x4*>(sWm1 + l31 * RSH + kk * 32 + lh * 16);
          const u32x4 bf = *reinterpret_cast<const u32x4*>(sMS + p * RS + kk * 32 + lh * 16);
          MMA<T>::run(af, bf, acc);
        }
        const int py = p / PW, px = p - py * PW;
        const int hi = ty0 - 1 + py, wi = tx0 - 1 + px;
        const bool inside = (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int co = 8 * g + 4 * lh;
          const f32x4 sc = *reinterpret_cast<const f32x4*>(sSB + G::SM1 + co), bi = *reinterpret_cast<const f32x4*>(sSB + G::BM1 + co);
          const f32x4 xv = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
          f32x4 yv = scale_bias_act4<T>(xv, sc, bi, GLSDET_ACT_SILU);
          if (!inside) yv = f32x4{0.f, 0.f, 0.f, 0.f};     // the 3x3's zero padding
          const float v[4] = {yv[0], yv[1], yv[2], yv[3]};
          store4(sR1 + p * RSH + co * 2, v, (T*)nullptr);
        }
      }
    }
    __syncthreads();

    // ---- stage 3: main' = act(bn(Wm2 * h)) [+ main] on the interior, written over main in MS
    if (wave < NIB) {                              // uniform
      f32x16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
      int oy, ox;
      pix_to_xy16<PW>(wave * 32 + l31, oy, ox);
      const unsigned char* brow = sR1 + (oy * PW + ox) * RSH + lh * 16;
      const unsigned char* arow = sWm2 + l31 * RSW + lh * 16;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const u32x4 af = *reinterpret_cast<const u32x4*>(arow + tap * 64 + kk * 32);
          const u32x4 bf = *reinterpret_cast<const u32x4*>(brow + ((tap / 3) * PW + tap % 3) * RSH + kk * 32);
          MMA<T>::run(af, bf, acc);
        }
      unsigned char* mrow = sMS + ((oy + 1) * PW + ox + 1) * RS;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int co = 8 * g + 4 * lh;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(sSB + G::SM2 + co), bi = *reinterpret_cast<const f32x4*>(sSB + G::BM2 + co);
        const f32x4 xv = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        const f32x4 yv = scale_bias_act4<T>(xv, sc, bi, GLSDET_ACT_SILU);
        float v[4] = {yv[0], yv[1], yv[2], yv[3]};
        if (a.shortcut) {                          // act(..) + main in fp32, rounded once (conv_common.h: add_chunk_wide)
          const f16x4 m = *reinterpret_cast<const f16x4*>(mrow + co * 2);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            // the stand-alone kernels add after a trip through LDS; here the activation's last multiply must not be
            // contracted with the add into an fma (one rounding less: not the same bits)
            asm volatile("" : "+v"(v[e]));
            v[e] = v[e] + (float)m[e];
          }
        }
        store4(mrow + co * 2, v, (T*)nullptr);
      }
    }
    __syncthreads();                               // MS = [main' | short]; H is dead: its bytes become the output tile

    // ---- stage 4: y = act(bn(W3 . [main' | short])) on the interior -> staged tile (row-major pixels)
    {
      f32x16 acc[NI4];
#pragma unroll
      for (int i = 0; i < NI4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;
      int pn[NI4];
#pragma unroll
      for (int i = 0; i < NI4; ++i) {
        const int u = wave + 4 * i;
        int oy, ox;
        pix_to_xy16<PW>((u % NIB) * 32 + l31, oy, ox);
        pn[i] = oy * 16 + ox;
        const unsigned char* brow = sMS + ((oy + 1) * PW + ox + 1) * RS + lh * 16;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const u32x4 bf = *reinterpret_cast<const u32x4*>(brow + kk * 32);
          MMA<T>::run(a3[i][kk], bf, acc[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < NI4; ++i) {
        const int cb = (wave + 4 * i) / NIB;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int co = cb * 32 + 8 * g + 4 * lh;
          const f32x4 sc = *reinterpret_cast<const f32x4*>(sSB + G::S3 + co), bi = *reinterpret_cast<const f32x4*>(sSB + G::B3 + co);
          const f32x4 xv = {acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
          const f32x4 yv = scale_bias_act4<T>(xv, sc, bi, GLSDET_ACT_SILU);
          const float v[4] = {yv[0], yv[1], yv[2], yv[3]};
          store4(sR1 + pn[i] * RS + co * 2, v, (T*)nullptr);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < G::NPX * 8 / 256; ++k) {   // eight threads store the 128 bytes of a pixel
      // (unconditional buffer stores: hipcc can then count them, and the wait for the next tile's x loads -- issued
      // before them -- does not drain them: vmcnt counts loads and stores together in issue order)
      const int q = tid + k * 256;
      const int px_l = q >> 3, cq = q & 7;
      const int ho = ty0 + (px_l >> 4), wo = tx0 + (px_l & 15);
      const bool ok = ho < a.H && wo < a.W;
      const unsigned off = ok ? a.y_off + (unsigned)(((long)img * a.y_sn + (long)ho * a.y_sh + (long)wo * a.y_sw + cq * 8) * 2L) : GLS_OOB;
      __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(sR1 + px_l * RS + cq * 16), yrs, (int)off, 0, 0);
    }
  }
}

template <int TH>
static int launch_csp(const CspArgs& a0, hipStream_t st) {
  using G = CspGeom<TH>;
  auto kern = csp_fused_kernel<TH>;
  static bool attr_set = false;
  if (!attr_set && G::LDS > 64 * 1024) {
    GLS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS));
    attr_set = true;
  }
  CspArgs a = a0;
  a.tiles_x = (a.W + 15) / 16;
  a.tiles_y = (a.H + TH - 1) / TH;
  // strip length: the fewest rounds of workgroups over the chip (256 CUs x 2 workgroups), a workgroup costing its tiles
  // + about one more for the weights and the first, unoverlapped x patch; ties -> the longer strip
  const long rows = (long)a.N * a.tiles_y;
  int best = 1;
  long best_cost = -1;
  for (int sl = 1; sl <= 8 && sl <= a.tiles_x; ++sl) {
    const long wgs = rows * ((a.tiles_x + sl - 1) / sl);
    const long cost = ((wgs + 511) / 512) * (sl + 1);
    if (best_cost < 0 || cost <= best_cost) { best = sl; best_cost = cost; }
  }
  a.strip = best;
  a.strips_x = (a.tiles_x + a.strip - 1) / a.strip;
  const long grid = rows * a.strips_x;
  if (grid <= 0 || grid > 0x7fffffffL) GLS_FAIL(GLSDET_E_ARG, "csp_fused: grid %ld out of range", grid);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), G::LDS, st, a);
  GLS_HIP(hipGetLastError());
  return 0;
}

// validate the descriptor and build the op; hint 0: 8 x 16 pixel tiles, 1: 4 x 16
static int build_csp_op(const glsdet_csp_desc* d, int hint, OpRecord& op) {
  if (!d) GLS_FAIL(GLSDET_E_ARG, "csp_fused: null descriptor");
  const glsdet_view &x = d->x, &y = d->y;
  int rc;
  if ((rc = check_view(x, "csp_fused.x"))) return rc;
  if ((rc = check_view(y, "csp_fused.y"))) return rc;
  if (x.dtype != GLSDET_F16 || y.dtype != GLSDET_F16) GLS_FAIL(GLSDET_E_ARG, "csp_fused: fp16 storage only");
  if (x.c != 64 || y.c != 64) GLS_FAIL(GLSDET_E_ARG, "csp_fused: 64 -> 64 channels (hidden 32, one Bottleneck) only, got %d -> %d", x.c, y.c);
  if (y.n != x.n || y.h != x.h || y.w != x.w) GLS_FAIL(GLSDET_E_ARG, "csp_fused: output extent [%d,%d,%d] != input [%d,%d,%d]", y.n, y.h, y.w, x.n, x.h, x.w);
  const void* ptrs[12] = {d->w12, d->scale12, d->bias12, d->wm1, d->scalem1, d->biasm1, d->wm2, d->scalem2, d->biasm2, d->w3, d->scale3, d->bias3};
  for (const void* p : ptrs) {
    if (!p) GLS_FAIL(GLSDET_E_ARG, "csp_fused: null weight/scale/bias");
    if ((uintptr_t)p & 15) GLS_FAIL(GLSDET_E_ALIGN, "csp_fused: weight/scale/bias must be 16-byte aligned");
  }
  if (d->act != GLSDET_ACT_SILU) GLS_FAIL(GLSDET_E_ARG, "csp_fused: act %d, only SiLU (BaseConv's) is compiled", d->act);
  if (d->shortcut != 0 && d->shortcut != 1) GLS_FAIL(GLSDET_E_ARG, "csp_fused: shortcut must be 0 or 1");
  if (hint != 0 && hint != 1) GLS_FAIL(GLSDET_E_ARG, "csp_fused: hint must be 0 (8 x 16 tiles) or 1 (4 x 16)");
  const long M = (long)x.n * x.h * x.w;
  if (M <= 0 || M > 0x7fffffffL) GLS_FAIL(GLSDET_E_ARG, "csp_fused: pixel count %ld out of range", M);
  const int64_t xalloc = (const char*)x.alloc_hi - (const char*)x.alloc_lo;
  const int64_t yalloc = (const char*)y.alloc_hi - (const char*)y.alloc_lo;
  if (xalloc >= 0x7fffffffLL || yalloc >= 0x7fffffffLL)
    GLS_FAIL(GLSDET_E_ARG, "csp_fused: operand allocation of %lld bytes exceeds the 2 GiB descriptor range", (long long)(xalloc > yalloc ? xalloc : yalloc));
  // in place is impossible: a workgroup reads the halo of x while its neighbours store their tiles of y
  // (overlapping address ranges are fine only for disjoint channel slices of one pixel-interleaved buffer)
  if (views_overlap(x, y) && !channel_slices_disjoint(x, y)) GLS_FAIL(GLSDET_E_ARG, "csp_fused: y overlaps x (the fused form cannot run in place)");
  CspArgs a = {};
  a.x_lo = (const unsigned char*)x.alloc_lo;
  a.x_off = (unsigned)((const char*)x.base - (const char*)x.alloc_lo);
  a.x_bytes = (unsigned)xalloc;
  a.x_sn = x.sn; a.x_sh = x.sh; a.x_sw = x.sw;
  a.y_lo = (unsigned char*)y.alloc_lo;
  a.y_off = (unsigned)((const char*)y.base - (const char*)y.alloc_lo);
  a.y_bytes = (unsigned)yalloc;
  a.y_sn = y.sn; a.y_sh = y.sh; a.y_sw = y.sw;
  a.w12 = (const unsigned char*)d->w12; a.s12 = d->scale12; a.b12 = d->bias12;
  a.wm1 = (const unsigned char*)d->wm1; a.sm1 = d->scalem1; a.bm1 = d->biasm1;
  a.wm2 = (const unsigned char*)d->wm2; a.sm2 = d->scalem2; a.bm2 = d->biasm2;
  a.w3 = (const unsigned char*)d->w3; a.s3 = d->scale3; a.b3 = d->bias3;
  a.N = x.n; a.H = x.h; a.W = x.w; a.shortcut = d->shortcut;
  a.kp12 = a.kp3 = glsdet_conv_kpad(1, 1, 64, GLSDET_F16);
  a.kpm1 = glsdet_conv_kpad(1, 1, 32, GLSDET_F16);
  a.kpm2 = glsdet_conv_kpad(3, 3, 32, GLSDET_F16);
  op.kind = 0;
  op.flops = 2.0 * (double)M * (64.0 * 64 + 32.0 * 32 + 32.0 * 288 + 64.0 * 64);   // algorithmic: no halo recompute
  op.bytes = 2.0 * (double)M * 64 * 2;
  char nm[112];
  snprintf(nm, sizeof nm, "csp_fused<f16,32,%dx16> 64->64 hid32 3x3%s", hint ? 4 : 8, d->shortcut ? " +x" : "");
  op.name = nm;
  op.launch = [a, hint](hipStream_t st) -> int { return hint ? launch_csp<4>(a, st) : launch_csp<8>(a, st); };
  return 0;
}

}  // namespace glsdet

using namespace glsdet;

extern "C" int glsdet_csp_fused(const glsdet_csp_desc* d, int32_t hint, void* stream) {
  OpRecord op;
  int rc = build_csp_op(d, hint, op);
  if (rc) return rc;
  return submit(std::move(op), stream);
}

// times both tile heights on the device (one warm launch, then the minimum over 3 rounds of 5 back-to-back launches each,
// the rounds interleaved) and reports the faster
extern "C" int glsdet_csp_fused_tune(const glsdet_csp_desc* d, void* stream, int32_t* best_hint, float* best_us) {
  if (!best_hint) GLS_FAIL(GLSDET_E_ARG, "csp_fused_tune: null argument");
  OpRecord ops[2];
  for (int h = 0; h < 2; ++h) {
    int rc = build_csp_op(d, h, ops[h]);
    if (rc) return rc;
  }
  hipStream_t st = (hipStream_t)stream;
  for (int h = 0; h < 2; ++h) {
    int rc = ops[h].launch(st);
    if (rc) return rc;
  }
  constexpr int TRIALS = 3, REPS = 5;
  hipEvent_t e0, e1;
  GLS_HIP(hipEventCreate(&e0));
  GLS_HIP(hipEventCreate(&e1));
  float us[2] = {1e30f, 1e30f};
  int rc = 0;
  for (int t = 0; t < TRIALS && !rc; ++t)
    for (int h = 0; h < 2 && !rc; ++h) {
      (void)hipEventRecord(e0, st);
      for (int r = 0; r < REPS && !rc; ++r) rc = ops[h].launch(st);
      (void)hipEventRecord(e1, st);
      if (hipEventSynchronize(e1) != hipSuccess) rc = GLSDET_E_HIP;
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, e0, e1);
      if (!rc && ms * 1000.f / REPS < us[h]) us[h] = ms * 1000.f / REPS;
    }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc) GLS_FAIL(rc, "csp_fused_tune: a timed launch failed");
  *best_hint = us[1] < us[0] ? 1 : 0;
  if (best_us) *best_us = us[*best_hint];
  set_error("");
  return 0;
}
