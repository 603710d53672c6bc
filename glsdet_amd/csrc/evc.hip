// The three steps of the reference's EVCBlock (models/cfp/evc_blocks.py:214-308) that no other entry point covers:
//   glsdet_lvc_encode    the codebook Encoding layer (models/cfp/Functions.py:25-84) on the matrix cores
//   glsdet_lvc_gate      BatchNorm1d per code + ReLU + mean over the codes + fc + sigmoid of LVCBlock.forward
//   glsdet_channel_fuse  the two per-channel elementwise steps: relu(x + x * gam) and x + ls * t
//
// Encoding, with x [N pixels][C], c [64][C], s [64]:  A = softmax_k(s_k |x_n - c_k|^2),  E[k] = sum_n A[n][k] (x_n - c_k).
// The reference expands [B, N, 64, C] tensors twice.  Here, per tile of 64 pixels:
//   dot[n][k] = sum_ch x[n][ch] c[k][ch]                 [64 x C] . [C x 64] on v_mfma_f32_32x32x2_f32, ch ascending
//   D[n][k]   = s_k * (fmaf(-2, dot, |x_n|^2) + |c_k|^2)  |x_n|^2, |c_k|^2: four interleaved fmaf chains (channel j of a
//               32-channel chunk goes to chain j / 8), added as ((p0 + p1) + p2) + p3
//   A[n][k]   = expf(D - max_k D) / sum_k, the sum as four chains of 16 codes added as ((q0 + q1) + q2) + q3
//   Ep[k][ch] += sum_n A[n][k] x[n][ch]                  [64 x 64 pixels] . [64 pixels x C] on the same MFMA, n ascending
//   Sp[k]     += sum_n A[n][k]                           n ascending
// A lives in LDS only.  The pixels of an image are cut into slices by lvc_slices(h * w); a workgroup owns one (slice, image,
// 64-channel chunk) and writes its Ep / Sp to the workspace; lvc_fold_kernel adds the slices in ascending order:
// E = fmaf(-(Sp_0 + Sp_1 + ...), c, Ep_0 + Ep_1 + ...).  No atomics: a replay reproduces the bits.
// The workgroups of the channel chunks of one slice each compute the logits of its pixels (the same instructions on the same
// operands, hence the same A): at C = 256 that is 2.5 x the 0.28 GFLOP per image of the arithmetic, still far below a
// microsecond of the fp32 matrix rate, and it keeps every accumulator in 16 registers for any C.
// 256 threads = 2 x 2 waves on 32 x 32 accumulator tiles; lane maps in mfma_tile.h.
#include "mfma_tile.h"

namespace glsdet {

#define GLS_LVC_K 64            // codewords (evc_blocks.py:219 hard-wires 64)
#define GLS_LVC_MAXC 640
#define GLS_LVC_PT 64           // pixels per tile
#define GLS_LVC_SLICE 128       // smallest slice
#define GLS_LVC_MAXSL 64        // most slices per image
#define GLS_LVC_MAXPIX (1 << 24)

// the slice rule: a function of the pixel count alone
static inline void lvc_slices(long N, int* chunk, int* nsl) {
  long per = (N + (long)GLS_LVC_SLICE * GLS_LVC_MAXSL - 1) / ((long)GLS_LVC_SLICE * GLS_LVC_MAXSL);
  if (per < 1) per = 1;
  *chunk = (int)(per * GLS_LVC_SLICE);
  *nsl = (int)((N + *chunk - 1) / *chunk);
}

struct LvcArgs {
  const unsigned char* x;
  long xsn, xsh, xsw;
  const float *cw, *scale;
  float *Ep, *Sp, *E;
  int n, H, W, C, nsl, chunk;
};

// grid (slice, image, 64-channel chunk)
template <typename T>
__global__ __launch_bounds__(256) void lvc_encode_kernel(const LvcArgs a) {
  constexpr int VN = Vec16<T>::N;
  typedef typename Vec16<T>::type V;
  constexpr int LD1 = 33, LDD = 65;
  __shared__ __attribute__((aligned(16))) float stage[2 * 64 * 33];          // phase 1: xs | cs as [64][33] each; phase 2: [pixel][64 channels]
  __shared__ float Ds[GLS_LVC_PT * LDD];
  __shared__ __attribute__((aligned(16))) float As[GLS_LVC_PT * GLS_LVC_K];   // [pixel][code]
  __shared__ float xxs[GLS_LVC_PT], ccs[GLS_LVC_K], scs[GLS_LVC_K];
  float* xs = stage;
  float* cs = stage + 64 * LD1;
  const int z = blockIdx.x, b = blockIdx.y, c0 = blockIdx.z * 64;
  const int C = a.C, W = a.W, N = a.H * W;
  const int cw_ = min(64, C - c0);                                  // 32 or 64 channels of this chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int row4 = tid >> 2, part = tid & 3;
  const int pbeg = z * a.chunk, pend = min(N, pbeg + a.chunk);
  const T* xb = reinterpret_cast<const T*>(a.x) + b * a.xsn;
  if (tid < GLS_LVC_K) scs[tid] = a.scale[tid];
  f32x16 accE;
#pragma unroll
  for (int r = 0; r < 16; ++r) accE[r] = 0.f;
  float ssum = 0.f;                                                 // Sp of code tid (threads 0..63)
  for (int p0 = pbeg; p0 < pend; p0 += GLS_LVC_PT) {
    // ---- phase 1: dot, |x|^2, |c|^2 over the channels in chunks of 32
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float xxp = 0.f, ccp = 0.f;
    for (int k0 = 0; k0 < C; k0 += 32) {
      constexpr int CPR = 32 / VN;                                  // 16-byte chunks of x per pixel
      for (int t = tid; t < GLS_LVC_PT * CPR; t += 256) {
        const int r = t / CPR, ch = t - r * CPR;
        const int p = p0 + r;
        V v;
#pragma unroll
        for (int e = 0; e < VN; ++e) v[e] = (T)0.f;
        if (p < pend) v = *reinterpret_cast<const V*>(xb + (long)(p / W) * a.xsh + (long)(p % W) * a.xsw + k0 + ch * VN);
#pragma unroll
        for (int e = 0; e < VN; ++e) xs[r * LD1 + ch * VN + e] = (float)v[e];
      }
      for (int t = tid; t < GLS_LVC_K * 8; t += 256) {
        const int r = t >> 3, c4 = (t & 7) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(a.cw + (long)r * C + k0 + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) cs[r * LD1 + c4 + e] = v[e];
      }
      __syncthreads();
      {
        const float* pa = xs + (wm + l31) * LD1 + hi;
        const float* pb = cs + (wn + l31) * LD1 + hi;
        acc = mfma32_f32<16, 2, 2>(pa, pb, acc);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xv = xs[row4 * LD1 + part * 8 + j], cv = cs[row4 * LD1 + part * 8 + j];
        xxp = fmaf(xv, xv, xxp);
        ccp = fmaf(cv, cv, ccp);
      }
      __syncthreads();
    }
    {
      const int base = lane & ~3;
      const float x0 = __shfl(xxp, base, 64), x1 = __shfl(xxp, base + 1, 64), x2 = __shfl(xxp, base + 2, 64), x3 = __shfl(xxp, base + 3, 64);
      const float q0 = __shfl(ccp, base, 64), q1 = __shfl(ccp, base + 1, 64), q2 = __shfl(ccp, base + 2, 64), q3 = __shfl(ccp, base + 3, 64);
      if (part == 0) {
        xxs[row4] = ((x0 + x1) + x2) + x3;
        ccs[row4] = ((q0 + q1) + q2) + q3;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int px = wm + mfma32_row(r, lane), k = wn + l31;
      Ds[px * LDD + k] = scs[k] * (fmaf(-2.f, acc[r], xxs[px]) + ccs[k]);
    }
    // the 64 x 64 image of this chunk's channels for phase 2 (the staging area is free: everyone is past the last MFMA)
    {
      constexpr int CPP = 64 / VN;
      for (int t = tid; t < GLS_LVC_PT * CPP; t += 256) {
        const int r = t / CPP, ch = t - r * CPP;
        const int p = p0 + r;
        V v;
#pragma unroll
        for (int e = 0; e < VN; ++e) v[e] = (T)0.f;
        if (p < pend && ch * VN < cw_) v = *reinterpret_cast<const V*>(xb + (long)(p / W) * a.xsh + (long)(p % W) * a.xsw + c0 + ch * VN);
#pragma unroll
        for (int e = 0; e < VN; ++e) stage[r * 64 + ch * VN + e] = (float)v[e];
      }
    }
    __syncthreads();
    // ---- softmax over the 64 codes of pixel row4: four lanes, 16 codes each
    {
      float d[16];
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        d[j] = Ds[row4 * LDD + part * 16 + j];
        m = fmaxf(m, d[j]);
      }
      m = fmaxf(m, __shfl_xor(m, 1, 64));
      m = fmaxf(m, __shfl_xor(m, 2, 64));
      float q = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        d[j] = expf(d[j] - m);
        q += d[j];
      }
      const int base = lane & ~3;
      const float q0 = __shfl(q, base, 64), q1 = __shfl(q, base + 1, 64), q2 = __shfl(q, base + 2, 64), q3 = __shfl(q, base + 3, 64);
      const float tot = ((q0 + q1) + q2) + q3;
      const bool live = p0 + row4 < pend;
#pragma unroll
      for (int j = 0; j < 16; ++j) As[row4 * GLS_LVC_K + part * 16 + j] = live ? d[j] / tot : 0.f;
    }
    __syncthreads();
    // ---- phase 2: Ep[code][channel] += A^T X over the tile's pixels
    if (wn < cw_) {
      const float* pa = As + hi * GLS_LVC_K + wm + l31;
      const float* pb = stage + hi * 64 + wn + l31;
#pragma unroll
      for (int s = 0; s < GLS_LVC_PT / 2; ++s) accE = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[s * 128], pb[s * 128], accE, 0, 0, 0);
    }
    if (tid < GLS_LVC_K) {
      for (int p = 0; p < GLS_LVC_PT; ++p) ssum += As[p * GLS_LVC_K + tid];
    }
    __syncthreads();
  }
  const long slot = (long)b * a.nsl + z;
  if (wn < cw_) {
    float* o = a.Ep + (slot * GLS_LVC_K + wm) * C + c0 + wn + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[(long)mfma32_row(r, lane) * C] = accE[r];
  }
  if (blockIdx.z == 0 && tid < GLS_LVC_K) a.Sp[slot * GLS_LVC_K + tid] = ssum;
}

// E[b][k][ch] = fmaf(-(Sp_0 + Sp_1 + ...), c[k][ch], Ep_0 + Ep_1 + ...): one thread per four channels, slices ascending
__global__ __launch_bounds__(256) void lvc_fold_kernel(const LvcArgs a) {
  const int C4 = a.C / 4;
  const long total = (long)a.n * GLS_LVC_K * C4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c4 = (int)(i % C4);
    const long bk = i / C4;
    const int k = (int)(bk % GLS_LVC_K), b = (int)(bk / GLS_LVC_K);
    f32x4 e = {0.f, 0.f, 0.f, 0.f};
    float s = 0.f;
    for (int z = 0; z < a.nsl; ++z) {
      const long slot = (long)b * a.nsl + z;
      e += *reinterpret_cast<const f32x4*>(a.Ep + (slot * GLS_LVC_K + k) * a.C + c4 * 4);
      s += a.Sp[slot * GLS_LVC_K + k];
    }
    const f32x4 c = *reinterpret_cast<const f32x4*>(a.cw + (long)k * a.C + c4 * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = fmaf(-s, c[j], e[j]);
    *reinterpret_cast<f32x4*>(a.E + ((long)b * GLS_LVC_K + k) * a.C + c4 * 4) = e;
  }
}

// ---------------------------------------------------------------- gate
// grid (ceil(C / 64), image), 64 threads: every workgroup forms en[C] in LDS, thread t the output channel 64 blockIdx.x + t:
//   en[c]   = (m_63) * (1 / 64),  m_-1 = 0,  m_k = m_{k-1} + fmaxf(fmaf(a_k, E[b][k][c], b_k), 0)        k ascending
//   gam[co] = sigmoid(v_{C-1}),   v_-1 = bias[co],  v_c = fmaf(W[co][c], en[c], v_{c-1})                 c ascending
//   sigmoid(v) = 1 / (1 + expf(-v))
__global__ __launch_bounds__(64) void lvc_gate_kernel(const float* __restrict__ E, const float* __restrict__ ak, const float* __restrict__ bk,
                                                      const float* __restrict__ Wfc, const float* __restrict__ bfc, float* __restrict__ gam, int C) {
  __shared__ float en[GLS_LVC_MAXC];
  const int b = blockIdx.y;
  for (int c = threadIdx.x; c < C; c += 64) {
    float m = 0.f;
    for (int k = 0; k < GLS_LVC_K; ++k) m += fmaxf(fmaf(ak[k], E[((long)b * GLS_LVC_K + k) * C + c], bk[k]), 0.f);
    en[c] = m * (1.0f / GLS_LVC_K);
  }
  __syncthreads();
  const int co = blockIdx.x * 64 + threadIdx.x;
  if (co >= C) return;
  float v = bfc[co];
  const float* w = Wfc + (long)co * C;
  for (int c = 0; c < C; c += 4) {
    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) v = fmaf(wv[j], en[c + j], v);
  }
  gam[(long)b * C + co] = 1.0f / (1.0f + expf(-v));
}

// ---------------------------------------------------------------- channel fuse
// mode 0: y = relu(a + a * v[img][c])   mode 1: y = a + v[c] * t     fp32 arithmetic (fmaf), one rounding
template <typename T>
__global__ __launch_bounds__(256) void channel_fuse_kernel(const unsigned char* a, long asn, long ash, long asw, const unsigned char* t,
                                                           long tsn, long tsh, long tsw, unsigned char* y, long ysn, long ysh, long ysw,
                                                           const float* __restrict__ v, int n, int H, int W, int cch, int mode) {
  constexpr int VN = 16 / (int)sizeof(T);
  const long total = (long)n * H * W * cch;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int cc = (int)(i % cch);
    long p = i / cch;
    const int w = (int)(p % W);
    p /= W;
    const int h = (int)(p % H), img = (int)(p / H);
    T va[VN];
    *reinterpret_cast<uint4*>(va) = *reinterpret_cast<const uint4*>(a + (img * asn + h * ash + w * asw + cc * VN) * (long)sizeof(T));
    if (mode == 0) {
      const float* g = v + (long)img * cch * VN + cc * VN;
#pragma unroll
      for (int e = 0; e < VN; ++e) va[e] = (T)fmaxf(fmaf((float)va[e], g[e], (float)va[e]), 0.f);
    } else {
      T vt[VN];
      *reinterpret_cast<uint4*>(vt) = *reinterpret_cast<const uint4*>(t + (img * tsn + h * tsh + w * tsw + cc * VN) * (long)sizeof(T));
      const float* g = v + cc * VN;
#pragma unroll
      for (int e = 0; e < VN; ++e) va[e] = (T)fmaf(g[e], (float)vt[e], (float)va[e]);
    }
    *reinterpret_cast<uint4*>(y + (img * ysn + h * ysh + w * ysw + cc * VN) * (long)sizeof(T)) = *reinterpret_cast<uint4*>(va);
  }
}

}  // namespace glsdet

using namespace glsdet;

extern "C" int64_t glsdet_lvc_encode_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t C) {
  if (n < 1 || h < 1 || w < 1 || C < 32 || C % 32 || C > GLS_LVC_MAXC || (long)h * w > GLS_LVC_MAXPIX) return 0;
  int chunk, nsl;
  lvc_slices((long)h * w, &chunk, &nsl);
  const int64_t floats = (int64_t)n * nsl * GLS_LVC_K * ((int64_t)C + 1);
  return (floats * 4 + 255) / 256 * 256;
}

extern "C" int glsdet_lvc_encode(const glsdet_view* x, const float* codewords, const float* scale, void* ws, int64_t ws_bytes,
                                 float* E, void* stream) {
  if (int rc = check_views("lvc_encode: null argument", !codewords || !scale || !ws || !E, {{x, "lvc_encode.x"}})) return rc;
  const int C = x->c;
  if (C < 32 || C % 32 || C > GLS_LVC_MAXC) GLS_FAIL(GLSDET_E_ARG, "lvc_encode: C must be a multiple of 32 in [32, %d], got %d", GLS_LVC_MAXC, C);
  if ((long)x->h * x->w > GLS_LVC_MAXPIX) GLS_FAIL(GLSDET_E_ARG, "lvc_encode: more than 2^24 pixels per image");
  if (x->n > 65535) GLS_FAIL(GLSDET_E_ARG, "lvc_encode: at most 65535 images, got %d", x->n);
  if (((uintptr_t)codewords & 15) || ((uintptr_t)scale & 15) || ((uintptr_t)E & 15))
    GLS_FAIL(GLSDET_E_ALIGN, "lvc_encode: codewords / scale / E must be 16-byte aligned");
  if ((uintptr_t)ws & 255) GLS_FAIL(GLSDET_E_ALIGN, "lvc_encode: workspace must be 256-byte aligned");
  const int64_t need = glsdet_lvc_encode_workspace_bytes(x->n, x->h, x->w, C);
  if (ws_bytes < need) GLS_FAIL(GLSDET_E_ARG, "lvc_encode: workspace of %ld bytes, %ld needed", (long)ws_bytes, (long)need);
  LvcArgs a = {};
  a.x = (const unsigned char*)x->base;
  a.xsn = x->sn; a.xsh = x->sh; a.xsw = x->sw;
  a.cw = codewords; a.scale = scale; a.E = E;
  a.n = x->n; a.H = x->h; a.W = x->w; a.C = C;
  lvc_slices((long)x->h * x->w, &a.chunk, &a.nsl);
  a.Ep = (float*)ws;
  a.Sp = a.Ep + (long)a.n * a.nsl * GLS_LVC_K * C;
  const int dt = x->dtype;
  const double N = (double)x->h * x->w;
  OpRecord op = make_op(4, (double)a.n * 4.0 * N * GLS_LVC_K * C, (double)a.n * (2.0 * N * C * dtype_size(dt) + 4.0 * GLS_LVC_K * C),
                        "lvc_encode(logits+softmax+aggregate, fold)");
  return submit_op(std::move(op), stream, [=](hipStream_t st) {
    const dim3 g1(a.nsl, a.n, (a.C + 63) / 64);
    with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(lvc_encode_kernel<decltype(t)>, g1, dim3(256), 0, st, a); });
    hipLaunchKernelGGL(lvc_fold_kernel, dim3(grid_1d((long)a.n * GLS_LVC_K * (a.C / 4), 4096)), dim3(256), 0, st, a);
  });
}

extern "C" int glsdet_lvc_gate(const float* E, int32_t n, int32_t C, const float* a_k, const float* b_k, const float* fc_w,
                               const float* fc_b, float* gam, void* stream) {
  if (!E || !a_k || !b_k || !fc_w || !fc_b || !gam) GLS_FAIL(GLSDET_E_ARG, "lvc_gate: null argument");
  if (n < 1 || n > 65535) GLS_FAIL(GLSDET_E_ARG, "lvc_gate: 1..65535 images, got %d", n);
  if (C < 32 || C % 32 || C > GLS_LVC_MAXC) GLS_FAIL(GLSDET_E_ARG, "lvc_gate: C must be a multiple of 32 in [32, %d], got %d", GLS_LVC_MAXC, C);
  if (((uintptr_t)E & 15) || ((uintptr_t)fc_w & 15) || ((uintptr_t)gam & 15)) GLS_FAIL(GLSDET_E_ALIGN, "lvc_gate: E / fc_w / gam must be 16-byte aligned");
  OpRecord op = make_op(4, (double)n * (2.0 * C * C + 3.0 * GLS_LVC_K * C), (double)n * 4.0 * (GLS_LVC_K * C + C) + 4.0 * C * C,
                        "lvc_gate(bn1d+relu+mean+fc+sigmoid)");
  return submit_op(std::move(op), stream, [=](hipStream_t st) {
    hipLaunchKernelGGL(lvc_gate_kernel, dim3((C + 63) / 64, n), dim3(64), 0, st, E, a_k, b_k, fc_w, fc_b, gam, C);
  });
}

extern "C" int glsdet_channel_fuse(const glsdet_view* a, const glsdet_view* t, const glsdet_view* y, const float* v, int32_t mode,
                                   void* stream) {
  if (int rc = check_views("channel_fuse: bad argument", !v || mode < 0 || mode > 1 || (mode == 1 && !t), {{a, "channel_fuse.a"}, {y, "channel_fuse.y"}}))
    return rc;
  if (!same_extent(*a, *y) || a->dtype != y->dtype) GLS_FAIL(GLSDET_E_ARG, "channel_fuse: a / y mismatch");
  const int vn = 16 / dtype_size(a->dtype);
  if (a->c % vn) GLS_FAIL(GLSDET_E_ARG, "channel_fuse: channels must be a multiple of %d, got %d", vn, a->c);
  if ((uintptr_t)v & 15) GLS_FAIL(GLSDET_E_ALIGN, "channel_fuse: v must be 16-byte aligned");
  glsdet_view vt = *a;
  if (mode == 1) {
    if (int rc = check_view(*t, "channel_fuse.t")) return rc;
    if (!same_extent(*t, *y) || t->dtype != y->dtype) GLS_FAIL(GLSDET_E_ARG, "channel_fuse: t / y mismatch");
    vt = *t;
  }
  const glsdet_view va = *a, vy = *y;
  const char* name = mode == 0 ? "channel_fuse(relu(a + a * v[n,c]))" : "channel_fuse(a + v[c] * t)";
  return submit_op(make_op(3, 0, (mode == 1 ? 3.0 : 2.0) * va.n * va.h * va.w * va.c * dtype_size(va.dtype), name), stream, [=](hipStream_t st) {
    const unsigned g = grid_1d((long)va.n * va.h * va.w * (va.c / vn));
    with_dtype(va.dtype, [&](auto e) {
      hipLaunchKernelGGL(channel_fuse_kernel<decltype(e)>, dim3(g), dim3(256), 0, st, GLS_VIN(va), GLS_VIN(vt), GLS_VOUT(vy), v, va.n, va.h, va.w, va.c / vn, mode);
    });
  });
}
