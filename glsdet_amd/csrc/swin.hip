// The three steps of the reference's Swin trunk (ufp/mmdet/models/backbones/swin.py, ufp/mmdet/models/utils/transformer.py)
// that are no convolution:
//   glsdet_layernorm         nn.LayerNorm over the channels of every token (norm1 / norm2 / norm{i} / the merge and embed norms)
//   glsdet_window_attention  ShiftWindowMSA.forward + WindowMSA.forward (swin.py:80-118, 179-253) between the qkv and the
//                            proj linear, on the matrix cores
//   glsdet_patch_merge       AdaptivePadding('corner') + nn.Unfold(2, stride 2) of PatchMerging.forward (transformer.py)
//
// LayerNorm: one wave per token, the row read three times (it is at most 16 KiB and stays in the L1 / L2): lane l owns the
// 4-channel chunks l, l + 64, ...; fp32 throughout, TWO passes:
//   s    = sum of the lane's elements, chunks ascending, inside a chunk ((v0 + v1) + (v2 + v3)); xor butterfly 32, 16, .. 1
//   mean = s / C;  var = (the same sum over (v - mean)^2) / C;  rstd = 1 / sqrtf(var + eps)
//   y    = ((v - mean) * rstd) * gamma + beta, rounded once to the output type
//
// Window attention: a work item is (image, window of the padded map, head); workgroup b takes the items b, b + grid, ...
// (grid = min(items, GLS_WIN_MAXGRID)).  128 threads = 2 waves; wave w owns the query rows 32 w .. 32 w + 31 of the window's
// N = ws * ws <= 64 tokens.  Padding the map to a multiple of ws, the cyclic roll by -shift, the partition and its reverse are
// index arithmetic: token t = (ty, tx) of window (wy, wx) sits at (sy, sx) = (wy ws + ty, wx ws + tx) of the SHIFTED padded
// map, which is pixel ((sy + shift) mod Hp, (sx + shift) mod Wp) of the padded map.  A pixel outside H x W is a padded token:
// its q, k, v are the qkv bias (rounded to the storage type, as the linear would have stored it), it takes full part in the
// softmax, and its output row is dropped.
//   q~      = q * scale                                          one fp32 rounding, before the product (swin.py:94)
//   S[i][j] = sum_d q~[i][d] k[j][d]                             v_mfma_f32_32x32x2_f32, d ascending: an fmaf chain
//   S      += table[(ty_i - ty_j + ws - 1)(2 ws - 1) + (tx_i - tx_j + ws - 1)][head]      relative_position_index restated
//   S      += -100 where region(i) != region(j)   (shift > 0)    region = 3 rh + rw, rh = 0 / 1 / 2 for sy < Hp - ws /
//                                                                sy < Hp - shift / the rest (swin.py:199-219)
//   P[i][j] = expf(S - max_j S) / sum_j                          over the N real columns only: columns N .. 63 of the 64-wide
//                                                                tile are EXCLUDED (weight 0 by construction, not by a mask);
//                                                                two lanes per row, 32 columns each, sum = q_lo + q_hi
//   O[i][d] = sum_j P[i][j] v[j][d]                              the same MFMA, j ascending
// Both storage types run the fp32 MFMA on fp32 images of q, k, v in LDS: P never leaves fp32.
// LDS 43.4 KiB (q, k, v as [64][33], S / P as [64][65], the token table), no scratch, two 16-register accumulators.
#include "mfma_tile.h"

#include <cmath>

namespace glsdet {

#define GLS_LN_MAXC 4096
#define GLS_LN_MAXGRID 4096      // workgroups of 4 tokens
#define GLS_WIN_MAXC 1024
#define GLS_WIN_MAXGRID 4096     // workgroups of one (window, head) item at a time

struct LnArgs {
  const unsigned char* x;
  long xsn, xsh, xsw;
  unsigned char* y;
  long ysn, ysh, ysw;
  const float *gamma, *beta;
  float eps;
  int H, W, C;
  long tokens;
};

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

template <typename T>
__device__ __forceinline__ f32x4 load4(const T* p);
template <>
__device__ __forceinline__ f32x4 load4<float>(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
template <>
__device__ __forceinline__ f32x4 load4<f16>(const f16* p) {
  const f16x4 v = *reinterpret_cast<const f16x4*>(p);
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ void store4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void store4(f16* p, f32x4 v) {
  *reinterpret_cast<f16x4*>(p) = f16x4{(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void layernorm_kernel(const LnArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = a.C >> 2;
  const float invc = (float)a.C;
  for (long t = (long)blockIdx.x * 4 + wave; t < a.tokens; t += (long)gridDim.x * 4) {
    const int w = (int)(t % a.W);
    const long r = t / a.W;
    const int h = (int)(r % a.H);
    const long img = r / a.H;
    const TI* xp = reinterpret_cast<const TI*>(a.x) + img * a.xsn + h * a.xsh + w * a.xsw;
    TO* yp = reinterpret_cast<TO*>(a.y) + img * a.ysn + h * a.ysh + w * a.ysw;
    float s = 0.f;
    for (int c = lane; c < nch; c += 64) {
      const f32x4 v = load4<TI>(xp + 4 * c);
      s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    const float mean = wave_sum(s) / invc;
    float q = 0.f;
    for (int c = lane; c < nch; c += 64) {
      const f32x4 v = load4<TI>(xp + 4 * c);
      const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
      q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    const float var = wave_sum(q) / invc;
    const float rstd = 1.0f / sqrtf(var + a.eps);
    for (int c = lane; c < nch; c += 64) {
      const f32x4 v = load4<TI>(xp + 4 * c);
      const f32x4 g = *reinterpret_cast<const f32x4*>(a.gamma + 4 * c);
      const f32x4 b = *reinterpret_cast<const f32x4*>(a.beta + 4 * c);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = ((v[e] - mean) * rstd) * g[e] + b[e];
      store4(yp + 4 * c, o);
    }
  }
}

// ---------------------------------------------------------------- patch merge
// y[n, oh, ow, 4 c + 2 kh + kw] = x[n, 2 oh + kh, 2 ow + kw, c], zero past H / W: one thread per (pixel, c), one 4-element store
template <typename T>
__global__ __launch_bounds__(256) void patch_merge_kernel(const unsigned char* x, long xsn, long xsh, long xsw, unsigned char* y,
                                                          long ysn, long ysh, long ysw, int n, int H, int W, int C, int Ho, int Wo) {
  const long total = (long)n * Ho * Wo * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    long p = i / C;
    const int ow = (int)(p % Wo);
    p /= Wo;
    const int oh = (int)(p % Ho);
    const long img = p / Ho;
    const T* xb = reinterpret_cast<const T*>(x) + img * xsn + c;
    T o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int yy = 2 * oh + (k >> 1), xx = 2 * ow + (k & 1);
      o[k] = (yy < H && xx < W) ? xb[yy * xsh + xx * xsw] : (T)0.f;
    }
    T* yp = reinterpret_cast<T*>(y) + img * ysn + oh * ysh + ow * ysw + 4 * c;
    if (sizeof(T) == 2)
      *reinterpret_cast<uint2*>(yp) = *reinterpret_cast<uint2*>(o);
    else
      *reinterpret_cast<uint4*>(yp) = *reinterpret_cast<uint4*>(o);
  }
}

// ---------------------------------------------------------------- window attention
struct WinArgs {
  const unsigned char* x;
  long xsn, xsh, xsw;
  unsigned char* y;
  long ysn, ysh, ysw;
  const float *table, *qb;
  float scale;
  int n, H, W, C, heads, ws, shift, nwh, nww;
  long items;
};

template <typename T>
__global__ __launch_bounds__(128) void window_attention_kernel(const WinArgs a) {
  constexpr int VN = Vec16<T>::N;
  constexpr int CPR = 32 / VN;                  // 16-byte chunks of one head of one token
  constexpr int LDQ = 33, LDP = 65;
  typedef typename Vec16<T>::type V;
  __shared__ float qkv_s[3 * 64 * LDQ];         // q~ | k | v as [token][33]
  __shared__ float ss[64 * LDP];                // S, then P: [query][key]
  __shared__ int tpy[64], tpx[64], tty[64], ttx[64], treg[64];      // source pixel (-1: padded), window coordinates, region
  float* qs = qkv_s;
  float* ks = qkv_s + 64 * LDQ;
  float* vs = qkv_s + 2 * 64 * LDQ;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  const int wm = wave * 32;
  const int ws = a.ws, N = ws * ws, C = a.C, heads = a.heads;
  const int Hp = a.nwh * ws, Wp = a.nww * ws;
  for (long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const int head = (int)(item % heads);
    long wq = item / heads;
    const int wx = (int)(wq % a.nww);
    wq /= a.nww;
    const int wy = (int)(wq % a.nwh);
    const long img = wq / a.nwh;
    if (tid < 64) {
      int py = -1, px = 0, ty = 0, tx = 0, reg = 0;
      if (tid < N) {
        ty = tid / ws;
        tx = tid - ty * ws;
        const int sy = wy * ws + ty, sx = wx * ws + tx;
        int yy = sy + a.shift, xx = sx + a.shift;
        if (yy >= Hp) yy -= Hp;
        if (xx >= Wp) xx -= Wp;
        if (yy < a.H && xx < a.W) {
          py = yy;
          px = xx;
        }
        if (a.shift > 0) {
          const int rh = sy < Hp - ws ? 0 : (sy < Hp - a.shift ? 1 : 2);
          const int rw = sx < Wp - ws ? 0 : (sx < Wp - a.shift ? 1 : 2);
          reg = 3 * rh + rw;
        }
      }
      tpy[tid] = py; tpx[tid] = px; tty[tid] = ty; ttx[tid] = tx; treg[tid] = reg;
    }
    __syncthreads();
    // ---- q~, k, v of this head into LDS as fp32; rows N .. 63 are zero
    const T* xb = reinterpret_cast<const T*>(a.x) + img * a.xsn;
    for (int t = tid; t < 3 * 64 * CPR; t += 128) {
      const int m = t / (64 * CPR), rem = t - m * (64 * CPR);
      const int r = rem / CPR, ch = rem - r * CPR;
      const int col = m * C + head * 32 + ch * VN;
      float f[VN];
#pragma unroll
      for (int e = 0; e < VN; ++e) f[e] = 0.f;
      if (r < N) {
        if (tpy[r] >= 0) {
          const V v = *reinterpret_cast<const V*>(xb + (long)tpy[r] * a.xsh + (long)tpx[r] * a.xsw + col);
#pragma unroll
          for (int e = 0; e < VN; ++e) f[e] = (float)v[e];
        } else if (a.qb) {
#pragma unroll
          for (int e = 0; e < VN; ++e) f[e] = (float)(T)a.qb[col + e];
        }
      }
      float* dst = qkv_s + (m * 64 + r) * LDQ + ch * VN;
      if (m == 0) {
#pragma unroll
        for (int e = 0; e < VN; ++e) dst[e] = f[e] * a.scale;
      } else {
#pragma unroll
        for (int e = 0; e < VN; ++e) dst[e] = f[e];
      }
    }
    __syncthreads();
    const bool live = wm < N;                   // wave-uniform: wave 1 idles on windows of at most 32 tokens
    if (live) {
      // ---- S = q~ k^T: rows wm .. wm + 31, key columns 0 .. 31 and (N > 32) 32 .. 63
      f32x16 acc0, acc1;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
      const float* pa = qs + (wm + l31) * LDQ + hi;
      const float* pb0 = ks + l31 * LDQ + hi;
      const float* pb1 = ks + (32 + l31) * LDQ + hi;
      acc0 = mfma32_f32<16, 2, 2>(pa, pb0, acc0);
      if (N > 32) acc1 = mfma32_f32<16, 2, 2>(pa, pb1, acc1);
      const int span = 2 * ws - 1;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = wm + mfma32_row(r, lane);
        if (i < N) {
          const int iy = tty[i] + ws - 1, ix = ttx[i] + ws - 1, ir = treg[i];
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const int j = half * 32 + l31;
            if (j < N) {
              float s = (half ? acc1[r] : acc0[r]) + a.table[(long)((iy - tty[j]) * span + (ix - ttx[j])) * heads + head];
              if (ir != treg[j]) s += -100.f;
              ss[i * LDP + j] = s;
            }
          }
        }
      }
    }
    __syncthreads();
    if (live) {
      // ---- softmax of row wm + lane / 2 over its N columns: two lanes, 32 columns each
      const int i = wm + (lane >> 1), j0 = (lane & 1) * 32;
      float* row = ss + i * LDP;
      if (i < N) {
        const int j1 = min(N, j0 + 32);
        float m = -INFINITY;
        for (int j = j0; j < j1; ++j) m = fmaxf(m, row[j]);
        m = fmaxf(m, __shfl_xor(m, 1, 64));
        float q = 0.f;
        for (int j = j0; j < j1; ++j) {
          const float e = expf(row[j] - m);
          row[j] = e;
          q += e;
        }
        const float tot = __shfl(q, lane & ~1, 64) + __shfl(q, lane | 1, 64);
        for (int j = j0; j < j0 + 32; ++j) row[j] = j < j1 ? row[j] / tot : 0.f;
      } else {
        // (the shuffles above are reached by both lanes of a row or by neither)
        for (int j = j0; j < j0 + 32; ++j) row[j] = 0.f;
      }
    }
    __syncthreads();
    if (live) {
      // ---- O = P v over the N keys (P's columns and v's rows past N are zero; an odd N takes one of them along)
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const float* pa = ss + (wm + l31) * LDP + hi;
      const float* pb = vs + hi * LDQ + l31;
      const int steps = (N + 1) >> 1;
      for (int s = 0; s < steps; ++s) acc = mfma32_f32<1, 2, 2 * LDQ>(pa + 2 * s, pb + 2 * s * LDQ, acc);
      T* yb = reinterpret_cast<T*>(a.y) + img * a.ysn + head * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = wm + mfma32_row(r, lane);
        if (i < N && tpy[i] >= 0) yb[(long)tpy[i] * a.ysh + (long)tpx[i] * a.ysw] = (T)acc[r];
      }
    }
    __syncthreads();
  }
}

}  // namespace glsdet

using namespace glsdet;

extern "C" int glsdet_layernorm(const glsdet_view* x, const glsdet_view* y, const float* gamma, const float* beta, float eps,
                                void* stream) {
  if (int rc = check_views("layernorm: null argument", !gamma || !beta, {{x, "layernorm.x"}, {y, "layernorm.y"}})) return rc;
  if (!same_extent(*x, *y)) GLS_FAIL(GLSDET_E_ARG, "layernorm: x / y extents differ");
  const int C = x->c;
  if (C < 32 || C % 32 || C > GLS_LN_MAXC) GLS_FAIL(GLSDET_E_ARG, "layernorm: C must be a multiple of 32 in [32, %d], got %d", GLS_LN_MAXC, C);
  // in place (the same view) is safe: a lane writes a chunk after its own last read of it.  Any other overlap is not.
  const bool same_view = x->base == y->base && x->dtype == y->dtype && x->sn == y->sn && x->sh == y->sh && x->sw == y->sw;
  if (!same_view && views_overlap(*x, *y)) GLS_FAIL(GLSDET_E_ARG, "layernorm: y overlaps x without being the same view");
  if (!(eps >= 0.f) || !std::isfinite(eps)) GLS_FAIL(GLSDET_E_ARG, "layernorm: eps must be finite and not negative");
  if (((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15)) GLS_FAIL(GLSDET_E_ALIGN, "layernorm: gamma / beta must be 16-byte aligned");
  LnArgs a = {};
  a.x = (const unsigned char*)x->base; a.xsn = x->sn; a.xsh = x->sh; a.xsw = x->sw;
  a.y = (unsigned char*)y->base; a.ysn = y->sn; a.ysh = y->sh; a.ysw = y->sw;
  a.gamma = gamma; a.beta = beta; a.eps = eps;
  a.H = x->h; a.W = x->w; a.C = C;
  a.tokens = (long)x->n * x->h * x->w;
  const int di = x->dtype, dout = y->dtype;
  OpRecord op = make_op(3, 8.0 * a.tokens * C, (double)a.tokens * C * (dtype_size(di) + dtype_size(dout)) + 8.0 * C,
                        "layernorm(two-pass fp32, one wave per token)");
  return submit_op(std::move(op), stream, [=](hipStream_t st) {
    long g = (a.tokens + 3) / 4;      // workgroups of 4 tokens, not of 256 items: written out
    if (g > GLS_LN_MAXGRID) g = GLS_LN_MAXGRID;
    const dim3 grid((unsigned)g), block(256);
    with_dtype(di, [&](auto ti) {
      with_dtype(dout, [&](auto to) { hipLaunchKernelGGL((layernorm_kernel<decltype(ti), decltype(to)>), grid, block, 0, st, a); });
    });
  });
}

extern "C" int glsdet_patch_merge(const glsdet_view* x, const glsdet_view* y, void* stream) {
  if (int rc = check_views("patch_merge: null argument", false, {{x, "patch_merge.x"}, {y, "patch_merge.y"}})) return rc;
  if (x->dtype != y->dtype) GLS_FAIL(GLSDET_E_ARG, "patch_merge: x / y dtypes differ");
  if (views_overlap(*x, *y)) GLS_FAIL(GLSDET_E_ARG, "patch_merge: y overlaps x");
  if (x->c % 8) GLS_FAIL(GLSDET_E_ARG, "patch_merge: channels must be a multiple of 8, got %d", x->c);
  if (y->n != x->n || y->h != (x->h + 1) / 2 || y->w != (x->w + 1) / 2 || (long)y->c != 4L * x->c)
    GLS_FAIL(GLSDET_E_ARG, "patch_merge: y must be [%d,%d,%d,%ld], got [%d,%d,%d,%d]", x->n, (x->h + 1) / 2, (x->w + 1) / 2,
             4L * x->c, y->n, y->h, y->w, y->c);
  const glsdet_view vx = *x, vy = *y;
  const double bytes = ((double)vx.n * vx.h * vx.w * vx.c + (double)vy.n * vy.h * vy.w * vy.c) * dtype_size(vx.dtype);
  return submit_op(make_op(3, 0, bytes, "patch_merge(pad + unfold 2x2 / 2)"), stream, [=](hipStream_t st) {
    const unsigned g = grid_1d((long)vy.n * vy.h * vy.w * vx.c);
    with_dtype(vx.dtype, [&](auto t) {
      hipLaunchKernelGGL(patch_merge_kernel<decltype(t)>, dim3(g), dim3(256), 0, st, GLS_VIN(vx), GLS_VOUT(vy), vx.n, vx.h, vx.w, vx.c, vy.h, vy.w);
    });
  });
}

extern "C" int glsdet_window_attention(const glsdet_view* qkv, const glsdet_view* y, const float* bias_table, const float* qkv_bias,
                                       int32_t heads, int32_t ws, int32_t shift, float scale, void* stream) {
  if (int rc = check_views("window_attention: null argument", !bias_table, {{qkv, "window_attention.qkv"}, {y, "window_attention.y"}})) return rc;
  if (qkv->dtype != y->dtype) GLS_FAIL(GLSDET_E_ARG, "window_attention: qkv / y dtypes differ");
  const int C = y->c;
  if (C < 32 || C % 32 || C > GLS_WIN_MAXC)
    GLS_FAIL(GLSDET_E_ARG, "window_attention: C must be a multiple of 32 in [32, %d], got %d", GLS_WIN_MAXC, C);
  if (qkv->n != y->n || qkv->h != y->h || qkv->w != y->w || (long)qkv->c != 3L * C)
    GLS_FAIL(GLSDET_E_ARG, "window_attention: qkv must be [%d,%d,%d,%d], got [%d,%d,%d,%d]", y->n, y->h, y->w, 3 * C, qkv->n, qkv->h,
             qkv->w, qkv->c);
  if (views_overlap(*qkv, *y)) GLS_FAIL(GLSDET_E_ARG, "window_attention: y overlaps qkv (a window would read what another wrote)");
  if (heads < 1 || (long)heads * 32 != C)
    GLS_FAIL(GLSDET_E_ARG, "window_attention: head_dim must be 32 (C = %d asks for %d heads, got %d)", C, C / 32, heads);
  if (ws < 2 || ws > 8) GLS_FAIL(GLSDET_E_ARG, "window_attention: window_size must lie in 2..8, got %d", ws);
  if (shift < 0 || shift >= ws) GLS_FAIL(GLSDET_E_ARG, "window_attention: shift must lie in 0..%d, got %d", ws - 1, shift);
  if (!std::isfinite(scale)) GLS_FAIL(GLSDET_E_ARG, "window_attention: scale must be finite");
  if (((uintptr_t)bias_table & 3) || ((uintptr_t)qkv_bias & 3)) GLS_FAIL(GLSDET_E_ALIGN, "window_attention: bias_table / qkv_bias must be 4-byte aligned");
  WinArgs a = {};
  a.x = (const unsigned char*)qkv->base; a.xsn = qkv->sn; a.xsh = qkv->sh; a.xsw = qkv->sw;
  a.y = (unsigned char*)y->base; a.ysn = y->sn; a.ysh = y->sh; a.ysw = y->sw;
  a.table = bias_table; a.qb = qkv_bias; a.scale = scale;
  a.n = y->n; a.H = y->h; a.W = y->w; a.C = C; a.heads = heads; a.ws = ws; a.shift = shift;
  a.nwh = (y->h + ws - 1) / ws;
  a.nww = (y->w + ws - 1) / ws;
  a.items = (long)a.n * a.nwh * a.nww * heads;
  const int dt = y->dtype;
  const double N = (double)ws * ws;
  OpRecord op = make_op(4, (double)a.items * 4.0 * N * N * 32, (double)a.n * a.H * a.W * 4.0 * C * dtype_size(dt),
                        "window_attention(qk^T + bias + mask, softmax, pv)");
  return submit_op(std::move(op), stream, [=](hipStream_t st) {
    const long g = a.items < GLS_WIN_MAXGRID ? a.items : GLS_WIN_MAXGRID;      // one item per workgroup of 128: written out
    with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(window_attention_kernel<decltype(t)>, dim3((unsigned)g), dim3(128), 0, st, a); });
  });
}
