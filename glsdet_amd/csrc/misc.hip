// HBM-bound helpers of the forward pass: Focus space-to-depth, SPP max pool, channel max / mean,
// nearest resample / strided copy and transpose.
// All are coalesced 16-byte-per-lane NHWC kernels; none of them is GEMM shaped.
#include <algorithm>
#include <vector>

#include "common.h"

namespace glsdet {

// ---------------------------------------------------------------- Focus space-to-depth
// drone/models/base/darknet.py:15-21 : cat(TL, BL, TR, BR) on channels.
// One thread per output pixel: 2*cin float2 loads (a 2x2 patch of every channel), the
// 16-channel fp16 pixel leaves as two 16-byte stores (fp32: four).
template <typename T>
__global__ __launch_bounds__(256) void focus_pack_kernel(const float* __restrict__ img, int n, int cin, int H, int W,
                                                         unsigned char* y, long sn, long sh, long sw, int cy) {
  const int Ho = H >> 1, Wo = W >> 1;
  const long total = (long)n * Ho * Wo;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const int wo = (int)(p % Wo);
    const int ho = (int)((p / Wo) % Ho);
    const int b = (int)(p / ((long)Wo * Ho));
    T* out = reinterpret_cast<T*>(y) + b * sn + ho * sh + wo * sw;
    if (cin == 3 && cy == 16) {
      float v[16];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* r0 = img + (((long)b * 3 + c) * H + 2 * ho) * W + 2 * wo;
        const float2 t = *reinterpret_cast<const float2*>(r0);          // TL, TR
        const float2 u = *reinterpret_cast<const float2*>(r0 + W);      // BL, BR
        v[0 + c] = t.x;   // TL
        v[3 + c] = u.x;   // BL
        v[6 + c] = t.y;   // TR
        v[9 + c] = u.y;   // BR
      }
      v[12] = v[13] = v[14] = v[15] = 0.f;
      typedef typename Vec16<T>::type V;
      constexpr int VN = Vec16<T>::N;
#pragma unroll
      for (int q = 0; q < 16 / VN; ++q) {
        V pk;
#pragma unroll
        for (int e = 0; e < VN; ++e) pk[e] = (T)v[q * VN + e];
        reinterpret_cast<V*>(out)[q] = pk;
      }
      continue;
    }
    int ch = 0;
    // patch order: (dy,dx) = (0,0) TL, (1,0) BL, (0,1) TR, (1,1) BR
    for (int patch = 0; patch < 4; ++patch) {
      const int dy = patch & 1, dx = patch >> 1;
      for (int c = 0; c < cin; ++c, ++ch)
        out[ch] = (T)img[(((long)b * cin + c) * H + (2 * ho + dy)) * W + (2 * wo + dx)];
    }
    for (; ch < cy; ++ch) out[ch] = (T)0.0f;
  }
}

// ---------------------------------------------------------------- max pool k x k, s1
template <typename T>
__global__ __launch_bounds__(256) void maxpool_kernel(const unsigned char* x, long xsn, long xsh, long xsw,
                                                      unsigned char* y, long ysn, long ysh, long ysw, int n, int H,
                                                      int W, int C, int k) {
  typedef typename Vec16<T>::type V;
  constexpr int VN = Vec16<T>::N;
  const int cchunks = C / VN;
  const long total = (long)n * H * W * cchunks;
  const int r = k / 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % cchunks);
    long p = i / cchunks;
    const int w = (int)(p % W);
    p /= W;
    const int h = (int)(p % H);
    const int b = (int)(p / H);
    V m;
#pragma unroll
    for (int e = 0; e < VN; ++e) m[e] = (T)(-INFINITY);
    for (int dy = -r; dy <= r; ++dy) {
      const int hh = h + dy;
      if (hh < 0 || hh >= H) continue;
      for (int dx = -r; dx <= r; ++dx) {
        const int ww = w + dx;
        if (ww < 0 || ww >= W) continue;
        const V v = *reinterpret_cast<const V*>(x + (b * xsn + hh * xsh + ww * xsw + cc * VN) * (long)sizeof(T));
#pragma unroll
        for (int e = 0; e < VN; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
      }
    }
    *reinterpret_cast<V*>(y + (b * ysn + h * ysh + w * ysw + cc * VN) * (long)sizeof(T)) = m;
  }
}

// ---------------------------------------------------------------- SPP: the 5 / 9 / 13 max pools in one launch
// SPPBottleneck (drone/models/base/darknet.py:29,35): cat(x, pool5(x), pool9(x), pool13(x)).  A stride-1 max pool of 9 is
// pool5 of pool5, 13 is pool5 of pool9 (exact, -inf padding each time): a workgroup takes an 8 x 16 output tile of one
// 16-byte channel chunk, stages the (8+12) x (16+12) input patch in LDS and runs the three pools as separable row / column
// passes on shrinking regions, writing each pool's centre 8 x 16 to its output.  One read of x instead of three chained
// launches each re-reading the previous pool through L2.
template <typename T>
__global__ __launch_bounds__(256) void spp_pools_kernel(const unsigned char* x, long xsn, long xsh, long xsw, unsigned char* y5,
                                                        unsigned char* y9, unsigned char* y13, long ysn, long ysh, long ysw, int H,
                                                        int W, int cchunks, int tiles_x, int tiles_y) {
  typedef typename Vec16<T>::type V;
  constexpr int VN = Vec16<T>::N;
  constexpr int TH = 8, TW = 16, R = 6, PH = TH + 2 * R, PW = TW + 2 * R;
  __shared__ V sA[PH * PW], sB[PH * PW];
  int t = blockIdx.x;
  const int cc = t % cchunks;
  t /= cchunks;
  const int tx = t % tiles_x;
  t /= tiles_x;
  const int ty = t % tiles_y, b = t / tiles_y;
  const int y0 = ty * TH - R, x0 = tx * TW - R;            // image coordinates of patch (0, 0)
  V ninf;
#pragma unroll
  for (int e = 0; e < VN; ++e) ninf[e] = (T)(-INFINITY);
  auto vmax = [](V a, V c) { V r; for (int e = 0; e < VN; ++e) r[e] = a[e] > c[e] ? a[e] : c[e]; return r; };
  for (int q = threadIdx.x; q < PH * PW; q += 256) {
    const int py = q / PW, px = q - py * PW;
    const int h = y0 + py, w = x0 + px;
    V v = ninf;
    if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W)
      v = *reinterpret_cast<const V*>(x + (b * xsn + h * xsh + w * xsw + cc * VN) * (long)sizeof(T));
    sA[q] = v;
  }
  __syncthreads();
  unsigned char* outs[3] = {y5, y9, y13};
#pragma unroll
  for (int stage = 0; stage < 3; ++stage) {
    const int m = 2 * (stage + 1);                          // the valid region shrinks by 2 on every side per pool
    // rows: sB[py][px] = max over px-2..px+2 of sA, for py in [m-2, PH-m+2), px in [m, PW-m)
    for (int q = threadIdx.x; q < PH * PW; q += 256) {
      const int py = q / PW, px = q - py * PW;
      if (py >= m - 2 && py < PH - m + 2 && px >= m && px < PW - m) {
        V v = sA[q - 2];
        v = vmax(v, sA[q - 1]); v = vmax(v, sA[q]); v = vmax(v, sA[q + 1]); v = vmax(v, sA[q + 2]);
        sB[q] = v;
      }
    }
    __syncthreads();
    // columns, and -inf outside the image (the next pool pads with -inf again)
    for (int q = threadIdx.x; q < PH * PW; q += 256) {
      const int py = q / PW, px = q - py * PW;
      if (py >= m && py < PH - m && px >= m && px < PW - m) {
        V v = sB[q - 2 * PW];
        v = vmax(v, sB[q - PW]); v = vmax(v, sB[q]); v = vmax(v, sB[q + PW]); v = vmax(v, sB[q + 2 * PW]);
        const int h = y0 + py, w = x0 + px;
        const bool inside = (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
        sA[q] = inside ? v : ninf;
        if (inside && py >= R && py < R + TH && px >= R && px < R + TW)
          *reinterpret_cast<V*>(outs[stage] + (b * ysn + h * ysh + w * ysw + cc * VN) * (long)sizeof(T)) = v;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- channel max / mean
// SpatialAttention (Non_local_family.py:429-432).  One wave per pixel: lanes stride the
// channel chunks (16 B each), max and sum reduced across the wave with shuffles.
template <typename T>
__global__ __launch_bounds__(256) void channel_maxmean_kernel(const unsigned char* x, long xsn, long xsh, long xsw,
                                                              unsigned char* y, long ysn, long ysh, long ysw, int n,
                                                              int H, int W, int C) {
  typedef typename Vec16<T>::type V;
  constexpr int VN = Vec16<T>::N;
  const int lane = threadIdx.x & 63;
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
  const long total = (long)n * H * W;
  for (long p = wave; p < total; p += nwaves) {
    const int w = (int)(p % W);
    const int h = (int)((p / W) % H);
    const int b = (int)(p / ((long)W * H));
    const unsigned char* px = x + (b * xsn + h * xsh + w * xsw) * (long)sizeof(T);
    float mx = -INFINITY, sm = 0.f;
    for (int c = lane * VN; c < C; c += 64 * VN) {
      const V v = *reinterpret_cast<const V*>(px + c * (long)sizeof(T));
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        const float f = (float)v[e];
        mx = fmaxf(mx, f);
        sm += f;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      sm += __shfl_xor(sm, o, 64);
    }
    if (lane == 0) {
      V out;
#pragma unroll
      for (int e = 0; e < VN; ++e) out[e] = (T)0.f;
      out[0] = (T)mx;
      out[1] = (T)(sm / (float)C);
      T* o = reinterpret_cast<T*>(y) + b * ysn + h * ysh + w * ysw;
      *reinterpret_cast<V*>(o) = out;
      if (VN == 4) {
        V z;
#pragma unroll
        for (int e = 0; e < VN; ++e) z[e] = (T)0.f;
        *reinterpret_cast<V*>(o + 4) = z;
      }
    }
  }
}

// ---------------------------------------------------------------- nearest resample / copy
template <typename T>
__global__ __launch_bounds__(256) void resample_kernel(const unsigned char* x, long xsn, long xsh, long xsw,
                                                       unsigned char* y, long ysn, long ysh, long ysw, int n, int Ho,
                                                       int Wo, int C, int f) {
  constexpr int VN = Vec16<T>::N;
  const int cchunks = C / VN;
  const long total = (long)n * Ho * Wo * cchunks;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % cchunks);
    long p = i / cchunks;
    const int w = (int)(p % Wo);
    p /= Wo;
    const int h = (int)(p % Ho);
    const int b = (int)(p / Ho);
    const uint4 v = *reinterpret_cast<const uint4*>(x + (b * xsn + (h / f) * xsh + (w / f) * xsw + cc * VN) * (long)sizeof(T));
    *reinterpret_cast<uint4*>(y + (b * ysn + h * ysh + w * ysw + cc * VN) * (long)sizeof(T)) = v;
  }
}


// the same strided copy for up to GLS_COPY_JOBS independent (source, destination) pairs of one launch: blockIdx.y = pair
// (the dense per-(image, quadrant) operand copies of the ResNet GL plug-in were 96 launches of 7 us per step)
#define GLS_COPY_JOBS 32
struct CopyJob {
  const unsigned char* x;
  unsigned char* y;
  long xsn, xsh, xsw, ysn, ysh, ysw;
  int n, h, w;
};
struct CopyManyArgs {
  CopyJob j[GLS_COPY_JOBS];
  int C;
};
template <typename T>
__global__ __launch_bounds__(256) void copy_many_kernel(CopyManyArgs a) {
  constexpr int VN = Vec16<T>::N;
  const CopyJob& jb = a.j[blockIdx.y];
  const int cchunks = a.C / VN;
  const long total = (long)jb.n * jb.h * jb.w * cchunks;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % cchunks);
    long p = i / cchunks;
    const int w = (int)(p % jb.w);
    p /= jb.w;
    const int h = (int)(p % jb.h);
    const int b = (int)(p / jb.h);
    const uint4 v = *reinterpret_cast<const uint4*>(jb.x + (b * jb.xsn + h * jb.xsh + w * jb.xsw + cc * VN) * (long)sizeof(T));
    *reinterpret_cast<uint4*>(jb.y + (b * jb.ysn + h * jb.ysh + w * jb.ysw + cc * VN) * (long)sizeof(T)) = v;
  }
}


// transposed form of the same: y[i] is a dense matrix [rows = channels][cols = pixels of x[i]] (row pitch ysw), i.e. the
// `.view(b, c, -1)` operand of the reference's batched matrix products with the pixel index contiguous; 64 pixels x 64 channels per
// workgroup through LDS.  Columns [N, ceil_vec(N)) are written as zeros, later ones are left alone.
template <typename T>
__global__ __launch_bounds__(256) void transpose_many_kernel(CopyManyArgs a) {
  constexpr int VN = Vec16<T>::N;
  constexpr int PITCH = sizeof(T) == 2 ? 66 : 65;      // 33 / 65 words per tile row: the strided reads below hit distinct banks
  __shared__ T tile[64 * PITCH];
  const CopyJob& jb = a.j[blockIdx.z];
  const int N = jb.h * jb.w;
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  if (p0 >= N) return;                                  // whole-workgroup exit, before any barrier
  constexpr int CV = 64 / VN;                           // vectors per pixel row of the tile
  for (int i = threadIdx.x; i < 64 * CV; i += 256) {
    const int px = i / CV, cv = i % CV;
    const int p = p0 + px, c = c0 + cv * VN;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (p < N && c < a.C) v = *reinterpret_cast<const uint4*>(jb.x + ((long)(p / jb.w) * jb.xsh + (long)(p % jb.w) * jb.xsw + c) * (long)sizeof(T));
    const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
    for (int k = 0; k < VN; ++k) tile[px * PITCH + cv * VN + k] = e[k];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * CV; i += 256) {
    const int ch = i / CV, pg = i % CV;
    const int c = c0 + ch, p = p0 + pg * VN;
    if (c >= a.C || p >= N) continue;
    uint4 v;
    T* e = reinterpret_cast<T*>(&v);
#pragma unroll
    for (int k = 0; k < VN; ++k) e[k] = tile[(pg * VN + k) * PITCH + ch];
    *reinterpret_cast<uint4*>(jb.y + ((long)c * jb.ysw + p) * (long)sizeof(T)) = v;
  }
}

}  // namespace glsdet

using namespace glsdet;

extern "C" int glsdet_focus_pack(const float* img, int32_t n, int32_t cin, int32_t H, int32_t W,
                                 const glsdet_view* y, void* stream) {
  if (int rc = check_views("focus_pack: null argument", !img, {{y, "focus_pack.y"}})) return rc;
  if (H % 2 || W % 2 || n < 1 || cin < 1) GLS_FAIL(GLSDET_E_ARG, "focus_pack: H,W must be even");
  if (y->n != n || y->h != H / 2 || y->w != W / 2 || y->c < 4 * cin)
    GLS_FAIL(GLSDET_E_ARG, "focus_pack: output extent mismatch");
  const glsdet_view v = *y;
  const double bytes = (double)n * cin * H * W * 4 + (double)n * (H / 2) * (W / 2) * v.c * dtype_size(v.dtype);
  return submit_op(make_op(1, 0, bytes, "focus_pack"), stream, [=](hipStream_t st) {
    const unsigned g = grid_1d((long)n * (H / 2) * (W / 2));
    with_dtype(v.dtype, [&](auto t) {
      hipLaunchKernelGGL(focus_pack_kernel<decltype(t)>, dim3(g), dim3(256), 0, st, img, n, cin, H, W, GLS_VOUT(v), v.c);
    });
  });
}

extern "C" int glsdet_maxpool2d(const glsdet_view* x, const glsdet_view* y, int32_t k, void* stream) {
  if (int rc = check_views("maxpool2d: null argument", false, {{x, "maxpool2d.x"}, {y, "maxpool2d.y"}})) return rc;
  if (!same_extent(*x, *y) || x->dtype != y->dtype) GLS_FAIL(GLSDET_E_ARG, "maxpool2d: x/y extent or dtype mismatch");
  if (k < 1 || !(k & 1) || k > 31) GLS_FAIL(GLSDET_E_ARG, "maxpool2d: k must be odd in [1,31]");
  if (x->c % 8) GLS_FAIL(GLSDET_E_ARG, "maxpool2d: channels must be a multiple of 8");
  const glsdet_view a = *x, b = *y;
  return submit_op(make_op(2, 0, 2.0 * a.n * a.h * a.w * a.c * dtype_size(a.dtype), "maxpool"), stream, [=](hipStream_t st) {
    const int vn = 16 / dtype_size(a.dtype);
    const unsigned g = grid_1d((long)a.n * a.h * a.w * (a.c / vn));
    with_dtype(a.dtype, [&](auto t) {
      hipLaunchKernelGGL(maxpool_kernel<decltype(t)>, dim3(g), dim3(256), 0, st, GLS_VIN(a), GLS_VOUT(b), a.n, a.h, a.w, a.c, k);
    });
  });
}

extern "C" int glsdet_spp_pools(const glsdet_view* x, const glsdet_view* y5, const glsdet_view* y9, const glsdet_view* y13, void* stream) {
  if (int rc = check_views("spp_pools: null argument", !y5 || !y9 || !y13, {{x, "spp_pools.x"}})) return rc;
  for (const glsdet_view* yi : {y5, y9, y13}) {
    if (int rc = check_view(*yi, "spp_pools.y")) return rc;
    if (!same_extent(*x, *yi) || yi->dtype != x->dtype || yi->sn != y5->sn || yi->sh != y5->sh || yi->sw != y5->sw)
      GLS_FAIL(GLSDET_E_ARG, "spp_pools: outputs must have x's extent and dtype and share one set of strides");
  }
  if (x->c % 8) GLS_FAIL(GLSDET_E_ARG, "spp_pools: channels must be a multiple of 8");
  const glsdet_view a = *x, b5 = *y5, b9 = *y9, b13 = *y13;
  return submit_op(make_op(2, 0, 4.0 * a.n * a.h * a.w * a.c * dtype_size(a.dtype), "spp_pools(5,9,13)"), stream, [=](hipStream_t st) -> int {
    const int vn = 16 / dtype_size(a.dtype);
    const int tiles_x = (a.w + 15) / 16, tiles_y = (a.h + 7) / 8, cch = a.c / vn;
    const long g = (long)a.n * tiles_y * tiles_x * cch;
    if (g <= 0 || g > 0x7fffffffL) GLS_FAIL(GLSDET_E_ARG, "spp_pools: grid out of range");
    with_dtype(a.dtype, [&](auto t) {
      hipLaunchKernelGGL(spp_pools_kernel<decltype(t)>, dim3((unsigned)g), dim3(256), 0, st, GLS_VIN(a), (unsigned char*)b5.base, (unsigned char*)b9.base, (unsigned char*)b13.base, b5.sn, b5.sh, b5.sw, a.h, a.w, cch, tiles_x, tiles_y);
    });
    return 0;
  });
}

extern "C" int glsdet_channel_maxmean(const glsdet_view* x, const glsdet_view* y, void* stream) {
  if (int rc = check_views("channel_maxmean: null argument", false, {{x, "channel_maxmean.x"}, {y, "channel_maxmean.y"}})) return rc;
  if (x->dtype != y->dtype || y->n != x->n || y->h != x->h || y->w != x->w || y->c != 8 || x->c % 8)
    GLS_FAIL(GLSDET_E_ARG, "channel_maxmean: y must be [n,h,w,8] of x's dtype, x.c a multiple of 8");
  const glsdet_view a = *x, b = *y;
  return submit_op(make_op(2, 0, (double)a.n * a.h * a.w * (a.c + 8) * dtype_size(a.dtype), "channel_maxmean"), stream, [=](hipStream_t st) {
    const unsigned g = grid_1d((long)a.n * a.h * a.w * 64);
    with_dtype(a.dtype, [&](auto t) {
      hipLaunchKernelGGL(channel_maxmean_kernel<decltype(t)>, dim3(g), dim3(256), 0, st, GLS_VIN(a), GLS_VOUT(b), a.n, a.h, a.w, a.c);
    });
  });
}

extern "C" int glsdet_resample_copy(const glsdet_view* x, const glsdet_view* y, int32_t factor, void* stream) {
  if (int rc = check_views("resample_copy: null argument", false, {{x, "resample_copy.x"}, {y, "resample_copy.y"}})) return rc;
  if (factor < 1 || factor > 8) GLS_FAIL(GLSDET_E_ARG, "resample_copy: bad factor %d", factor);
  if (x->dtype != y->dtype || y->n != x->n || y->c != x->c || y->h != x->h * factor || y->w != x->w * factor)
    GLS_FAIL(GLSDET_E_ARG, "resample_copy: extent mismatch");
  if (x->c % 8) GLS_FAIL(GLSDET_E_ARG, "resample_copy: channels must be a multiple of 8");
  const glsdet_view a = *x, b = *y;
  const double bytes = ((double)a.n * a.h * a.w + (double)b.n * b.h * b.w) * a.c * dtype_size(a.dtype);
  return submit_op(make_op(3, 0, bytes, factor == 1 ? "copy" : "upsample_nearest"), stream, [=](hipStream_t st) {
    const int vn = 16 / dtype_size(a.dtype);
    const unsigned g = grid_1d((long)b.n * b.h * b.w * (b.c / vn));
    with_dtype(a.dtype, [&](auto t) {
      hipLaunchKernelGGL(resample_kernel<decltype(t)>, dim3(g), dim3(256), 0, st, GLS_VIN(a), GLS_VOUT(b), b.n, b.h, b.w, b.c, factor);
    });
  });
}

// the (source, destination) pair i of copy_many / transpose_many as the kernels take it
static CopyJob copy_job(const glsdet_view& x, const glsdet_view& y) {
  CopyJob j;
  j.x = (const unsigned char*)x.base;
  j.y = (unsigned char*)y.base;
  j.xsn = x.sn, j.xsh = x.sh, j.xsw = x.sw, j.ysn = y.sn, j.ysh = y.sh, j.ysw = y.sw;
  j.n = x.n, j.h = x.h, j.w = x.w;
  return j;
}

extern "C" int glsdet_copy_many(const glsdet_view* x, const glsdet_view* y, int32_t count, void* stream) {
  if (!x || !y) GLS_FAIL(GLSDET_E_ARG, "copy_many: null argument");
  if (count < 1 || count > 4096) GLS_FAIL(GLSDET_E_ARG, "copy_many: 1..4096 pairs, got %d", count);
  std::vector<CopyJob> jobs((size_t)count);
  double bytes = 0;
  for (int i = 0; i < count; ++i) {
    if (int rc = check_view(x[i], "copy_many.x")) return rc;
    if (int rc = check_view(y[i], "copy_many.y")) return rc;
    if (x[i].dtype != x[0].dtype || y[i].dtype != x[0].dtype || x[i].c != x[0].c || y[i].c != x[0].c)
      GLS_FAIL(GLSDET_E_ARG, "copy_many: pair %d: one dtype and one channel count per call", i);
    if (x[i].n != y[i].n || x[i].h != y[i].h || x[i].w != y[i].w) GLS_FAIL(GLSDET_E_ARG, "copy_many: pair %d: extent mismatch", i);
    jobs[(size_t)i] = copy_job(x[i], y[i]);
    bytes += 2.0 * ((long)x[i].n * x[i].h * x[i].w) * x[i].c * dtype_size(x[i].dtype);
  }
  if (x[0].c % 8) GLS_FAIL(GLSDET_E_ARG, "copy_many: channels must be a multiple of 8");
  const int C = x[0].c, dt = x[0].dtype;
  return submit_op(make_op(3, 0, bytes, "copy_many[" + std::to_string(count) + "]"), stream, [=](hipStream_t st) -> int {
    const int vn = 16 / dtype_size(dt);
    // the pairs share the chip: about four workgroups per CU over one launch, at least one per pair
    for (int j0 = 0; j0 < count; j0 += GLS_COPY_JOBS) {
      const int nj = std::min(GLS_COPY_JOBS, count - j0);
      CopyManyArgs a = {};
      long big = 0;
      for (int i = 0; i < nj; ++i) {
        a.j[i] = jobs[(size_t)(j0 + i)];
        big = std::max(big, (long)a.j[i].n * a.j[i].h * a.j[i].w * (C / vn));
      }
      a.C = C;
      const unsigned per = grid_1d(big, std::max(1, 2048 / nj));
      with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(copy_many_kernel<decltype(t)>, dim3(per, nj), dim3(256), 0, st, a); });
      GLS_HIP(hipGetLastError());
    }
    return 0;
  });
}

extern "C" int glsdet_transpose_many(const glsdet_view* x, const glsdet_view* y, int32_t count, void* stream) {
  if (!x || !y) GLS_FAIL(GLSDET_E_ARG, "transpose_many: null argument");
  if (count < 1 || count > 4096) GLS_FAIL(GLSDET_E_ARG, "transpose_many: 1..4096 pairs, got %d", count);
  std::vector<CopyJob> jobs((size_t)count);
  double bytes = 0;
  for (int i = 0; i < count; ++i) {
    if (int rc = check_view(x[i], "transpose_many.x")) return rc;
    if (int rc = check_view(y[i], "transpose_many.y")) return rc;
    if (x[i].dtype != x[0].dtype || y[i].dtype != x[0].dtype || x[i].c != x[0].c)
      GLS_FAIL(GLSDET_E_ARG, "transpose_many: pair %d: one dtype and one channel count per call", i);
    const int vn = 16 / dtype_size(x[i].dtype);
    const long N = (long)x[i].h * x[i].w;
    if (x[i].n != 1 || y[i].n != 1 || y[i].h != 1) GLS_FAIL(GLSDET_E_ARG, "transpose_many: pair %d: one image -> one matrix [1,1,rows,cols]", i);
    if (y[i].w < x[i].c || y[i].c < (N + vn - 1) / vn * vn)
      GLS_FAIL(GLSDET_E_ARG, "transpose_many: pair %d: matrix %d x %d too small for %d channels x %ld pixels", i, y[i].w, y[i].c, x[i].c, N);
    jobs[(size_t)i] = copy_job(x[i], y[i]);
    bytes += 2.0 * N * x[i].c * dtype_size(x[i].dtype);
  }
  if (x[0].c % 8) GLS_FAIL(GLSDET_E_ARG, "transpose_many: channels must be a multiple of 8");
  const int C = x[0].c, dt = x[0].dtype;
  return submit_op(make_op(3, 0, bytes, "transpose_many[" + std::to_string(count) + "]"), stream, [=](hipStream_t st) -> int {
    for (int j0 = 0; j0 < count; j0 += GLS_COPY_JOBS) {
      const int nj = std::min(GLS_COPY_JOBS, count - j0);
      CopyManyArgs a = {};
      long big = 0;
      for (int i = 0; i < nj; ++i) {
        a.j[i] = jobs[(size_t)(j0 + i)];
        big = std::max(big, (long)a.j[i].h * a.j[i].w);
      }
      a.C = C;
      const dim3 grid((unsigned)((big + 63) / 64), (unsigned)((C + 63) / 64), (unsigned)nj);
      with_dtype(dt, [&](auto t) { hipLaunchKernelGGL(transpose_many_kernel<decltype(t)>, grid, dim3(256), 0, st, a); });
      GLS_HIP(hipGetLastError());
    }
    return 0;
  });
}
