// The non-local block of glsdet_nonlocal_multi on the matrix cores, for wide blocks (ci a multiple of 32 up to 1280):
// new/yolox10.py:236-266 runs Patch_Conv_NonLocal_new on dark3 / dark4 / dark5 with inter_channels = C
// (Non_local_family.py:32-48): about 36 GFLOP per 8x800x1344 batch of YOLOX-s, on loops that nonlocal.hip sized for ci = 64.
// DESIGN section 5 has the measured times of both kernel families; Engine picks per geometry from them.
//
// Same association (nonlocal_common.h), same slice rule, same workspace layout and the same determinism as nonlocal.hip.
// No atomics; a replay reproduces the bits.  No new rounding: theta / phi / g are read in the storage type, G, P, Wout and
// bout are fp32.  The fp16 Gram runs on v_mfma_f32_32x32x16_f16, everything else on v_mfma_f32_32x32x2_f32 (mfma_tile.h
// has the lane maps): only the order of the sums differs from nonlocal.hip.
//
// Every kernel: 256 threads = 2 x 2 waves, a wave owns one 32 x 32 accumulator tile of the workgroup's 64 x 64 tile; a wave
// whose tile lies past a 32-multiple extent skips its MFMAs (wave-uniform) and its stores, never a barrier.
#include <algorithm>

#include "mfma_tile.h"
#include "nonlocal_common.h"

namespace glsdet {

#define GLS_NLM_MAXC 1280

// ---------------------------------------------------------------- Gram
// grid (tiles(c1) * tiles(c2), image, 8 * set + slice).  tpg is pixel-major, so K (the pixels) is outermost in memory:
// fp32 stages [pixel][64 channels] as it lies (the 32x32x2 operands are one row of it per lane half); fp16 stages the
// transposed image [channel][64 pixels + 8] so that a lane's 8 k-elements are one 16-byte read.
template <typename T>
__global__ __launch_bounds__(256) void nlm_gram_kernel(const NlmArgs a) {
  constexpr bool H16 = sizeof(T) == 2;
  constexpr int PX = H16 ? 64 : 32;                 // pixels per stage
  constexpr int LDH = PX + 8;                       // fp16 image: halves per channel row (144 B: 16-byte aligned rows)
  constexpr int VN = Vec16<T>::N, CPP = 64 / VN;    // 16-byte chunks per pixel and matrix
  typedef typename Vec16<T>::type V;
  __shared__ __attribute__((aligned(16))) unsigned char smem[H16 ? 2 * 64 * LDH * 2 : 2 * PX * 64 * 4];
  const int q = blockIdx.z >> 3, z = blockIdx.z & 7;
  const NlSet& S = a.s[q];
  if (z >= S.nsplit) return;                        // whole workgroup, before any barrier
  const int ci = a.ci, nb = (ci + 63) / 64;
  const int c1_0 = (blockIdx.x / nb) * 64, c2_0 = (blockIdx.x % nb) * 64;
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hi = lane >> 5;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const bool active = c1_0 + wm < ci && c2_0 + wn < ci;
  const int W = S.W, N = S.H * W;
  const int jbeg = z * S.jchunk, jend = min(N, jbeg + S.jchunk);
  const T* base = reinterpret_cast<const T*>(S.tpg) + b * S.tsn;
  f32x16 acc = mfma32_zero();
  for (int j0 = jbeg; j0 < jend; j0 += PX) {
    for (int t = threadIdx.x; t < 2 * PX * CPP; t += 256) {
      const int mat = t / (PX * CPP), r = t - mat * PX * CPP;
      const int jj = r / CPP, ch = r - jj * CPP;
      const int j = j0 + jj, c = (mat ? c2_0 : c1_0) + ch * VN;
      V v;
#pragma unroll
      for (int k = 0; k < VN; ++k) v[k] = (T)0.f;
      if (j < jend && c < ci)
        v = *reinterpret_cast<const V*>(base + (long)(j / W) * S.tsh + (long)(j % W) * S.tsw + (mat ? 2 * ci : ci) + c);
      if constexpr (H16) {
        f16* dst = reinterpret_cast<f16*>(smem) + mat * 64 * LDH;
#pragma unroll
        for (int k = 0; k < VN; ++k) dst[(ch * VN + k) * LDH + jj] = v[k];
      } else {
        *reinterpret_cast<V*>(reinterpret_cast<float*>(smem) + mat * PX * 64 + jj * 64 + ch * VN) = v;
      }
    }
    __syncthreads();
    if (active) {
      if constexpr (H16) {
        const f16* ph = reinterpret_cast<const f16*>(smem) + (wm + l31) * LDH + 8 * hi;
        const f16* gg = reinterpret_cast<const f16*>(smem) + 64 * LDH + (wn + l31) * LDH + 8 * hi;
        acc = mfma32_f16<PX / 16>(ph, gg, acc);
      } else {
        const float* ph = reinterpret_cast<const float*>(smem) + hi * 64 + wm + l31;
        const float* gg = reinterpret_cast<const float*>(smem) + PX * 64 + hi * 64 + wn + l31;
        acc = mfma32_f32<PX / 2, 128, 128>(ph, gg, acc);
      }
    }
    __syncthreads();
  }
  if (active) {
    float* G = S.gram + (((long)z * a.nimg + b) * ci + c1_0 + wm) * ci + c2_0 + wn + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) G[(long)mfma32_row(r, lane) * ci] = acc[r];
  }
}

// ---------------------------------------------------------------- fold
// grid (image + nimg * set, tiles(co), tiles(c1)).  A = Wout [co][c2], B = summed Gram read as [c2][c1]: both staged as
// [row][64 + 1] so that the lanes' reads of one k column hit distinct banks.
#define GLS_NLM_KC 64
__global__ __launch_bounds__(256) void nlm_fold_kernel(const NlmArgs a) {
  constexpr int LD = GLS_NLM_KC + 1;
  __shared__ float wsm[64 * LD], gs[64 * LD];
  const int q = blockIdx.x / a.nimg, b = blockIdx.x - q * a.nimg;
  const NlSet& S = a.s[q];
  const float* __restrict__ Gp = S.gram;
  const float* __restrict__ wout = S.wout;
  const int nsplit = S.nsplit, ci = a.ci, cx = a.cx;
  const int co0 = blockIdx.y * 64, c1_0 = blockIdx.z * 64;
  const long slice = (long)a.nimg * ci * ci;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hi = lane >> 5;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const bool active = co0 + wm < cx && c1_0 + wn < ci;
  f32x16 acc = mfma32_zero();
  for (int c2_0 = 0; c2_0 < ci; c2_0 += GLS_NLM_KC) {
    const int kn = min(GLS_NLM_KC, ci - c2_0);        // 32 or 64
    const int cpr = kn / 4;
    for (int e = threadIdx.x; e < 64 * cpr; e += 256) {
      const int r = e / cpr, c4 = (e - r * cpr) * 4;
      f32x4 w = {0.f, 0.f, 0.f, 0.f}, g = {0.f, 0.f, 0.f, 0.f};
      if (co0 + r < cx) w = *reinterpret_cast<const f32x4*>(wout + (long)(co0 + r) * ci + c2_0 + c4);
      if (c1_0 + r < ci) {
        const float* gp = Gp + ((long)b * ci + c1_0 + r) * ci + c2_0 + c4;
        f32x4 v[8];
#pragma unroll
        for (int z = 0; z < 8; ++z) {
          v[z] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (z < nsplit) v[z] = *reinterpret_cast<const f32x4*>(gp + z * slice);
        }
        g = v[0];
#pragma unroll
        for (int z = 1; z < 8; ++z) g += v[z];          // the slices in their order: deterministic
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        wsm[r * LD + c4 + k] = w[k];
        gs[r * LD + c4 + k] = g[k];
      }
    }
    __syncthreads();
    if (active) {
      const float* pa = wsm + (wm + l31) * LD + hi;
      const float* pb = gs + (wn + l31) * LD + hi;
      for (int s0 = 0; s0 < kn / 2; s0 += 8) acc = mfma32_f32<8, 2, 2>(pa + 2 * s0, pb + 2 * s0, acc);      // kn / 2 is 16 or 32
    }
    __syncthreads();
  }
  if (active) {
    float* P = S.P + ((long)b * cx + co0 + wm) * ci + c1_0 + wn + l31;
    const float invN = S.invN;
#pragma unroll
    for (int r = 0; r < 16; ++r) P[(long)mfma32_row(r, lane) * ci] = acc[r] * invN;
  }
}

// ---------------------------------------------------------------- apply
// grid (pixel tiles of the largest set, image + nimg * set, tiles(co)).  A = theta [pixel][c1] (converted to fp32 on the way
// into LDS), B = P read as [c1][co].  The accumulators leave through LDS so that a thread adds x + bout to one 16-byte
// chunk of one pixel and stores it whole.
template <typename T>
__global__ __launch_bounds__(256) void nlm_apply_kernel(const NlmArgs a) {
  constexpr int LD = GLS_NLM_KC + 1;
  constexpr int VN = Vec16<T>::N;
  typedef typename Vec16<T>::type V;
  __shared__ float sm[2 * 64 * LD];                  // theta tile | P tile; afterwards the 64 x (64 + 1) accumulator image
  float* th = sm;
  float* pr = sm + 64 * LD;
  const int q = blockIdx.y / a.nimg, b = blockIdx.y - q * a.nimg;
  const NlSet& S = a.s[q];
  const int W = S.W, N = S.H * W, ci = a.ci, cx = a.cx;
  const int j0 = blockIdx.x * 64, co0 = blockIdx.z * 64;
  if (j0 >= N) return;                               // whole workgroup: this set is smaller than the largest one
  const float* __restrict__ P = S.P;
  const T* tbase = reinterpret_cast<const T*>(S.tpg) + b * S.tsn;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hi = lane >> 5;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const bool active = j0 + wm < N && co0 + wn < cx;
  f32x16 acc = mfma32_zero();
  for (int c0 = 0; c0 < ci; c0 += GLS_NLM_KC) {
    const int kn = min(GLS_NLM_KC, ci - c0);          // 32 or 64
    const int cpr = kn / VN;
    for (int idx = threadIdx.x; idx < 64 * cpr; idx += 256) {
      const int r = idx / cpr, ch = idx - r * cpr;
      const int jr = j0 + r;
      stage_f32(th + r * LD + ch * VN, tbase + (long)(jr / W) * S.tsh + (long)(jr % W) * S.tsw + c0 + ch * VN, jr < N);
    }
    const int cp4 = kn / 4;
    for (int idx = threadIdx.x; idx < 64 * cp4; idx += 256) {
      const int r = idx / cp4, c4 = (idx - r * cp4) * 4;
      f32x4 p = {0.f, 0.f, 0.f, 0.f};
      if (co0 + r < cx) p = *reinterpret_cast<const f32x4*>(P + ((long)b * cx + co0 + r) * ci + c0 + c4);
#pragma unroll
      for (int k = 0; k < 4; ++k) pr[r * LD + c4 + k] = p[k];
    }
    __syncthreads();
    if (active) {
      const float* pa = th + (wm + l31) * LD + hi;
      const float* pb = pr + (wn + l31) * LD + hi;
      for (int s0 = 0; s0 < kn / 2; s0 += 8) acc = mfma32_f32<8, 2, 2>(pa + 2 * s0, pb + 2 * s0, acc);      // kn / 2 is 16 or 32
    }
    __syncthreads();
  }
  float* so = sm;                                    // [64 pixels][64 + 1]: 4160 floats of the 8320
  if (active) {
#pragma unroll
    for (int r = 0; r < 16; ++r) so[(wm + mfma32_row(r, lane)) * LD + wn + l31] = acc[r];
  }
  __syncthreads();
  constexpr int CPP = 64 / VN;
  const T* xb = reinterpret_cast<const T*>(S.x) + b * S.xsn;
  T* ob = reinterpret_cast<T*>(S.out) + b * S.osn;
  const float* __restrict__ bout = S.bout;
  for (int idx = threadIdx.x; idx < 64 * CPP; idx += 256) {
    const int r = idx / CPP, ch = idx - r * CPP;
    const int jr = j0 + r, co = co0 + ch * VN;
    if (jr >= N || co >= cx) continue;
    const int py = jr / W, px = jr - py * W;
    V v = *reinterpret_cast<const V*>(xb + (long)py * S.xsh + (long)px * S.xsw + co);
#pragma unroll
    for (int k = 0; k < VN; ++k) v[k] = (T)((float)v[k] + bout[co + k] + so[r * LD + ch * VN + k]);
    *reinterpret_cast<V*>(ob + (long)py * S.osh + (long)px * S.osw + co) = v;
  }
}

}  // namespace glsdet

using namespace glsdet;

extern "C" int64_t glsdet_nonlocal_mfma_workspace_bytes(int32_t n, int32_t n_sets, int32_t ci, int32_t cx) {
  if (n < 1 || n_sets < 1 || n_sets > GLS_NL_SETS || ci < 1 || cx < 1) return 0;
  return (n_sets * nl_layout(n, ci, cx).per_set * 4 + 255) / 256 * 256;
}

extern "C" int glsdet_nonlocal_mfma(const glsdet_view* x, const glsdet_view* tpg, int32_t n_sets, int32_t ci,
                                    const float* const* wout, const float* const* bout, void* ws, int64_t ws_bytes,
                                    const glsdet_view* out, void* stream) {
  if (!x || !tpg || !out || !wout || !bout || !ws) GLS_FAIL(GLSDET_E_ARG, "nonlocal_mfma: null argument");
  if (n_sets < 1 || n_sets > GLS_NL_SETS) GLS_FAIL(GLSDET_E_ARG, "nonlocal_mfma: 1..%d sets, got %d", GLS_NL_SETS, n_sets);
  if (ci < 32 || ci % 32 || ci > GLS_NLM_MAXC)
    GLS_FAIL(GLSDET_E_ARG, "nonlocal_mfma: ci must be a multiple of 32 in [32, %d], got %d", GLS_NLM_MAXC, ci);
  NlmArgs a = {};
  a.n = n_sets; a.ci = ci; a.cx = x[0].c; a.nimg = x[0].n;
  const int dt = x[0].dtype;
  if (dt != GLSDET_F16 && dt != GLSDET_F32) GLS_FAIL(GLSDET_E_ARG, "nonlocal_mfma: dtype must be f16 or f32, got %d", dt);
  if (a.cx < 32 || a.cx % 32 || a.cx > GLS_NLM_MAXC)
    GLS_FAIL(GLSDET_E_ARG, "nonlocal_mfma: x channels must be a multiple of 32 in [32, %d], got %d", GLS_NLM_MAXC, a.cx);
  if (a.nimg < 1 || (long)a.nimg * n_sets > 65535) GLS_FAIL(GLSDET_E_ARG, "nonlocal_mfma: 1..%d images, got %d", 65535 / n_sets, a.nimg);
  if ((uintptr_t)ws & 255) GLS_FAIL(GLSDET_E_ALIGN, "nonlocal_mfma: workspace must be 256-byte aligned");
  const int64_t need = glsdet_nonlocal_mfma_workspace_bytes(a.nimg, n_sets, ci, a.cx);
  if (ws_bytes < need) GLS_FAIL(GLSDET_E_ARG, "nonlocal_mfma: workspace of %ld bytes, %ld needed", (long)ws_bytes, (long)need);
  OpRecord op;
  op.kind = 4;
  op.flops = op.bytes = 0;
  int maxN = 0;
  for (int q = 0; q < n_sets; ++q) {
    int rc;
    if ((long)x[q].h * x[q].w > (1L << 24)) GLS_FAIL(GLSDET_E_ARG, "nonlocal_mfma: set %d: more than 2^24 pixels", q);
    if ((rc = nl_build_set("nonlocal_mfma", a, q, dt, x[q], tpg[q], out[q], wout[q], bout[q], (float*)ws, true, true))) return rc;
    const int N = a.s[q].H * a.s[q].W;
    maxN = std::max(maxN, N);
    // the count of the association these kernels run: Gram 2 N ci^2, fold 2 cx ci^2, apply 2 N ci cx per image
    op.flops += (double)a.nimg * (2.0 * N * ci * (double)ci + 2.0 * a.cx * ci * (double)ci + 2.0 * N * ci * (double)a.cx);
    op.bytes += (double)a.nimg * N * (3.0 * ci + 2.0 * a.cx) * dtype_size(dt);
  }
  op.name = "nonlocal_mfma(gram+fold+apply)";
  op.launch = [=](hipStream_t st) -> int {
    const int nbi = (a.ci + 63) / 64, nbx = (a.cx + 63) / 64;
    const dim3 g1(nbi * nbi, a.nimg, 8 * a.n), g2(a.nimg * a.n, nbx, nbi), g3((maxN + 63) / 64, a.nimg * a.n, nbx);
    return with_dtype(dt, [&](auto t) {
      return nl_launch<nlm_gram_kernel<decltype(t)>, nlm_fold_kernel, nlm_apply_kernel<decltype(t)>>(st, a, g1, g2, g3, 0, 0);
    });
  };
  return submit(std::move(op), stream);
}

