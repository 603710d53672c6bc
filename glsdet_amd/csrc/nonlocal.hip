// The non-local block (re-associated dot-product form) on scalar loops: glsdet_nonlocal, glsdet_nonlocal_multi and
// glsdet_nonlocal_split.  Coalesced 16-byte-per-lane NHWC kernels sized for ci = 64, where the block is 0.35 % of the
// model's MACs before re-association; nonlocal_mfma.hip runs the same three steps on the matrix cores for wide blocks.
// nonlocal_common.h has the association, the kernarg structs, the slice rule and the workspace layout of both.
#include "nonlocal_common.h"

namespace glsdet {

// the window of set q: the static one of its views, or the quadrant that `split` cuts out of the full map
struct NlWin { int H, W, nsplit, jchunk; long xo, to, oo; float invN; };
__device__ __forceinline__ NlWin nl_window(const NlArgs& a, int q) {
  const NlSet& S = a.s[q];
  NlWin w = {S.H, S.W, S.nsplit, S.jchunk, 0, 0, 0, S.invN};
  if (a.split) {
    const int cx = a.split[0] >> a.shift, cyl = a.split[1] >> a.shift, cyr = a.split[2] >> a.shift;
    const bool bottom = q & 1, right = q >> 1;
    const int c = bottom ? cyr : cyl;
    const int r0 = bottom ? cx : 0, c0 = right ? c : 0;
    w.H = bottom ? a.FH - cx : cx;
    w.W = right ? a.FW - c : c;
    w.xo = r0 * S.xsh + c0 * S.xsw;
    w.to = r0 * S.tsh + c0 * S.tsw;
    w.oo = r0 * S.osh + c0 * S.osw;
    const NlSlices sl = nl_slices(w.H * w.W, true);
    w.nsplit = sl.nsplit;
    w.jchunk = sl.jchunk;
    w.invN = sl.invN;
  }
  return w;
}

// Gp[z][b][c1][c2] = sum_{j in slice z} phi[b,j,c1] * g[b,j,c2]   (16x16 block per workgroup;
// the position range is split over blockIdx.z for parallelism, partial sums are added in a
// fixed order by nl_fold_kernel -> deterministic)
template <typename T>
__global__ __launch_bounds__(256) void nl_gram_kernel(const NlArgs a) {
  __shared__ float ph[64][17], gg[64][17];
  const int q = blockIdx.z >> 3, z = blockIdx.z & 7;
  const NlSet& S = a.s[q];
  const NlWin wn = nl_window(a, q);
  if (z >= wn.nsplit) return;
  const int ci = a.ci;
  const int nb = (ci + 15) / 16;
  const int c1_0 = (blockIdx.x / nb) * 16, c2_0 = (blockIdx.x % nb) * 16;
  const int b = blockIdx.y;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const int W = wn.W, N = wn.H * W;
  const int jbeg = z * wn.jchunk, jend = min(N, jbeg + wn.jchunk);
  const T* base = reinterpret_cast<const T*>(S.tpg) + b * S.tsn + wn.to;
  float acc = 0.f;
  constexpr int VN = 16 / (int)sizeof(T);          // channels per 16-byte chunk
  // whole 16-channel blocks of 16-byte-aligned rows: one vector load per thread and tile instead of 2-byte loads (thread t:
  // matrix t / 128 (phi | g), position (t % 128) / CPB, chunk (t % 128) % CPB; fp32: two passes)
  const bool vec = (ci % 16) == 0 && (S.tsw % VN) == 0 && (S.tsh % VN) == 0 && (S.tsn % VN) == 0 && (wn.to % VN) == 0 &&
                   ((uintptr_t)S.tpg & 15) == 0;
  for (int j0 = jbeg; j0 < jend; j0 += 64) {
    if (vec) {
      constexpr int CPB = 16 / VN;                 // chunks per 16-channel block: 2 (fp16) / 4 (fp32)
#pragma unroll
      for (int e = 0; e < CPB / 2; ++e) {
        const int t = threadIdx.x + e * 256;
        const int mat = t / (64 * CPB), r = t - mat * 64 * CPB;
        const int jj = r / CPB, ch = r - jj * CPB;
        const int j = j0 + jj;
        typename Vec16<T>::type v;
#pragma unroll
        for (int k = 0; k < VN; ++k) v[k] = (T)0.f;
        if (j < jend) {
          const T* px = base + (j / W) * S.tsh + (j % W) * S.tsw;
          v = *reinterpret_cast<const typename Vec16<T>::type*>(px + (mat ? 2 * ci + c2_0 : ci + c1_0) + ch * VN);
        }
        float(*dst)[17] = mat ? gg : ph;
#pragma unroll
        for (int k = 0; k < VN; ++k) dst[jj][ch * VN + k] = (float)v[k];
      }
    } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = threadIdx.x + e * 256;
      const int jj = idx >> 4, cc = idx & 15;
      const int j = j0 + jj;
      float vp = 0.f, vg = 0.f;
      if (j < jend) {
        const T* px = base + (j / W) * S.tsh + (j % W) * S.tsw;
        if (c1_0 + cc < ci) vp = (float)px[ci + c1_0 + cc];
        if (c2_0 + cc < ci) vg = (float)px[2 * ci + c2_0 + cc];
      }
      ph[jj][cc] = vp;
      gg[jj][cc] = vg;
    }
    }
    __syncthreads();
#pragma unroll 16
    for (int jj = 0; jj < 64; ++jj) acc += ph[jj][ty] * gg[jj][tx];
    __syncthreads();
  }
  if (c1_0 + ty < ci && c2_0 + tx < ci)
    S.gram[(((long)z * a.nimg + b) * ci + c1_0 + ty) * ci + c2_0 + tx] = acc;
}

// P[b][co][c1] = (1/N) sum_c2 Wout[co][c2] * (sum_z Gp[z][b][c1][c2]).  Workgroup = (image,
// 16 output channels, 64 rows c1).  The Gram rows are walked in c2 chunks of kc (<= 128)
// columns: the partial slices of a chunk are summed into LDS with all 8 slice loads of an
// element in flight (fixed order -> deterministic); a wave owns 4 output channels, so its
// weight rows are wave-uniform (scalar loads) while lanes are the c1 rows (stride kc+1,
// conflict-free).  Any ci works: LDS holds one chunk, never the whole Gram.
#define GLS_FOLD_CO 16
#define GLS_NL_KC 128
__global__ __launch_bounds__(256) void nl_fold_kernel(const NlArgs a) {
  extern __shared__ float gs[];   // [64][kc+1]
  const int q = blockIdx.x / a.nimg, b = blockIdx.x - q * a.nimg;
  const NlSet& S = a.s[q];
  const float* __restrict__ Gp = S.gram;
  const float* __restrict__ wout = S.wout;
  float* P = S.P;
  const NlWin wn = nl_window(a, q);
  const int nsplit = wn.nsplit, nimg = a.nimg, ci = a.ci, cx = a.cx, kc = a.kc;
  const float invN = wn.invN;
  const int co0 = blockIdx.y * GLS_FOLD_CO, c1_0 = blockIdx.z * 64, ld = kc + 1;
  const long slice = (long)nimg * ci * ci;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) w[q] = wout + (long)min(co0 + wave * 4 + q, cx - 1) * ci;   // wave-uniform rows
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c2_0 = 0; c2_0 < ci; c2_0 += kc) {
    const int kn = min(kc, ci - c2_0);
    for (int e = threadIdx.x; e < 64 * kc; e += 256) {
      const int r = e / kc, c = e - r * kc;
      float a = 0.f;
      if (c1_0 + r < ci && c < kn) {
        const float* g = Gp + ((long)b * ci + c1_0 + r) * ci + c2_0 + c;
        float v[8];
#pragma unroll
        for (int z = 0; z < 8; ++z) v[z] = z < nsplit ? g[z * slice] : 0.f;
        a = v[0];
#pragma unroll
        for (int z = 1; z < 8; ++z) a += v[z];
      }
      gs[r * ld + c] = a;
    }
    __syncthreads();
    const float* g = gs + lane * ld;
#pragma unroll 8
    for (int c = 0; c < kn; ++c) {
      const float gv = g[c];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] += w[q][c2_0 + c] * gv;
    }
    __syncthreads();
  }
  const int c1 = c1_0 + lane;
  if (c1 < ci) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int co = co0 + wave * 4 + q;
      if (co < cx) P[((long)b * cx + co) * ci + c1] = acc[q] * invN;
    }
  }
}

// out[b,i,co] = x[b,i,co] + bout[co] + sum_c1 theta[b,i,c1] * P[b][co][c1]
// Workgroup = 64 pixels x 32 output channels of one image.  c1 is walked in chunks of kc:
// a theta tile [64][kc+1] and the P rows [32][kc] live in LDS; lanes are pixels (theta rows
// conflict-free), a wave owns 8 output channels (P reads are broadcasts), whose 8
// accumulators share each theta read and persist across the chunks.
#define GLS_APPLY_CO 32
template <typename T>
__global__ __launch_bounds__(256) void nl_apply_kernel(const NlArgs a) {
  extern __shared__ float th[];   // [64][kc+1] theta, then [GLS_APPLY_CO][kc] P rows
  const int q = blockIdx.y / a.nimg, b = blockIdx.y - q * a.nimg;
  const NlSet& S = a.s[q];
  const unsigned char *x = S.x, *tpg = S.tpg;
  unsigned char* out = S.out;
  const long xsn = S.xsn, xsh = S.xsh, xsw = S.xsw, tsn = S.tsn, tsh = S.tsh, tsw = S.tsw, osn = S.osn, osh = S.osh,
             osw = S.osw;
  const float* __restrict__ P = S.P;
  const float* __restrict__ bout = S.bout;
  const NlWin wn = nl_window(a, q);
  const int W = wn.W, ci = a.ci, cx = a.cx, kc = a.kc;
  const int N = wn.H * W;
  const int j0 = blockIdx.x * 64, co0 = blockIdx.z * GLS_APPLY_CO;
  if (j0 >= N) return;            // block-uniform: this set is smaller than the largest one
  const int ld = kc + 1;
  float* pr = th + 64 * ld;
  const int jj = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int j = j0 + jj;
  constexpr int VN = 16 / (int)sizeof(T);
  // 16-byte loads / stores where the views allow it (rows and windows on 16-byte boundaries)
  const bool vec_t = (tsw % VN) == 0 && (tsh % VN) == 0 && (tsn % VN) == 0 && (wn.to % VN) == 0 && ((uintptr_t)tpg & 15) == 0;
  const bool vec_o = (xsw % VN) == 0 && (xsh % VN) == 0 && (xsn % VN) == 0 && (wn.xo % VN) == 0 && ((uintptr_t)x & 15) == 0 &&
                     (osw % VN) == 0 && (osh % VN) == 0 && (osn % VN) == 0 && (wn.oo % VN) == 0 && ((uintptr_t)out & 15) == 0 &&
                     (cx % VN) == 0 && kc >= GLS_APPLY_CO;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < ci; c0 += kc) {
    const int kn = min(kc, ci - c0);
    if (vec_t && (kn % VN) == 0) {                   // theta tile by 16-byte loads
      const int cpr = kn / VN;
      for (int idx = threadIdx.x; idx < 64 * cpr; idx += 256) {
        const int r = idx / cpr, ch = idx - r * cpr;
        const int jr = j0 + r;
        typename Vec16<T>::type v;
#pragma unroll
        for (int k = 0; k < VN; ++k) v[k] = (T)0.f;
        if (jr < N)
          v = *reinterpret_cast<const typename Vec16<T>::type*>(reinterpret_cast<const T*>(tpg) + b * tsn + wn.to + (jr / W) * tsh + (jr % W) * tsw + c0 + ch * VN);
#pragma unroll
        for (int k = 0; k < VN; ++k) th[r * ld + ch * VN + k] = (float)v[k];
      }
    } else
    for (int idx = threadIdx.x; idx < 64 * kn; idx += 256) {
      const int r = idx / kn, c = idx - r * kn;
      const int jr = j0 + r;
      float v = 0.f;
      if (jr < N) v = (float)(reinterpret_cast<const T*>(tpg) + b * tsn + wn.to + (jr / W) * tsh + (jr % W) * tsw)[c0 + c];
      th[r * ld + c] = v;
    }
    for (int idx = threadIdx.x; idx < GLS_APPLY_CO * kn; idx += 256) {
      const int r = idx / kn, c = idx - r * kn;
      pr[r * kc + c] = (co0 + r) < cx ? P[((long)b * cx + co0 + r) * ci + c0 + c] : 0.f;
    }
    __syncthreads();
    const float* t = th + jj * ld;
    const float* p0 = pr + grp * 8 * kc;
#pragma unroll 4
    for (int c = 0; c < kn; ++c) {
      const float tv = t[c];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] += tv * p0[q * kc + c];
    }
    __syncthreads();
  }
  if (vec_o) {
    // the accumulators go through LDS ([64 pixels][32 channels + 1], the theta tile's space: 64 * (kc + 1) floats with
    // kc >= 32) so that a thread adds x + bout to ONE 16-byte chunk of one pixel and stores it whole; lanes that hold pixels
    // wrote 64 two-byte stores per instruction before
    float* so = th;
#pragma unroll
    for (int q = 0; q < 8; ++q) so[jj * (GLS_APPLY_CO + 1) + grp * 8 + q] = acc[q];
    __syncthreads();
    constexpr int CPP = GLS_APPLY_CO / VN;          // chunks per pixel
    for (int idx = threadIdx.x; idx < 64 * CPP; idx += 256) {
      const int r = idx / CPP, ch = idx - r * CPP;
      const int jr = j0 + r, co = co0 + ch * VN;
      if (jr >= N || co >= cx) continue;
      const long px_x = b * xsn + wn.xo + (jr / W) * xsh + (jr % W) * xsw + co;
      const long px_o = b * osn + wn.oo + (jr / W) * osh + (jr % W) * osw + co;
      typename Vec16<T>::type v = *reinterpret_cast<const typename Vec16<T>::type*>(reinterpret_cast<const T*>(x) + px_x);
#pragma unroll
      for (int k = 0; k < VN; ++k) v[k] = (T)((float)v[k] + bout[co + k] + so[r * (GLS_APPLY_CO + 1) + ch * VN + k]);
      *reinterpret_cast<typename Vec16<T>::type*>(reinterpret_cast<T*>(out) + px_o) = v;
    }
    return;
  }
  if (j >= N) return;
  const long poff_x = b * xsn + wn.xo + (j / W) * xsh + (j % W) * xsw;
  const long poff_o = b * osn + wn.oo + (j / W) * osh + (j % W) * osw;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int co = co0 + grp * 8 + q;
    if (co < cx) {
      const float xv = (float)(reinterpret_cast<const T*>(x) + poff_x)[co];
      (reinterpret_cast<T*>(out) + poff_o)[co] = (T)(xv + bout[co] + acc[q]);
    }
  }
}

// the op of a.n validated sets, shared by the static and the device-side windows; maxN sizes the apply grid
static int nl_submit(const NlArgs& a, int dt, int maxN, OpRecord&& op, void* stream) {
  op.kind = 4;
  op.launch = [=](hipStream_t st) -> int {
    const int nb = (a.ci + 15) / 16;
    const dim3 g1(nb * nb, a.nimg, 8 * a.n), g2(a.nimg * a.n, (a.cx + GLS_FOLD_CO - 1) / GLS_FOLD_CO, (a.ci + 63) / 64),
        g3((maxN + 63) / 64, a.nimg * a.n, (a.cx + GLS_APPLY_CO - 1) / GLS_APPLY_CO);
    const size_t lds2 = (size_t)64 * (a.kc + 1) * 4;
    const size_t lds3 = ((size_t)64 * (a.kc + 1) + (size_t)GLS_APPLY_CO * a.kc) * 4;
    return with_dtype(dt, [&](auto t) {
      return nl_launch<nl_gram_kernel<decltype(t)>, nl_fold_kernel, nl_apply_kernel<decltype(t)>>(st, a, g1, g2, g3, lds2, lds3);
    });
  };
  return submit(std::move(op), stream);
}

}  // namespace glsdet

using namespace glsdet;

extern "C" int glsdet_nonlocal_multi(const glsdet_view* x, const glsdet_view* tpg, int32_t n_sets, int32_t ci,
                                     const float* const* wout, const float* const* bout, float* gram,
                                     const glsdet_view* out, void* stream) {
  if (!x || !tpg || !out || !wout || !bout || !gram) GLS_FAIL(GLSDET_E_ARG, "nonlocal: null argument");
  if (n_sets < 1 || n_sets > GLS_NL_SETS) GLS_FAIL(GLSDET_E_ARG, "nonlocal: 1..%d sets", GLS_NL_SETS);
  NlArgs a = {};
  a.n = n_sets; a.ci = ci; a.cx = x[0].c; a.nimg = x[0].n;
  a.kc = ci < GLS_NL_KC ? ci : GLS_NL_KC;
  OpRecord op;
  op.flops = op.bytes = 0;
  int maxN = 0;
  const int dt = x[0].dtype;
  for (int q = 0; q < n_sets; ++q) {
    int rc;
    if ((rc = nl_build_set("nonlocal", a, q, dt, x[q], tpg[q], out[q], wout[q], bout[q], gram, false, false))) return rc;
    const int N = a.s[q].H * a.s[q].W;
    if (N > maxN) maxN = N;
    // algorithmic count of the reference's two matmuls: 2 * (N*N*ci) MACs per image
    op.flops += 2.0 * 2.0 * (double)a.nimg * N * (double)N * ci;
    op.bytes += (double)a.nimg * N * (3.0 * ci + 2.0 * a.cx) * dtype_size(dt);
  }
  op.name = n_sets > 1 ? "nonlocal_multi(gram+fold+apply)" : "nonlocal(gram+fold+apply)";
  return nl_submit(a, dt, maxN, std::move(op), stream);
}

// Patch_Conv_NonLocal_adapt_new: the four quadrant blocks on windows whose extents live in DEVICE memory (`split`, written
// by glsdet_attn_split): x / out are the full maps, tpg[q] the full-map projections with quadrant q's weights.
extern "C" int glsdet_nonlocal_split(const glsdet_view* x, const glsdet_view* tpg, int32_t ci, const float* const* wout,
                                     const float* const* bout, float* gram, const glsdet_view* out, const int32_t* split,
                                     int32_t split_shift, void* stream) {
  if (!x || !tpg || !out || !wout || !bout || !gram || !split || split_shift < 0 || split_shift > 1)
    GLS_FAIL(GLSDET_E_ARG, "nonlocal_split: bad argument");
  NlArgs a = {};
  a.n = 4; a.ci = ci; a.cx = x->c; a.nimg = x->n;
  a.kc = ci < GLS_NL_KC ? ci : GLS_NL_KC;
  a.split = split; a.FH = x->h; a.FW = x->w; a.shift = split_shift;
  const int dt = x->dtype;
  for (int q = 0; q < 4; ++q) {
    int rc;
    if ((rc = nl_build_set("nonlocal_split", a, q, dt, *x, tpg[q], *out, wout[q], bout[q], gram, false, false, true))) return rc;
  }
  const int maxN = x->h * x->w;
  OpRecord op;
  op.flops = 2.0 * 2.0 * (double)a.nimg * maxN * (double)maxN / 4.0 * ci;      // four quadrants of ~N/4 positions each
  op.bytes = (double)a.nimg * maxN * (3.0 * ci + 2.0 * a.cx) * dtype_size(dt);
  op.name = "nonlocal_split(gram+fold+apply, device-side quadrants)";
  return nl_submit(a, dt, maxN, std::move(op), stream);
}

extern "C" int glsdet_nonlocal(const glsdet_view* x, const glsdet_view* tpg, int32_t ci, const float* wout,
                               const float* bout, float* gram, const glsdet_view* out, void* stream) {
  return glsdet_nonlocal_multi(x, tpg, 1, ci, &wout, &bout, gram, out, stream);
}
