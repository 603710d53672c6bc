// What the two kernel families of the non-local block share (nonlocal.hip: scalar loops sized for ci = 64; nonlocal_mfma.hip:
// the matrix cores for wide blocks): the kernarg structs, the slice rule, the workspace layout, the host code that validates
// one set and fills its NlSet, and the three-kernel launch.
//
//   gram   Gp[z][b][c1][c2] = sum_{j in slice z} phi[b,j,c1] g[b,j,c2]
//   fold   P[b][co][c1]     = (sum_c2 Wout[co][c2] (Gp[0] + Gp[1] + ... in this order)) * fl32(1 / N)
//   apply  out[b,i,co]      = x[b,i,co] + bout[co] + sum_c1 theta[b,i,c1] P[b][co][c1]
#pragma once
#include <string>

#include "common.h"

namespace glsdet {

// Up to GLS_NL_SETS independent blocks (the four quadrants of Patch_Conv_NonLocal) per launch: every kernel takes the
// per-set operands in one kernarg struct and finds its set from the block index.
#define GLS_NL_SETS 4
struct NlSet {
  const unsigned char *x, *tpg;
  unsigned char* out;
  long xsn, xsh, xsw, tsn, tsh, tsw, osn, osh, osw;
  const float *wout, *bout;
  float *gram, *P;
  int H, W, nsplit, jchunk;
  float invN;
};
// the kernarg of the matrix-core kernels, and the head of the scalar kernels' (a larger kernarg moved instructions in
// nlm_fold / nlm_apply, so they keep the short one)
struct NlmArgs {
  NlSet s[GLS_NL_SETS];
  int n, nimg, ci, cx;
};
struct NlArgs : NlmArgs {
  int kc;
  // data-dependent quadrants (Patch_Conv_NonLocal_adapt_new): split = device int32 {row split, column split of the top
  // part, of the bottom part} written by glsdet_attn_split; every set's views then span the FULL FH x FW map and the
  // kernels cut their own window (sets in the order lt, lb, rt, rb).  nullptr: the static windows of the views.
  const int* split;
  int FH, FW, shift;          // shift 1: the windows live on the stride-2 map of the split's map (indices halved)
};

// The slice rule.  The N positions of a set are cut into nsplit slices of jchunk (a multiple of 64) positions; a slice is one
// partial Gram, and the fold adds the partial Grams in ascending order.  A static window picks nsplit from N; a window
// whose extent is only known on the device always takes all 8 (the grid was sized before N existed).
struct NlSlices { int nsplit, jchunk; float invN; };
__host__ __device__ __forceinline__ NlSlices nl_slices(int N, bool device_window) {
  NlSlices s;
  s.nsplit = device_window ? 8 : (N >= 1024 ? 8 : (N >= 256 ? 4 : 1));
  s.jchunk = (((N + s.nsplit - 1) / s.nsplit) + 63) / 64 * 64;
  s.invN = 1.0f / (float)N;
  return s;
}

// The workspace of one set, in floats: eight partial Gram slices [8][nimg][ci][ci], then P [nimg][cx][ci].
struct NlLayout { int64_t per_set, p_off; };
inline NlLayout nl_layout(int nimg, int ci, int cx) {
  const int64_t gram = (int64_t)nimg * 8 * ci * ci;
  return {gram + (int64_t)nimg * cx * ci, gram};
}

// Validates set q of entry point `name` against a.nimg / a.ci / a.cx and the dtype `dt` of the call, and fills a.s[q].
// need16: the views must be 16-byte compatible (check_view); align_w: so must wout / bout.  device_window: the views are the
// full map and the kernels cut the window (NlArgs::split).  Touches nothing but a.s[q].
inline int nl_build_set(const char* name, NlmArgs& a, int q, int dt, const glsdet_view& x, const glsdet_view& tpg,
                        const glsdet_view& out, const float* wout, const float* bout, float* ws, bool need16, bool align_w,
                        bool device_window = false) {
  const std::string nm(name);
  int rc;
  if ((rc = check_view(x, (nm + ".x").c_str(), need16))) return rc;
  if ((rc = check_view(tpg, (nm + ".tpg").c_str(), need16))) return rc;
  if ((rc = check_view(out, (nm + ".out").c_str(), need16))) return rc;
  if (x.dtype != dt || out.dtype != dt || tpg.dtype != dt) GLS_FAIL(GLSDET_E_ARG, "%s: set %d: x / tpg / out must share one dtype", name, q);
  if (x.c != a.cx || x.n != a.nimg) GLS_FAIL(GLSDET_E_ARG, "%s: the sets must agree in n and channels", name);
  if (!same_extent(x, out)) GLS_FAIL(GLSDET_E_ARG, "%s: set %d: x / out extent mismatch", name, q);
  if (tpg.n != x.n || tpg.h != x.h || tpg.w != x.w || a.ci < 1 || tpg.c < 3 * a.ci)
    GLS_FAIL(GLSDET_E_ARG, "%s: set %d: theta|phi|g view must be [n,h,w,>=3*ci]", name, q);
  if (!wout || !bout) GLS_FAIL(GLSDET_E_ARG, "%s: null weight", name);
  if (align_w && (((uintptr_t)wout & 15) || ((uintptr_t)bout & 15))) GLS_FAIL(GLSDET_E_ALIGN, "%s: wout / bout must be 16-byte aligned", name);
  const NlLayout lay = nl_layout(a.nimg, a.ci, a.cx);
  NlSet& S = a.s[q];
  S.x = (const unsigned char*)x.base; S.tpg = (const unsigned char*)tpg.base; S.out = (unsigned char*)out.base;
  S.xsn = x.sn; S.xsh = x.sh; S.xsw = x.sw;
  S.tsn = tpg.sn; S.tsh = tpg.sh; S.tsw = tpg.sw;
  S.osn = out.sn; S.osh = out.sh; S.osw = out.sw;
  S.wout = wout; S.bout = bout;
  S.gram = ws + q * lay.per_set;
  S.P = S.gram + lay.p_off;
  S.H = x.h; S.W = x.w;
  // of a device-side window these hold for the full map, and the kernels replace them per window (nl_window)
  const NlSlices sl = nl_slices(x.h * x.w, device_window);
  S.nsplit = sl.nsplit; S.jchunk = sl.jchunk; S.invN = sl.invN;
  return 0;
}

// gram, fold, apply on one stream: the three grids, and the dynamic LDS of fold and apply
template <auto GRAM, auto FOLD, auto APPLY, typename Args>
inline int nl_launch(hipStream_t st, const Args& a, dim3 g1, dim3 g2, dim3 g3, size_t lds2, size_t lds3) {
  hipLaunchKernelGGL(GRAM, g1, dim3(256), 0, st, a);
  hipLaunchKernelGGL(FOLD, g2, dim3(256), lds2, st, a);
  hipLaunchKernelGGL(APPLY, g3, dim3(256), lds3, st, a);
  GLS_HIP(hipGetLastError());
  return 0;
}

}  // namespace glsdet
