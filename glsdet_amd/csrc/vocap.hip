// VOC-style mAP on the device: the drone harness's score,
//   get_map            drone/models/core/utils_map.py:474-512  (greedy matching of the ranked detections of a class)
//                                                     :570-617  (cumulative tp / fp, recall, precision, F1 at score 0.5)
//   voc_ap             :99-140                                  (suffix maximum of the precision, area under the curve)
//   log_average_miss_rate :26-62                                (the nine miss rates picked at the reference FPPI points)
// Everything is fp64 like the reference (python floats, numpy float64), every product and quotient is rounded on its own
// (no fused multiply-add) and the AP is summed one term at a time in ascending index from 0.0, so every number is the
// reference's bit for bit.  `log` / `exp` of the log-average miss rate stay on the host (numpy).
//
// voc_match_kernel: one wave per ((class, image) pair, threshold), lanes across the pair's ground truths, the pair's
// detections sequential in rank order (a match consumes a ground truth).  The `used` flags live in the workspace (no cap
// on the ground truths of a pair); they are cleared by voc_reset_used_kernel ahead of the kernel and then read and written by lane 0
// alone, so no lane ever reads what another lane of the wave stored and the kernel needs no wave-level fence.
// voc_curve_kernel: one workgroup per (class, threshold): chunked scans with a carry, then the sequential AP sum over the
// compacted change points of the recall (at most tp + 1 terms).
// Every offset read from the device is clamped to its array before use: malformed offsets give wrong numbers, not a fault.
#include "common.h"

namespace glsdet {

// grid caps; the kernels stride over what is left
constexpr long VOC_MATCH_GRID = 16384;    // waves: (pair, threshold)
constexpr long VOC_CURVE_GRID = 512;      // workgroups: (class, threshold)
constexpr long VOC_RESET_GRID = 1024;     // workgroups of 256 flags, grid-stride beyond

struct VocArgs {
  const double* dt_box;      // [ND][4] left, top, right, bottom; class-major, rank order inside a class
  const double* score;       // [ND]
  const int* cls_off;        // [C+1]
  const int* pair_off;       // [P+1] into pair_det
  const int* pair_det;       // [ND] detection indices of the pair, ascending
  const int* gt_off;         // [P+1]
  const double* gt_box;      // [NG][4]
  const unsigned char* gt_difficult;   // [NG]
  const int* n_gt;           // [C] non-difficult ground truths
  const int* n_img;          // [C] images with a non-difficult ground truth
  const double* min_overlap; // [T]
  const double* fppi_ref;    // [9]
  int ND, C, P, NG, T;
  unsigned char* used;       // workspace [T][NG]
  int* tp;                   // out [T][ND]: flags after the match kernel, cumulative after the curve kernel
  int* fp;                   // out [T][ND]
  double* rec;               // out [T][ND]
  double* prec;              // out [T][ND]
  double* mpre;              // out [T][ND]  mpre[1 .. n] of voc_ap
  double* cls_out;           // out [T][C][16]
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// arg max over the wave, the LOWEST position wins a tie; lanes without a candidate carry pos = -1
__device__ __forceinline__ void wave_argmax_first(double& v, int& pos) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const double ov = __shfl_xor(v, s, 64);
    const int op = __shfl_xor(pos, s, 64);
    if (op >= 0 && (pos < 0 || ov > v || (ov == v && op < pos))) {
      v = ov;
      pos = op;
    }
  }
}

// The `used` flags are cleared by a kernel of the op's own, not by hipMemsetAsync: replayed from a captured graph the memset
// node did not clear them (tests/test_replay_invariance.py: eager replay equal to the immediate launch, graph replay not),
// the observation csrc/post.hip records for its counters.
__global__ __launch_bounds__(256) void voc_reset_used_kernel(unsigned char* used, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) used[i] = 0;
}

__global__ __launch_bounds__(64) void voc_match_kernel(VocArgs a) {
  const int lane = threadIdx.x;
  const long n = (long)a.P * a.T;
  for (long e = blockIdx.x; e < n; e += gridDim.x) {
    const int p = (int)(e % a.P), t = (int)(e / a.P);
    const int k0 = clampi(a.pair_off[p], 0, a.ND), k1 = clampi(a.pair_off[p + 1], k0, a.ND);
    const int g0 = clampi(a.gt_off[p], 0, a.NG), G = clampi(a.gt_off[p + 1], g0, a.NG) - g0;
    const double thr = a.min_overlap[t];
    unsigned char* used = a.used + (long)t * a.NG + g0;
    const unsigned char* diff = a.gt_difficult + g0;
    int* tp = a.tp + (long)t * a.ND;
    int* fp = a.fp + (long)t * a.ND;
    for (int k = k0; k < k1; ++k) {
      const int di = a.pair_det[k];
      if (di < 0 || di >= a.ND) continue;
      const double* bb = a.dt_box + 4l * di;
      const double b0 = bb[0], b1 = bb[1], b2 = bb[2], b3 = bb[3];
      double best = -1.0;          // ovmax = -1
      int pos = -1;
      for (int g = lane; g < G; g += 64) {
        const double* q = a.gt_box + 4l * (g0 + g);
        const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
        {
#pragma clang fp contract(off)
          const double iw = fmin(b2, q2) - fmax(b0, q0) + 1.0;
          const double ih = fmin(b3, q3) - fmax(b1, q1) + 1.0;
          if (iw > 0 && ih > 0) {
            const double ua = (b2 - b0 + 1.0) * (b3 - b1 + 1.0) + (q2 - q0 + 1.0) * (q3 - q1 + 1.0) - iw * ih;
            const double ov = iw * ih / ua;
            if (ov > best) {       // strict: the first ground truth in file order keeps a tie
              best = ov;
              pos = g;
            }
          }
        }
      }
      wave_argmax_first(best, pos);
      if (lane == 0) {
        int is_tp = 0, is_fp = 0;
        if (pos >= 0 && best >= thr) {
          if (!diff[pos]) {        // a difficult match is neither, and stays unused
            if (!used[pos]) {
              is_tp = 1;
              used[pos] = 1;
            } else {
              is_fp = 1;
            }
          }
        } else {
          is_fp = 1;
        }
        tp[di] = is_tp;
        fp[di] = is_fp;
      }
    }
  }
}

// inclusive sum over the 256 threads of the block; `total` is the block's sum (sm: 4 words of LDS)
__device__ __forceinline__ unsigned long long block_scan_add(unsigned long long v, unsigned long long* sm,
                                                             unsigned long long& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const unsigned long long o = __shfl_up(v, s, 64);
    if (lane >= s) v += o;
  }
  if (lane == 63) sm[wv] = v;
  __syncthreads();
  unsigned long long pre = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const unsigned long long x = sm[w];
    if (w < wv) pre += x;
    all += x;
  }
  __syncthreads();
  total = all;
  return v + pre;
}

// inclusive SUFFIX maximum over the 256 threads of the block
__device__ __forceinline__ double block_scan_max_rev(double v, double* sm, double& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const double o = __shfl_down(v, s, 64);
    if (lane + s < 64) v = fmax(v, o);
  }
  if (lane == 0) sm[wv] = v;
  __syncthreads();
  double post = 0.0, all = 0.0;      // precisions are >= 0
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const double x = sm[w];
    if (w > wv) post = fmax(post, x);
    all = fmax(all, x);
  }
  __syncthreads();
  total = all;
  return fmax(v, post);
}

__global__ __launch_bounds__(256) void voc_curve_kernel(VocArgs a) {
  __shared__ unsigned long long s_sum[4];
  __shared__ double s_max[4];
  __shared__ double s_term[256];
  __shared__ int s_mr[9];
  __shared__ int s_s05;
  const int tid = threadIdx.x;
  const long n_ct = (long)a.C * a.T;
  for (long e = blockIdx.x; e < n_ct; e += gridDim.x) {
    const int c = (int)(e % a.C), t = (int)(e / a.C);
    const int d0 = clampi(a.cls_off[c], 0, a.ND), n = clampi(a.cls_off[c + 1], d0, a.ND) - d0;
    const long base = (long)t * a.ND + d0;
    int* tp = a.tp + base;
    int* fp = a.fp + base;
    double* rec = a.rec + base;
    double* prec = a.prec + base;
    double* mpre = a.mpre + base;
    const double* score = a.score + d0;
    const int ngt_i = a.n_gt[c];
    const double ngt = (double)(ngt_i > 1 ? ngt_i : 1);       // np.maximum(gt_counter_per_class, 1)
    const double nimg = (double)a.n_img[c];
    double ref[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) ref[k] = a.fppi_ref[k];
    if (tid < 9) s_mr[tid] = 0;
    if (tid == 0) s_s05 = -1;
    __syncthreads();

    // ---- cumulative tp / fp, recall, precision; the last index per FPPI point and the last score above 0.5
    unsigned long long carry = 0;
    int last_mr[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) last_mr[k] = 0;
    int s05 = -1;
    for (int b = 0; b < n; b += 256) {
      const int i = b + tid;
      unsigned long long v = 0;
      if (i < n) v = ((unsigned long long)(tp[i] != 0) << 32) | (unsigned long long)(fp[i] != 0);
      unsigned long long total;
      v = block_scan_add(v, s_sum, total) + carry;
      carry += total;
      if (i < n) {
        const int ctp = (int)(v >> 32), cfp = (int)(v & 0xffffffffull);
        tp[i] = ctp;
        fp[i] = cfp;
        const int both = cfp + ctp;
        const double r = (double)ctp / ngt;
        const double pr = (double)ctp / (double)(both > 1 ? both : 1);
        rec[i] = r;
        prec[i] = pr;
        if (score[i] > 0.5) s05 = i;
        const double fppi = (double)cfp / nimg;
#pragma unroll
        for (int k = 0; k < 9; ++k)
          if (fppi <= ref[k]) last_mr[k] = i + 1;          // index into [-1, fppi...]
      }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k)
      if (last_mr[k] > 0) atomicMax(&s_mr[k], last_mr[k]);
    if (s05 >= 0) atomicMax(&s_s05, s05);

    // ---- mpre[1 .. n]: suffix maximum of [prec..., 0], chunks from the back
    double cmax = 0.0;
    for (int b = n > 0 ? ((n - 1) / 256) * 256 : -1; b >= 0; b -= 256) {
      const int i = b + tid;
      double total;
      const double v = fmax(block_scan_max_rev(i < n ? prec[i] : 0.0, s_max, total), cmax);
      cmax = fmax(cmax, total);
      if (i < n) mpre[i] = v;
    }
    __syncthreads();          // rec / mpre of the whole class are visible to the block

    // ---- AP: q = 0 .. n stands for index q + 1 of mrec = [0, rec..., 1] and mpre = [0, prec..., 0]
    double ap = 0.0;
    for (int b = 0; b <= n; b += 256) {
      const int q = b + tid;
      double term = 0.0;
      int flag = 0;
      if (q <= n) {
        const double cur = q < n ? rec[q] : 1.0;
        const double prev = q > 0 ? rec[q - 1] : 0.0;
        if (cur != prev) {
#pragma clang fp contract(off)
          flag = 1;
          term = (cur - prev) * (q < n ? mpre[q] : 0.0);
        }
      }
      unsigned long long total;
      const unsigned long long at = block_scan_add((unsigned long long)flag, s_sum, total);
      if (flag) s_term[(int)at - 1] = term;
      __syncthreads();
      if (tid == 0) {
        const int m = (int)total;
        for (int k = 0; k < m; ++k) {
#pragma clang fp contract(off)
          ap += s_term[k];
        }
      }
      __syncthreads();
    }

    if (tid == 0) {
      double* o = a.cls_out + e * 16;
      const int s = s_s05 < 0 ? 0 : s_s05;
      double f1 = 0.0, r05 = 0.0, p05 = 0.0;
      if (n > 0) {
#pragma clang fp contract(off)
        r05 = rec[s];
        p05 = prec[s];
        const double sum = p05 + r05;
        f1 = r05 * p05 * 2.0 / (sum == 0.0 ? 1.0 : sum);
      }
      o[0] = ap;
      o[1] = (double)(int)(carry >> 32);
      o[2] = (double)s;
      o[3] = f1;
      o[4] = r05;
      o[5] = p05;
      for (int k = 0; k < 9; ++k) {
        const int j = s_mr[k];
        o[6 + k] = j == 0 ? 1.0 : 1.0 - rec[j - 1];       // [1, 1 - rec...][j]
      }
      o[15] = (double)(int)(carry & 0xffffffffull);
    }
    __syncthreads();
  }
}

}  // namespace glsdet

using namespace glsdet;

extern "C" int64_t glsdet_voc_ap_workspace_bytes(int32_t n_gt_boxes, int32_t n_thr) {
  if (n_gt_boxes < 0 || n_thr < 1) return 0;
  const int64_t need = (int64_t)n_gt_boxes * (int64_t)n_thr;
  return need < 256 ? 256 : ((need + 255) / 256) * 256;
}

extern "C" int glsdet_voc_ap(const double* dt_box, const double* score, const int32_t* cls_off, int32_t n_dt, int32_t n_cls,
                             const int32_t* pair_off, const int32_t* pair_det, const int32_t* gt_off, int32_t n_pairs,
                             const double* gt_box, const unsigned char* gt_difficult, int32_t n_gt_boxes,
                             const int32_t* n_gt, const int32_t* n_img, const double* min_overlap, int32_t n_thr,
                             const double* fppi_ref, int32_t* tp, int32_t* fp, double* rec, double* prec, double* mpre,
                             double* cls_out, void* wsp, int64_t ws_bytes, void* stream) {
  if (n_dt < 0 || n_cls < 0 || n_pairs < 0 || n_gt_boxes < 0)
    GLS_FAIL(GLSDET_E_ARG, "voc_ap: negative size (n_dt %d, n_cls %d, n_pairs %d, n_gt_boxes %d)", n_dt, n_cls, n_pairs, n_gt_boxes);
  if (n_thr < 1) GLS_FAIL(GLSDET_E_ARG, "voc_ap: n_thr %d, need at least one threshold", n_thr);
  if (n_pairs > n_dt) GLS_FAIL(GLSDET_E_ARG, "voc_ap: %d pairs for %d detections (a pair owns at least one)", n_pairs, n_dt);
  if (!cls_off || !pair_off || !gt_off || !n_gt || !n_img || !min_overlap || !fppi_ref || !cls_out || !wsp)
    GLS_FAIL(GLSDET_E_ARG, "voc_ap: null argument");
  if (n_dt > 0 && (!dt_box || !score || !pair_det || !tp || !fp || !rec || !prec || !mpre))
    GLS_FAIL(GLSDET_E_ARG, "voc_ap: null detection array");
  if (n_gt_boxes > 0 && (!gt_box || !gt_difficult)) GLS_FAIL(GLSDET_E_ARG, "voc_ap: null ground-truth array");
  if (((uintptr_t)dt_box | (uintptr_t)score | (uintptr_t)gt_box | (uintptr_t)min_overlap | (uintptr_t)fppi_ref | (uintptr_t)rec |
       (uintptr_t)prec | (uintptr_t)mpre | (uintptr_t)cls_out) & 7)
    GLS_FAIL(GLSDET_E_ALIGN, "voc_ap: fp64 arrays must be 8-byte aligned");
  if (((uintptr_t)cls_off | (uintptr_t)pair_off | (uintptr_t)pair_det | (uintptr_t)gt_off | (uintptr_t)n_gt | (uintptr_t)n_img |
       (uintptr_t)tp | (uintptr_t)fp) & 3)
    GLS_FAIL(GLSDET_E_ALIGN, "voc_ap: int32 arrays must be 4-byte aligned");
  const int64_t need = glsdet_voc_ap_workspace_bytes(n_gt_boxes, n_thr);
  if (ws_bytes < need) GLS_FAIL(GLSDET_E_CAPACITY, "voc_ap: workspace %ld < %ld bytes", (long)ws_bytes, (long)need);
  if (n_cls == 0) return 0;
  VocArgs a;
  a.dt_box = dt_box; a.score = score; a.cls_off = cls_off; a.pair_off = pair_off; a.pair_det = pair_det; a.gt_off = gt_off;
  a.gt_box = gt_box; a.gt_difficult = gt_difficult; a.n_gt = n_gt; a.n_img = n_img; a.min_overlap = min_overlap;
  a.fppi_ref = fppi_ref;
  a.ND = n_dt; a.C = n_cls; a.P = n_pairs; a.NG = n_gt_boxes; a.T = n_thr;
  a.used = (unsigned char*)wsp;
  a.tp = tp; a.fp = fp; a.rec = rec; a.prec = prec; a.mpre = mpre; a.cls_out = cls_out;
  OpRecord op = make_op(6, 0, 44.0 * n_dt + 33.0 * n_gt_boxes + (double)n_thr * (32.0 * n_dt + n_gt_boxes), "voc_ap(match+curve)");
  op.launch = [=](hipStream_t st) -> int {
    const long nm = (long)a.P * a.T;
    if (nm > 0) {
      const long nu = (long)a.NG * a.T, nb = (nu + 255) / 256;
      if (nu > 0)
        hipLaunchKernelGGL(voc_reset_used_kernel, dim3((unsigned)(nb < VOC_RESET_GRID ? nb : VOC_RESET_GRID)), dim3(256), 0, st,
                           a.used, nu);
      hipLaunchKernelGGL(voc_match_kernel, dim3((unsigned)(nm < VOC_MATCH_GRID ? nm : VOC_MATCH_GRID)), dim3(64), 0, st, a);
    }
    const long nc = (long)a.C * a.T;
    hipLaunchKernelGGL(voc_curve_kernel, dim3((unsigned)(nc < VOC_CURVE_GRID ? nc : VOC_CURVE_GRID)), dim3(256), 0, st, a);
    GLS_HIP(hipGetLastError());
    return 0;
  };
  return submit(std::move(op), stream);
}
