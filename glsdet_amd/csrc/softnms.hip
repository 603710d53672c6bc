// Soft-NMS of merged result files: drone/merge_results.py:41-130 (py_cpu_softnms, batched_soft_nms)
// with the call of :159-163 taken.  The contract is in include/glsdet_hip.h; in short, per class segment (rows in
// ascending original index) and for i = 0 .. N-2:
//     m = first position of the maximum of score[i:]          (== the reference's strict `score[i] < max(score[i+1:])`
//     swap rows i and m (box, score, index) when m != i           with numpy's first-maximum argmax)
//     for k > i: score[k] = fp32(weight(ovr(i, k)) * fp64(score[k]))
// Boxes and scores are fp32 in LDS; areas, intersections, ovr and the weight are fp64 in registers, every operation
// rounded on its own (numpy evaluates one ufunc at a time), one rounding to fp32 per update.
//
// One workgroup owns one (image, class).  It gathers its segment with a stable block scan, then runs the sequential
// loop with ONE barrier per step: the update of step i also forms the arg-max of step i + 1, each wave publishes its
// winner (score, position, box, index) in a parity-buffered slot, and after the barrier every thread reduces the <= 16
// slots on its own.  The pivot therefore travels through the slots, never through the row arrays, and the swap is
// written by the one thread that updates position m (nobody else touches rows i and m in that step).
#include "common.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace glsdet {

static constexpr int SNMS_SCRATCH = 1024;                                   // bytes of LDS in front of the rows
static constexpr int SNMS_ROW = 24;                                         // float4 box + float score + int index
static constexpr int SNMS_LIMIT = (160 * 1024 - SNMS_SCRATCH) / SNMS_ROW;   // 6784 rows: gfx950 has 160 KiB of LDS per CU
static constexpr int SNMS_MAX_CAP = 32768;
static constexpr int SNMS_MAX_WAVES = 16;

struct SnmsArgs {
  const float4* cand;      // [n][cap][2]
  const int* cand_count;   // [n]
  float* dec;              // [n][cap] decayed score by original index (workspace)
  int cap, num_classes, method, lcap;
  double nt, sigma;
  float thresh;
};

__global__ void soft_nms_reset_kernel(int* status) { *status = 0; }

__device__ __forceinline__ bool snms_better(float s, int k, float bs, int bk) { return s > bs || (s == bs && k < bk); }

// the wave's best (score, first position); lane 0 publishes it with the row's box and index.  The rows of this wave's
// own positions were written by this wave: LDS operations of one wave complete in order, the fence keeps the compiler
// from moving the reads above the writes.
__device__ __forceinline__ void snms_publish(float s, int k, int N, const float4* box, const int* idx, float4* pbox, float* ps,
                                             int* pk, int* pidx, int slot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float s2 = __shfl_xor(s, o, 64);
    const int k2 = __shfl_xor(k, o, 64);
    if (snms_better(s2, k2, s, k)) { s = s2; k = k2; }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  if ((threadIdx.x & 63) == 0) {
    ps[slot] = s;
    pk[slot] = k;
    if (k < N) {
      pbox[slot] = box[k];
      pidx[slot] = idx[k];
    }
  }
}

__global__ __launch_bounds__(1024) void soft_nms_segment_kernel(const SnmsArgs a, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char snms_lds[];
  float4* pbox = reinterpret_cast<float4*>(snms_lds);                       // [2][16]
  float* ps = reinterpret_cast<float*>(snms_lds + 512);                     // [2][16]
  int* pk = reinterpret_cast<int*>(snms_lds + 640);                         // [2][16]
  int* pidx = reinterpret_cast<int*>(snms_lds + 768);                       // [2][16]
  int* wcnt = reinterpret_cast<int*>(snms_lds + 896);                       // [16]
  float4* box = reinterpret_cast<float4*>(snms_lds + SNMS_SCRATCH);         // [lcap]
  float* sc = reinterpret_cast<float*>(box + a.lcap);                       // [lcap]
  int* idx = reinterpret_cast<int*>(sc + a.lcap);                           // [lcap]

  const int c = blockIdx.x, img = blockIdx.y;
  const int tid = threadIdx.x, B = blockDim.x, lane = tid & 63, wave = tid >> 6, nwaves = B >> 6;
  int cnt = a.cand_count[img];
  cnt = cnt < 0 ? 0 : (cnt > a.cap ? a.cap : cnt);
  const float4* rows = a.cand + (long)img * a.cap * 2;
  float* dec = a.dec + (long)img * a.cap;

  // ---- stage 1: the class's rows in ascending original index (stable block scan over the image's rows)
  int N = 0;
  bool bad_label = false;
  for (int r0 = 0; r0 < cnt; r0 += B) {
    const int r = r0 + tid;
    bool mine = false;
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.f;
    if (r < cnt) {
      const float4 q = rows[2 * r + 1];
      const bool valid = q.y >= 0.f && q.y < (float)a.num_classes;          // false for NaN
      if (!valid && c == 0) {
        bad_label = true;
        dec[r] = 0.f;
      }
      mine = valid && (int)q.y == c;
      if (mine) {
        b = rows[2 * r];
        s = q.x;
      }
    }
    const unsigned long long bal = __ballot(mine);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int woff = 0, tot = 0;
    for (int w = 0; w < nwaves; ++w) {
      const int v = wcnt[w];
      woff += w < wave ? v : 0;
      tot += v;
    }
    if (mine) {
      const int p = N + woff + __popcll(bal & ((1ull << lane) - 1ull));
      if (p < a.lcap) {
        box[p] = b;
        sc[p] = s;
        idx[p] = r;
      }
    }
    N += tot;
    __syncthreads();
  }
  if (bad_label) atomicOr(status, 2);
  if (N == 0) return;
  if (N > a.lcap) {                                                         // over the segment limit: nothing of it is kept
    for (int r = tid; r < cnt; r += B) {
      const float lab = rows[2 * r + 1].y;
      if (lab >= 0.f && lab < (float)a.num_classes && (int)lab == c) dec[r] = 0.f;
    }
    if (tid == 0) atomicOr(status, 2);
    return;
  }

  // ---- stage 2: the sequential loop
  {
    float bs = -INFINITY;
    int bk = 0x7fffffff;
    for (int k = tid; k < N; k += B) {
      const float s = sc[k];
      if (snms_better(s, k, bs, bk)) { bs = s; bk = k; }
    }
    snms_publish(bs, bk, N, box, idx, pbox, ps, pk, pidx, wave);
  }
  int par = 0;
  for (int i = 0; i < N - 1; ++i) {
    __syncthreads();
    float pvs = ps[par * SNMS_MAX_WAVES];
    int m = pk[par * SNMS_MAX_WAVES], slot = 0;
    for (int w = 1; w < nwaves; ++w) {
      const float s = ps[par * SNMS_MAX_WAVES + w];
      const int k = pk[par * SNMS_MAX_WAVES + w];
      if (snms_better(s, k, pvs, m)) { pvs = s; m = k; slot = w; }
    }
    // the largest remaining score is not above the threshold: scores are >= 0 and weights lie in [0, 1], so nothing
    // from here on can be kept
    if (!(pvs > a.thresh)) break;
    const float4 pb = pbox[par * SNMS_MAX_WAVES + slot];
    const int pi = pidx[par * SNMS_MAX_WAVES + slot];
    const double px1 = pb.x, py1 = pb.y, px2 = pb.z, py2 = pb.w;
    const double parea = (px2 - px1 + 1.0) * (py2 - py1 + 1.0);
    par ^= 1;
    float bs = -INFINITY;
    int bk = 0x7fffffff;
    for (int k = i + 1 + tid; k < N; k += B) {
      const bool swapped = k == m;                                          // m > i here: position m receives old row i
      const int src = swapped ? i : k;
      const float4 kb = box[src];
      float s = sc[src];
      if (swapped) {
        const int ki = idx[i];
        box[i] = pb; sc[i] = pvs; idx[i] = pi;
        box[k] = kb; idx[k] = ki;
      }
      const double x1 = kb.x, y1 = kb.y, x2 = kb.z, y2 = kb.w;
      const double karea = (x2 - x1 + 1.0) * (y2 - y1 + 1.0);
      const double w = fmax(0.0, fmin(px2, x2) - fmax(px1, x1) + 1.0);
      const double h = fmax(0.0, fmin(py2, y2) - fmax(py1, y1) + 1.0);
      const double inter = w * h;
      const double ovr = inter / (parea + karea - inter);
      double weight;
      if (a.method == 1) {
        weight = ovr > a.nt ? 1.0 - ovr : 1.0;
      } else if (a.method == 2) {
        weight = exp(-(ovr * ovr) / a.sigma);
      } else {
        weight = ovr > a.nt ? 0.0 : 1.0;
      }
      s = (float)(weight * (double)s);
      sc[k] = s;
      if (s > bs) { bs = s; bk = k; }                                       // k ascends: the first maximum stays
    }
    snms_publish(bs, bk, N, box, idx, pbox, ps, pk, pidx, par * SNMS_MAX_WAVES + wave);
  }
  __syncthreads();
  for (int k = tid; k < N; k += B) dec[idx[k]] = sc[k];
}

// ---- stage 3: survivors (decayed score > thresh) ranked by (key descending, original index ascending); key = the
// original score, or the decayed one with rescore.  One thread per row, the image's rows pass through LDS in tiles.
__global__ __launch_bounds__(256) void soft_nms_rank_kernel(const SnmsArgs a, int rescore, int max_det, float* __restrict__ dets,
                                                            int* __restrict__ count, int n, int* __restrict__ status) {
  __shared__ float tkey[256];
  __shared__ unsigned char tkeep[256];
  const int img = blockIdx.y, tid = threadIdx.x;
  const int raw = a.cand_count[img];
  const int cnt = raw < 0 ? 0 : (raw > a.cap ? a.cap : raw);
  if (blockIdx.x != 0 && blockIdx.x * 256 >= cnt) return;
  const float4* rows = a.cand + (long)img * a.cap * 2;
  const float* dec = a.dec + (long)img * a.cap;
  const int r = blockIdx.x * 256 + tid;
  float key = 0.f, d = 0.f;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  bool keep = false;
  if (r < cnt) {
    q = rows[2 * r + 1];
    d = dec[r];
    keep = d > a.thresh;
    key = rescore ? d : q.x;
  }
  int rank = 0, total = 0;
  for (int j0 = 0; j0 < cnt; j0 += 256) {
    const int j = j0 + tid;
    float kj = 0.f;
    bool kpj = false;
    if (j < cnt) {
      const float dj = dec[j];
      kpj = dj > a.thresh;
      kj = rescore ? dj : rows[2 * j + 1].x;
    }
    __syncthreads();
    tkey[tid] = kj;
    tkeep[tid] = kpj ? 1 : 0;
    __syncthreads();
    const int lim = min(256, cnt - j0);
    for (int t = 0; t < lim; ++t) {
      const int kp = tkeep[t];
      const float kt = tkey[t];
      total += kp;
      rank += (kp && (kt > key || (kt == key && j0 + t < r))) ? 1 : 0;
    }
  }
  if (keep && rank < max_det) {
    const float4 b = rows[2 * r];
    float* o = dets + ((long)img * max_det + rank) * 7;
    o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w;
    o[4] = q.x; o[5] = d; o[6] = q.y;
  }
  if (blockIdx.x == 0 && tid == 0) {
    count[img] = total < max_det ? total : max_det;
    count[n + img] = total;
    if (raw > a.cap) atomicOr(status, 1);
  }
}

}  // namespace glsdet

using namespace glsdet;

extern "C" int32_t glsdet_soft_nms_segment_limit(void) { return SNMS_LIMIT; }

extern "C" int64_t glsdet_soft_nms_workspace_bytes(int32_t n, int32_t cap) {
  if (n < 1 || cap < 1 || cap > SNMS_MAX_CAP) return 0;
  return (((int64_t)n * cap * 4 + 255) / 256) * 256;
}

extern "C" int glsdet_soft_nms(const float* cand, const int32_t* cand_count, int32_t n, int32_t cap, int32_t num_classes,
                               int32_t method, double iou_thr, double sigma, float min_score, int32_t rescore, int32_t max_det,
                               float* dets, int32_t* count, int32_t* status, void* wsp, int64_t ws_bytes, void* stream) {
  if (!cand || !cand_count || !dets || !count || !status || !wsp) GLS_FAIL(GLSDET_E_ARG, "soft_nms: null argument");
  if (n < 1 || n > 65535 || cap < 1 || max_det < 1) GLS_FAIL(GLSDET_E_ARG, "soft_nms: bad sizes (n %d, cap %d, max_det %d)", n, cap, max_det);
  if (cap > SNMS_MAX_CAP) GLS_FAIL(GLSDET_E_ARG, "soft_nms: cap %d above %d", cap, SNMS_MAX_CAP);
  if (num_classes < 1 || num_classes > 65535) GLS_FAIL(GLSDET_E_ARG, "soft_nms: num_classes %d, need 1 .. 65535", num_classes);
  if (method < 1 || method > 3) GLS_FAIL(GLSDET_E_ARG, "soft_nms: method %d is not 1 (linear), 2 (gaussian) or 3 (hard)", method);
  if (method == 2 && !(sigma > 0.0)) GLS_FAIL(GLSDET_E_ARG, "soft_nms: gaussian decay needs sigma > 0 (got %g)", sigma);
  if (iou_thr != iou_thr) GLS_FAIL(GLSDET_E_ARG, "soft_nms: iou_thr is NaN");
  // rows that are dropped (bad label, over-long segment) get a decayed score of 0: that must never pass `> min_score`
  if (!(min_score >= 0.f) || min_score > 3.0e38f)
    GLS_FAIL(GLSDET_E_ARG, "soft_nms: min_score must be finite and >= 0 (got %g)", (double)min_score);
  if (((uintptr_t)cand & 15) || ((uintptr_t)dets & 3) || ((uintptr_t)count & 3) || ((uintptr_t)cand_count & 3) ||
      ((uintptr_t)status & 3))
    GLS_FAIL(GLSDET_E_ALIGN, "soft_nms: cand must be 16-byte, dets / counts / status 4-byte aligned");
  if ((uintptr_t)wsp & 255) GLS_FAIL(GLSDET_E_ALIGN, "soft_nms: workspace must be 256-byte aligned");
  const int64_t need = glsdet_soft_nms_workspace_bytes(n, cap);
  if (ws_bytes < need) GLS_FAIL(GLSDET_E_CAPACITY, "soft_nms: workspace %ld < %ld bytes", (long)ws_bytes, (long)need);
  SnmsArgs a;
  a.cand = (const float4*)cand;
  a.cand_count = cand_count;
  a.dec = (float*)wsp;
  a.cap = cap; a.num_classes = num_classes; a.method = method;
  a.lcap = std::min(cap, SNMS_LIMIT);
  a.nt = iou_thr; a.sigma = sigma; a.thresh = min_score;
  const int lds = SNMS_SCRATCH + SNMS_ROW * a.lcap;
  const int block = std::min(1024, (a.lcap + 63) / 64 * 64);
  OpRecord op = make_op(6, 0, (double)n * cap * 32.0 + (double)n * max_det * 28.0, "soft_nms(segment+decay+rank)");
  op.launch = [=](hipStream_t st) -> int {
    static int attr_lds = 64 * 1024;
    if (lds > attr_lds) {
      GLS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(soft_nms_segment_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024));
      attr_lds = 160 * 1024;
    }
    hipLaunchKernelGGL(soft_nms_reset_kernel, dim3(1), dim3(1), 0, st, status);
    hipLaunchKernelGGL(soft_nms_segment_kernel, dim3(num_classes, n), dim3(block), lds, st, a, status);
    hipLaunchKernelGGL(soft_nms_rank_kernel, dim3((cap + 255) / 256, n), dim3(256), 0, st, a, rescore != 0 ? 1 : 0, max_det, dets,
                       count, n, status);
    GLS_HIP(hipGetLastError());
    return 0;
  };
  return submit(std::move(op), stream);
}
