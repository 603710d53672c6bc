// Unified foreground packing on the device: ufp/UFPMP-Det-Tools/ufp/unified_foreground_packing.py:6-197
// (scale_boxes, ForegroundRegionGeneration, Packing) and spp.py:77-168 (phsppog with sorting='height', recursive_packing)
// on the float32 rows of the coarse detector, so that no chip list crosses the bus between the two stages.  The contract
// (orders, dtypes, tie rules) is in include/glsdet_hip.h; tests/ufp_pack_reference.py restates it one scalar at a time.
//
// The algorithm is sequential in its decisions, and each decision looks at up to a few hundred rectangles: one wave of 64
// per image takes the decisions in uniform control flow and spreads the looking over its lanes.
//   merge : row i keeps its region in registers; the lanes test their j against it, the first hit of the ballot grows the
//           region, and only the lanes behind the hit are tested again (speculate and repair: later j see the grown
//           region, earlier j are not revisited).
//   fill  : one ballot per fitting class per 64 candidates in height order; the free slots wait on an explicit LIFO
//           stack (a fill places one rectangle or dies, so the stack never holds more than regions + 1 slots).
//   claim : placed rectangles in region order; the lanes compare the pending regions' sizes, a ballot prefix orders the
//           chips.
// All state is in LDS (104 bytes per box).  A workgroup is ONE wave: __syncthreads() below orders the LDS traffic of
// that wave for the compiler and costs no waiting.
#include "common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace glsdet {

static constexpr int UFPK_ROW = 104;                                        // bytes of LDS per box, see the layout below
static constexpr int UFPK_TAIL = 32;                                        // the stack's slot number max_det
static constexpr int UFPK_LIMIT = (160 * 1024 - UFPK_TAIL) / UFPK_ROW;      // 1575: gfx950 has 160 KiB of LDS per CU

struct UfpkArgs {
  const float* dets;       // [n_img][max_det][7]
  const int* count;        // [n_img]
  double* chips;           // [n_img][max_det][7]
  float* chips_floor;      // [n_img][max_det][7]
  double* header;          // [n_img][4]
  int* status;             // [n_img]
  int max_det, img_w, img_h;
  float expand;
};

// np.clip on float32 (minimum(maximum(x, lo), hi) with numpy's comparisons): NaN passes, a tie gives the bound
__device__ __forceinline__ float ufpk_clip(float x, float lo, float hi) {
  if (x != x) return x;
  x = x > lo ? x : lo;
  return x < hi ? x : hi;
}

// get_merge_bbox_aera + the test of ForegroundRegionGeneration, float32, every operation rounded on its own
__device__ __forceinline__ bool ufpk_mergeable(const float4 r, const float4 o) {
  const float ux0 = o.x < r.x ? o.x : r.x, uy0 = o.y < r.y ? o.y : r.y;     // Python's min(r, o) / max(r, o)
  const float ux1 = o.z > r.z ? o.z : r.z, uy1 = o.w > r.w ? o.w : r.w;
  const float pa = (r.z - r.x) * (r.w - r.y);
  const float pb = (o.z - o.x) * (o.w - o.y);
  const float both = pa + pb;
  return (ux1 - ux0) * (uy1 - uy0) < both;
}

__device__ __forceinline__ unsigned long long ufpk_lanes_below(int lane) { return (1ull << lane) - 1ull; }

__global__ __launch_bounds__(64) void ufp_pack_kernel(const UfpkArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ufpk_lds[];
  const int L = a.max_det, lane = threadIdx.x, img = blockIdx.x;
  float4* reg = reinterpret_cast<float4*>(ufpk_lds);                         // [L] enlarged box -> region
  double* sw = reinterpret_cast<double*>(ufpk_lds + 16 * (size_t)L);         // [L] magnified width by height rank
  double* sh = sw + L;                                                       // [L] magnified height by height rank
  double* px = sh + L;                                                       // [L] canvas x by height rank (before: width by region)
  double* py = px + L;                                                       // [L] canvas y by height rank (before: height by region)
  double* stack = py + L;                                                    // [L + 1][4] free slots x, y, w, h
  float* asum = reinterpret_cast<float*>(stack + 4 * ((size_t)L + 1));       // [L] object area sum of the region
  int* cnt = reinterpret_cast<int*>(asum + L);                               // [L] objects of the region, 0 = swallowed; then magnification
  int* ord = cnt + L;                                                        // [L] height rank -> region
  int* kpos = ord + L;                                                       // [L] region -> height rank
  int* placed = kpos + L;                                                    // [L] by height rank
  int* pending = placed + L;                                                 // [L] by region
  int* lab = reinterpret_cast<int*>(stack);                                  // [L] labels, before the stack is in use

  double* hdr = a.header + 4 * (long)img;
  const int n = a.count[img];
  if (n <= 0 || n > L) {
    if (lane == 0) {
      a.status[img] = n < 0 || n > L ? 1 : 0;
      hdr[0] = (double)n; hdr[1] = 0.0; hdr[2] = 0.0; hdr[3] = 0.0;      // the count as read
    }
    return;
  }
  const float* rows = a.dets + (long)img * L * 7;
  double* chips = a.chips + (long)img * L * 7;
  float* chips_floor = a.chips_floor + (long)img * L * 7;

  // ---- class-major stable order (np.argsort(labels, kind="stable")) and scale_boxes, float32
  for (int r = lane; r < n; r += 64) {
    const float l = rows[7 * r + 6];
    lab[r] = (l >= -2.0e9f && l <= 2.0e9f) ? (int)l : 0;
  }
  __syncthreads();
  {
    const float wmax = (float)(a.img_w - 1), hmax = (float)(a.img_h - 1), e = a.expand;
    for (int r = lane; r < n; r += 64) {
      const int l = lab[r];
      int p = 0;
      for (int j = 0; j < n; ++j) {
        const int lj = lab[j];
        p += (lj < l || (lj == l && j < r)) ? 1 : 0;
      }
      const float x1 = rows[7 * r], y1 = rows[7 * r + 1], x2 = rows[7 * r + 2], y2 = rows[7 * r + 3];
      const float half_w = ((x2 - x1) * 0.5f) * e, half_h = ((y2 - y1) * 0.5f) * e;
      const float cx = (x2 + x1) * 0.5f, cy = (y2 + y1) * 0.5f;
      reg[p] = make_float4(ufpk_clip(cx - half_w, 0.f, wmax), ufpk_clip(cy - half_h, 0.f, hmax),
                           ufpk_clip(cx + half_w, 0.f, wmax), ufpk_clip(cy + half_h, 0.f, hmax));
      asum[p] = (x2 - x1 + 1.0f) * (y2 - y1 + 1.0f);
      cnt[p] = 1;
    }
  }
  __syncthreads();

  // ---- ForegroundRegionGeneration
  for (int i = 0; i < n; ++i) {
    int c = cnt[i];
    if (c == 0) continue;
    float4 R = reg[i];
    float as = asum[i];
    for (int j0 = 0; j0 < n; j0 += 64) {
      const int j = j0 + lane;
      bool live = j < n && j != i && cnt[j] > 0;
      const float4 o = live ? reg[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      int start = 0;
      for (;;) {
        const unsigned long long hits = __ballot(live && lane >= start && ufpk_mergeable(R, o));
        if (!hits) break;
        const int h = __ffsll((long long)hits) - 1;
        const float4 oh = make_float4(__shfl(o.x, h, 64), __shfl(o.y, h, 64), __shfl(o.z, h, 64), __shfl(o.w, h, 64));
        R = make_float4(oh.x < R.x ? oh.x : R.x, oh.y < R.y ? oh.y : R.y, oh.z > R.z ? oh.z : R.z, oh.w > R.w ? oh.w : R.w);
        as = as + asum[j0 + h];
        c += cnt[j0 + h];
        if (lane == h) {
          cnt[j] = 0;
          live = false;
        }
        start = h + 1;
      }
    }
    if (lane == 0) {
      reg[i] = R;
      asum[i] = as;
      cnt[i] = c;
    }
    __syncthreads();
  }

  // ---- the regions left, in box order, with magnification and magnified size (float64 from here on)
  int m = 0;
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    const int c = j < n ? cnt[j] : 0;
    const float4 R = c > 0 ? reg[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float as = c > 0 ? asum[j] : 0.f;
    const unsigned long long keep = __ballot(c > 0);
    __syncthreads();
    if (c > 0) {
      const int q = m + __popcll(keep & ufpk_lanes_below(lane));
      const double mean = (double)as / (double)c;
      const int mag = mean < 1024.0 ? 4 : (mean < 9216.0 ? 2 : 1);
      reg[q] = R;
      cnt[q] = mag;
      px[q] = (double)(R.z - R.x) * (double)mag;
      py[q] = (double)(R.w - R.y) * (double)mag;
    }
    m += __popcll(keep);
    __syncthreads();
  }

  // ---- sorted(range(m), key=-height): stable.  (Slots are preset so that a NaN height, which has no rank, leaves
  // nothing unwritten: every index below stays inside [0, m).)
  for (int k = lane; k < m; k += 64) {
    ord[k] = 0;
    sw[k] = 0.0;
    sh[k] = 0.0;
  }
  __syncthreads();
  for (int i = lane; i < m; i += 64) {
    const double h = py[i];
    int k = 0;
    for (int j = 0; j < m; ++j) {
      const double hj = py[j];
      k += (hj > h || (hj == h && j < i)) ? 1 : 0;
    }
    ord[k] = i;
    kpos[i] = k;
    sw[k] = px[i];
    sh[k] = h;
  }
  __syncthreads();

  // ---- Packing: bisection on the strip width, the layout of the LAST probe stays in px / py
  double lo = 300.0, hi = 2666.0;
  for (int probe = 0; probe < 16 && lo <= hi; ++probe) {                      // 11 probes: the interval halves and loses 1 each time
    const double width = (lo + hi) / 2.0;
    for (int k = lane; k < m; k += 64) {
      placed[k] = 0;
      px[k] = 0.0;
      py[k] = 0.0;
    }
    __syncthreads();
    double top = 0.0;
    for (int k0 = 0; k0 < m; ++k0) {
      if (placed[k0]) continue;
      const double w0 = sw[k0], h0 = sh[k0];
      if (lane == 0) {
        placed[k0] = 1;
        px[k0] = 0.0;
        py[k0] = top;
        stack[0] = w0; stack[1] = top; stack[2] = width - w0; stack[3] = h0;
      }
      int sp = 1;
      __syncthreads();
      while (sp > 0) {
        --sp;
        const double x = stack[4 * sp], y = stack[4 * sp + 1], w = stack[4 * sp + 2], h = stack[4 * sp + 3];
        int pick = -1, f2 = -1, f3 = -1, f4 = -1, rank = 5;
        for (int c0 = 0; c0 < m; c0 += 64) {
          const int k = c0 + lane;
          const bool ok = k < m && !placed[k];
          const double rw = ok ? sw[k] : 0.0, rh = ok ? sh[k] : 0.0;
          const bool ew = ok && rw == w, lw = ok && rw < w, eh = rh == h, lh = rh < h;
          const unsigned long long b1 = __ballot(ew && eh);
          if (b1) {
            pick = c0 + __ffsll((long long)b1) - 1;
            rank = 1;
            break;
          }
          if (f2 < 0) {
            const unsigned long long b = __ballot(ew && lh);
            if (b) f2 = c0 + __ffsll((long long)b) - 1;
          }
          if (f3 < 0) {
            const unsigned long long b = __ballot(lw && eh);
            if (b) f3 = c0 + __ffsll((long long)b) - 1;
          }
          if (f4 < 0) {
            const unsigned long long b = __ballot(lw && lh);
            if (b) f4 = c0 + __ffsll((long long)b) - 1;
          }
        }
        if (rank != 1) {
          if (f2 >= 0) { rank = 2; pick = f2; }
          else if (f3 >= 0) { rank = 3; pick = f3; }
          else if (f4 >= 0) { rank = 4; pick = f4; }
        }
        if (rank == 5) continue;
        const double rw = sw[pick], rh = sh[pick];
        if (lane == 0) {
          placed[pick] = 1;
          px[pick] = x;
          py[pick] = y;
        }
        __syncthreads();
        // the slots to fill next, the one to visit first pushed last
        double s0x, s0y, s0w, s0h, s1x = 0.0, s1y = 0.0, s1w = 0.0, s1h = 0.0;
        int pushes = 1;
        if (rank == 1) {
          continue;
        } else if (rank == 2) {
          s0x = x; s0y = y + rh; s0w = w; s0h = h - rh;
        } else if (rank == 3) {
          s0x = x + rw; s0y = y; s0w = w - rw; s0h = h;
        } else {
          double smallest = INFINITY;                                         // over the rectangles still unplaced after the pick
          for (int c0 = 0; c0 < m; c0 += 64) {
            const int k = c0 + lane;
            if (k < m && !placed[k]) {
              const double cw = sw[k], chh = sh[k];
              const double s = chh < cw ? chh : cw;
              smallest = s < smallest ? s : smallest;
            }
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const double s = __shfl_xor(smallest, o, 64);
            smallest = s < smallest ? s : smallest;
          }
          if (w - rw < smallest) {
            s0x = x; s0y = y + rh; s0w = w; s0h = h - rh;
          } else if (h - rh < smallest) {
            s0x = x + rw; s0y = y; s0w = w - rw; s0h = h;
          } else if (rw < smallest) {
            pushes = 2;
            s1x = x + rw; s1y = y; s1w = w - rw; s1h = rh;                    // visited first
            s0x = x; s0y = y + rh; s0w = w; s0h = h - rh;
          } else {
            pushes = 2;
            s1x = x; s1y = y + rh; s1w = rw; s1h = h - rh;                    // visited first
            s0x = x + rw; s0y = y; s0w = w - rw; s0h = h;
          }
        }
        if (sp + pushes <= L + 1) {                                           // always: see the header of this file
          if (lane == 0) {
            stack[4 * sp] = s0x; stack[4 * sp + 1] = s0y; stack[4 * sp + 2] = s0w; stack[4 * sp + 3] = s0h;
            if (pushes == 2) {
              stack[4 * sp + 4] = s1x; stack[4 * sp + 5] = s1y; stack[4 * sp + 6] = s1w; stack[4 * sp + 7] = s1h;
            }
          }
          sp += pushes;
        }
        __syncthreads();
      }
      top = top + h0;
    }
    if (top > width) lo = width + 1.0;
    else hi = width - 1.0;
    __syncthreads();
  }

  // ---- the claim loop of Packing: placed rectangles in region order, each takes EVERY pending region of its size
  for (int q = lane; q < m; q += 64) pending[q] = 1;
  __syncthreads();
  int n_chips = 0;
  double cw = 0.0, ch = 0.0;
  for (int i = 0; i < m; ++i) {
    const int k = kpos[i];
    const double x = px[k], y = py[k], w = sw[k], h = sh[k];
    cw = x + w > cw ? x + w : cw;
    ch = y + h > ch ? y + h : ch;
    if (!pending[i]) continue;
    for (int q0 = 0; q0 < m; q0 += 64) {
      const int q = q0 + lane;
      bool mine = false;
      if (q < m && pending[q]) {
        const int kq = kpos[q];
        mine = sw[kq] == w && sh[kq] == h;
      }
      const unsigned long long claim = __ballot(mine);
      if (mine) {
        const int c = n_chips + __popcll(claim & ufpk_lanes_below(lane));
        const float4 R = reg[q];
        pending[q] = 0;
        if (c < L) {
          const double v[7] = {(double)R.x, (double)R.y, (double)(R.z - R.x), (double)(R.w - R.y), x, y, (double)cnt[q]};
#pragma unroll
          for (int e = 0; e < 7; ++e) {
            chips[7 * c + e] = v[e];
            chips_floor[7 * c + e] = (float)floor(v[e]);
          }
        }
      }
      n_chips += __popcll(claim);
    }
    __syncthreads();
  }
  if (lane == 0) {
    a.status[img] = 0;
    hdr[0] = (double)n; hdr[1] = (double)n_chips; hdr[2] = cw; hdr[3] = ch;
  }
}

}  // namespace glsdet

using namespace glsdet;

extern "C" int32_t glsdet_ufp_pack_max_boxes(void) { return UFPK_LIMIT; }

extern "C" int glsdet_ufp_pack(const float* dets, const int32_t* count, int32_t n_img, int32_t max_det, float expand,
                               int32_t img_w, int32_t img_h, double* chips, float* chips_floor, double* header,
                               int32_t* status, void* stream) {
  if (!dets || !count || !chips || !chips_floor || !header || !status) GLS_FAIL(GLSDET_E_ARG, "ufp_pack: null argument");
  if (n_img < 1) GLS_FAIL(GLSDET_E_ARG, "ufp_pack: n_img %d, need >= 1", n_img);
  if (max_det < 1 || max_det > UFPK_LIMIT)
    GLS_FAIL(GLSDET_E_ARG, "ufp_pack: max_det %d outside 1 .. %d (what the LDS layout holds)", max_det, UFPK_LIMIT);
  if (!std::isfinite(expand) || !(expand > 0.f)) GLS_FAIL(GLSDET_E_ARG, "ufp_pack: expand must be finite and > 0 (got %g)", (double)expand);
  if (img_w < 1 || img_h < 1) GLS_FAIL(GLSDET_E_ARG, "ufp_pack: image %d x %d", img_w, img_h);
  if (((uintptr_t)dets & 3) || ((uintptr_t)count & 3) || ((uintptr_t)chips_floor & 3) || ((uintptr_t)status & 3) ||
      ((uintptr_t)chips & 7) || ((uintptr_t)header & 7))
    GLS_FAIL(GLSDET_E_ALIGN, "ufp_pack: dets / count / chips_floor / status must be 4-byte, chips / header 8-byte aligned");
  UfpkArgs a;
  a.dets = dets; a.count = count; a.chips = chips; a.chips_floor = chips_floor; a.header = header; a.status = status;
  a.max_det = max_det; a.img_w = img_w; a.img_h = img_h; a.expand = expand;
  const int lds = UFPK_ROW * max_det + UFPK_TAIL;
  OpRecord op = make_op(6, 0, (double)n_img * max_det * (28.0 + 84.0), "ufp_pack");
  op.launch = [=](hipStream_t st) -> int {
    static int attr_lds = 64 * 1024;
    if (lds > attr_lds) {
      GLS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ufp_pack_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  160 * 1024));
      attr_lds = 160 * 1024;
    }
    hipLaunchKernelGGL(ufp_pack_kernel, dim3(n_img), dim3(64), lds, st, a);
    GLS_HIP(hipGetLastError());
    return 0;
  };
  return submit(std::move(op), stream);
}
