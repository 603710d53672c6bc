// The 32 x 32 accumulator tile of one wave on the matrix cores, as nonlocal_mfma.hip, evc.hip and swin.hip use it.
// Lane maps of v_mfma_f32_32x32x2_f32 (k = 2) and v_mfma_f32_32x32x16_f16 (k = 16):
//   A[i = lane & 31][k = lane >> 5 (f32) | 8 (lane >> 5) + e (f16)], B[k][j = lane & 31],
//   C/D register r: row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31.
// The fp32 instruction is a k-ordered fmaf chain, and a product of two fp16 numbers is exact in fp32: neither adds a rounding
// to a scalar loop over the same k order.
// A call site is moved onto a helper only where the kernel then times within the run-to-run spread of the written-out form:
// lvc_encode (zeroing, staging, the k-major loop) and window_attention (zeroing) stay written out for that reason.
#pragma once
#include "common.h"

namespace glsdet {

// row of accumulator register r in the tile (its column is lane & 31)
__device__ __forceinline__ int mfma32_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ f32x16 mfma32_zero() {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  return acc;
}

// acc += A B over k = 0 .. 2 STEPS - 1, fully unrolled.  pa / pb point at this lane's operands of step 0 (already offset by
// its row / column and by lane >> 5 along k); step s reads pa[s * SA] and pb[s * SB].  An operand that lies [row][k] in LDS
// has stride 2, one that lies [k][row of width w] has stride 2 w.
template <int STEPS, int SA, int SB>
__device__ __forceinline__ f32x16 mfma32_f32(const float* pa, const float* pb, f32x16 acc) {
#pragma unroll
  for (int s = 0; s < STEPS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[s * SA], pb[s * SB], acc, 0, 0, 0);
  return acc;
}

// the same over k = 0 .. 16 STEPS - 1 of fp16 operands that lie [row][k]: pa / pb point at this lane's 8 halves of step 0
// (16-byte aligned, already offset by 8 (lane >> 5))
template <int STEPS>
__device__ __forceinline__ f32x16 mfma32_f16(const f16* pa, const f16* pb, f32x16 acc) {
#pragma unroll
  for (int s = 0; s < STEPS; ++s)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8*>(pa + 16 * s), *reinterpret_cast<const f16x8*>(pb + 16 * s),
                                                 acc, 0, 0, 0);
  return acc;
}

// one 16-byte chunk of storage type T into an fp32 LDS row: dst[0 .. Vec16<T>::N) = src[..] if `live`, else zeros
template <typename T>
__device__ __forceinline__ void stage_f32(float* dst, const T* src, bool live) {
  typedef typename Vec16<T>::type V;
  constexpr int VN = Vec16<T>::N;
  V v;
#pragma unroll
  for (int k = 0; k < VN; ++k) v[k] = (T)0.f;
  if (live) v = *reinterpret_cast<const V*>(src);
#pragma unroll
  for (int k = 0; k < VN; ++k) dst[k] = (float)v[k];
}

}  // namespace glsdet
