// Internal helpers shared by the translation units of libglsdet_hip.so (gfx950 only).
// The host front of an entry point is written with the helpers below: check_views (null test, then check_view per operand
// in order), the two overlap rules (views_overlap: byte spans, used by the swin.hip ops; channel_slices_disjoint: the
// exemption the conv builders add for slices of one concat buffer), with_dtype, grid_1d and make_op / submit_op.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <functional>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <utility>

#include "../../include/glsdet_hip.h"

typedef _Float16 f16;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// the 16-byte vector of a storage type: what one lane loads or stores of an NHWC pixel
template <typename T> struct Vec16;
template <> struct Vec16<f16> { typedef f16x8 type; static constexpr int N = 8; };
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int N = 4; };

namespace glsdet {

// ---- error plumbing -------------------------------------------------------------------
void set_error(const char* fmt, ...);
#define GLS_FAIL(code, ...)          \
  do {                               \
    ::glsdet::set_error(__VA_ARGS__); \
    return (code);                   \
  } while (0)
#define GLS_HIP(expr)                                                             \
  do {                                                                            \
    hipError_t _e = (expr);                                                       \
    if (_e != hipSuccess) GLS_FAIL(GLSDET_E_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

inline int dtype_size(int dt) { return dt == GLSDET_F16 ? 2 : 4; }

// Host-side check that a view is well formed and that every byte it can address lies in
// its allocation.  `what` names the operand in the error text.
int check_view(const glsdet_view& v, const char* what, bool need16 = true);
// same extent (n,h,w,c)?
inline bool same_extent(const glsdet_view& a, const glsdet_view& b) {
  return a.n == b.n && a.h == b.h && a.w == b.w && a.c == b.c;
}

// [lo, hi) in bytes of everything a view can address
inline void view_span(const glsdet_view& v, const char** lo, const char** hi) {
  *lo = (const char*)v.base;
  *hi = *lo + ((int64_t)(v.n - 1) * v.sn + (int64_t)(v.h - 1) * v.sh + (int64_t)(v.w - 1) * v.sw + v.c) * dtype_size(v.dtype);
}
// The two "y overlaps x" rules.  views_overlap: the byte spans intersect.  channel_slices_disjoint: both views share one
// set of strides and name disjoint channel slices of one pixel (two slices of a concat buffer), so their interleaved spans
// never touch; the conv builders refuse `views_overlap(x, y) && !channel_slices_disjoint(x, y)`.
inline bool views_overlap(const glsdet_view& a, const glsdet_view& b) {
  const char *alo, *ahi, *blo, *bhi;
  view_span(a, &alo, &ahi);
  view_span(b, &blo, &bhi);
  return alo < bhi && blo < ahi;
}
inline bool channel_slices_disjoint(const glsdet_view& x, const glsdet_view& y) {
  const bool same_geom = x.sn == y.sn && x.sh == y.sh && x.sw == y.sw;
  const int64_t off = ((const char*)y.base - (const char*)x.base) / dtype_size(x.dtype), sw = x.sw;
  return same_geom && (off > 0 ? (off >= x.c && off + y.c <= sw) : (off < 0 && -off >= y.c && -off + x.c <= sw));
}

// One operand of check_views: the view, its name in the error text, and whether it needs 16-byte base / strides.
struct ViewArg {
  const glsdet_view* v;
  const char* what;
  bool need16 = true;
};
// The argument checks every entry point opens with: `null_msg` if an operand is null or `also_bad` holds (the entry
// point's other pointer and mode tests that share that message), then check_view per operand in order, first failure wins.
inline int check_views(const char* null_msg, bool also_bad, std::initializer_list<ViewArg> vs) {
  for (const ViewArg& a : vs) also_bad |= !a.v;
  if (also_bad) GLS_FAIL(GLSDET_E_ARG, "%s", null_msg);
  for (const ViewArg& a : vs)
    if (int rc = check_view(*a.v, a.what, a.need16)) return rc;
  return 0;
}
// (base, sn, sh, sw) of a view as the kernels take it
#define GLS_VIN(v) (const unsigned char*)(v).base, (v).sn, (v).sh, (v).sw
#define GLS_VOUT(v) (unsigned char*)(v).base, (v).sn, (v).sh, (v).sw

// ---- dtype dispatch and the 1-D grid rule ---------------------------------------------
// f(T{}) with T the storage type of `dt`: one launch written once instead of an f16 arm and a float arm.
template <typename F>
inline auto with_dtype(int dt, F&& f) {
  return dt == GLSDET_F16 ? f(f16{}) : f(float{});
}
// (x storage, y storage) of a conv: f16 -> f16, f16 -> fp32, fp32 -> fp32
template <typename F>
inline int with_conv_types(int xdt, int ydt, F&& f) {
  if (xdt == GLSDET_F16 && ydt == GLSDET_F16) return f(f16{}, f16{});
  if (xdt == GLSDET_F16 && ydt == GLSDET_F32) return f(f16{}, float{});
  return f(float{}, float{});
}
// workgroups of 256 threads for `items` grid-stride work items: ceil(items / 256) clamped to [1, cap]
inline unsigned grid_1d(long items, long cap = 8192) {
  const long g = (items + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---- plan recording -------------------------------------------------------------------
struct OpRecord {
  int kind;                 // 0 conv, 1 focus, 2 maxpool, 3 resample, 4 nonlocal, 5 decode, 6 nms
  int branch = 0;           // 0 = main sequence; ops of different non-zero branches between two
                            // main ops are independent and may overlap (set by submit())
  double flops, bytes;      // algorithmic 2*MACs and min HBM bytes of this op
  std::string name;         // kernel family / tile name
  std::function<int(hipStream_t)> launch;
};
// If the calling thread is recording a plan the op is appended and 0 returned, otherwise it
// is launched on `stream` right away.
int submit(OpRecord&& op, void* stream);
inline OpRecord make_op(int kind, double flops, double bytes, std::string name) {
  OpRecord op;
  op.kind = kind;
  op.flops = flops;
  op.bytes = bytes;
  op.name = std::move(name);
  return op;
}
// submit() of `op` with `body(stream)` as its launch.  A body that returns void only launches; one that returns int may
// refuse (non-zero ends the launch).  The launch error of either is collected here; a body that launches in a loop may
// also check after each launch.
template <typename F>
inline int submit_op(OpRecord&& op, void* stream, F body) {
  op.launch = [body = std::move(body)](hipStream_t st) -> int {
    if constexpr (std::is_void_v<decltype(body(st))>) {
      body(st);
    } else {
      if (int rc = body(st)) return rc;
    }
    GLS_HIP(hipGetLastError());
    return 0;
  };
  return submit(std::move(op), stream);
}

}  // namespace glsdet
