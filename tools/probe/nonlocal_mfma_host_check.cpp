// Stand-alone host check of the validation, the recorded op and the workspace helper of the four non-local entry points
// (glsdet_nonlocal, glsdet_nonlocal_multi, glsdet_nonlocal_split, glsdet_nonlocal_mfma), for a sanitizer build on a machine
// without a GPU: every call below is refused before anything is launched, or recorded into a plan that is never run, and no
// device pointer is dereferenced.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         tools/probe/nonlocal_mfma_host_check.cpp glsdet_amd/csrc/nonlocal.hip glsdet_amd/csrc/nonlocal_mfma.hip \
//         glsdet_amd/csrc/plan.hip -o nlm_host_check
//   ./nlm_host_check          # one line per refusal and per recorded op; exits 0 when every call was refused with a message
//                             # naming its entry point and every accepted call recorded the expected op ("all refused")
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/glsdet_hip.h"

static glsdet_view view(int n, int h, int w, int c, int dtype, uintptr_t base, int ct = 0, long extra = 0) {
  glsdet_view v;
  memset(&v, 0, sizeof v);
  const int es = dtype == GLSDET_F16 ? 2 : 4;
  if (!ct) ct = c;
  v.base = (void*)base;
  v.n = n, v.h = h, v.w = w, v.c = c, v.dtype = dtype;
  v.sw = ct, v.sh = (int64_t)w * ct, v.sn = (int64_t)h * w * ct;
  v.alloc_lo = (void*)(base & ~(uintptr_t)0xFF);
  v.alloc_hi = (void*)(base + (uintptr_t)((int64_t)n * h * w * ct * es + extra));
  return v;
}

enum Entry { SINGLE, MULTI, SPLIT, MFMA };
static const char* const entry_name[] = {"glsdet_nonlocal", "glsdet_nonlocal_multi", "glsdet_nonlocal_split", "glsdet_nonlocal_mfma"};
static const char* const entry_prefix[] = {"nonlocal", "nonlocal", "nonlocal_split", "nonlocal_mfma"};

// two sets of 2 x {3, 4} x 5 x 96, ci = 64 (five slots, so that a set count of 5 reads fabricated views too); the split
// entry takes one 2 x 4 x 5 map (slot 0 of x / o) and four projections of it
struct Call {
  Entry e;
  int dt;
  glsdet_view x[5], t[5], o[5];
  const float *w[5], *b[5];
  const glsdet_view *px = x, *pt = t, *po = o;      // nulled by the null-operand cases
  const float *const *pw = w, *const *pb = b;
  int n_sets = 2, ci = 64, shift = 0;
  void* ws = (void*)0x4000000;
  const int32_t* split = (const int32_t*)0x5000000;
  int64_t ws_bytes;
  Call(Entry e_, int dt_) : e(e_), dt(dt_) {
    for (int q = 0; q < 5; ++q) {
      const int h = e == SPLIT ? 4 : 3 + (q & 1);
      x[q] = view(2, h, 5, 96, dt, 0x100000 + 0x100000 * q);
      o[q] = view(2, h, 5, 96, dt, 0x2000000 + 0x100000 * q);
      t[q] = view(2, h, 5, 192, dt, 0x1000000 + 0x100000 * q);
      w[q] = (const float*)(uintptr_t)(0x3000000 + 0x10000 * q);
      b[q] = (const float*)(uintptr_t)(0x3100000 + 0x400 * q);
    }
    ws_bytes = glsdet_nonlocal_mfma_workspace_bytes(2, 2, 64, 96);
  }
  int first() const { return 0; }
  int last() const { return e == SINGLE ? 0 : 1; }                 // the last set (projection) the entry reads
  int run() const {
    switch (e) {
      case SINGLE: return glsdet_nonlocal(px, pt, ci, pw ? w[0] : nullptr, pb ? b[0] : nullptr, (float*)ws, po, nullptr);
      case MULTI: return glsdet_nonlocal_multi(px, pt, n_sets, ci, pw, pb, (float*)ws, po, nullptr);
      case SPLIT: return glsdet_nonlocal_split(px, pt, ci, pw, pb, (float*)ws, po, split, shift, nullptr);
      default: return glsdet_nonlocal_mfma(px, pt, n_sets, ci, pw, pb, ws, ws_bytes, po, nullptr);
    }
  }
};

static int failures = 0;
static void expect_refused(const char* what, const Call& c, int want = GLSDET_E_ARG) {
  const int rc = c.run();
  const char* msg = glsdet_last_error();
  const char* pre = entry_prefix[c.e];
  const size_t n = strlen(pre);
  const bool ok = rc == want && msg && !strncmp(msg, pre, n) && (msg[n] == ':' || msg[n] == '.');
  printf("%-22s %-32s rc %d  %s%s\n", entry_name[c.e], what, rc, msg ? msg : "(no message)", ok ? "" : "   <-- UNEXPECTED");
  if (!ok) ++failures;
}

// what every entry point refuses
static void common_sweep(Entry e, int dt) {
  const bool sets = e == MULTI || e == MFMA;
  { Call c(e, dt); c.px = nullptr; expect_refused("null x", c); }
  { Call c(e, dt); c.pt = nullptr; expect_refused("null tpg", c); }
  { Call c(e, dt); c.po = nullptr; expect_refused("null out", c); }
  { Call c(e, dt); c.pw = nullptr; expect_refused("null wout", c); }
  { Call c(e, dt); c.pb = nullptr; expect_refused("null bout", c); }
  { Call c(e, dt); c.ws = nullptr; expect_refused("null ws", c); }
  if (sets) {
    { Call c(e, dt); c.n_sets = 0; expect_refused("n_sets 0", c); }
    { Call c(e, dt); c.n_sets = 5; expect_refused("n_sets 5", c); }
    { Call c(e, dt); c.x[1] = view(3, 4, 5, 96, dt, 0x200000); c.o[1] = view(3, 4, 5, 96, dt, 0x2100000); expect_refused("sets disagree in n", c); }
    { Call c(e, dt); c.x[1] = view(2, 4, 5, 128, dt, 0x200000); c.o[1] = view(2, 4, 5, 128, dt, 0x2100000); expect_refused("sets disagree in channels", c); }
  }
  { Call c(e, dt); c.ci = 0; expect_refused("ci 0", c); }
  const int f = Call(e, dt).first(), l = Call(e, dt).last();
  const int hf = Call(e, dt).x[f].h, hl = Call(e, dt).x[l].h;
  const uintptr_t tl = 0x1000000 + 0x100000 * l, of = 0x2000000 + 0x100000 * f, xf = 0x100000 + 0x100000 * f;
  { Call c(e, dt); c.t[l] = view(2, hl, 5, 160, dt, tl); expect_refused("tpg.c < 3 ci", c); }
  { Call c(e, dt); c.t[l] = view(2, hl, 5, 192, 1 - dt, tl); expect_refused("tpg of another dtype", c); }
  { Call c(e, dt); c.o[f] = view(2, hf, 5, 96, 1 - dt, of); expect_refused("out of another dtype", c); }
  { Call c(e, dt); c.o[f] = view(2, hf, 6, 96, dt, of); expect_refused("x / out extent mismatch", c); }
  { Call c(e, dt); c.t[l] = view(2, hl + 1, 5, 192, dt, tl); expect_refused("tpg / x extent mismatch", c); }
  { Call c(e, dt); c.t[l] = view(2, hl, 5, 192, dt, tl, 0, -2); expect_refused("a view outside its allocation", c, GLSDET_E_BOUNDS); }
  { Call c(e, dt); c.x[f] = view(2, 0, 5, 96, dt, xf); c.o[f] = view(2, 0, 5, 96, dt, of); expect_refused("an empty window", c); }
  if (e != SINGLE) {
    { Call c(e, dt); c.w[l] = nullptr; expect_refused("a null wout of the last set", c); }
    { Call c(e, dt); c.b[l] = nullptr; expect_refused("a null bout of the last set", c); }
  }
}

// kind, flops, bytes (fp16; fp32 doubles them) and name of the op an accepted call records, as the library recorded them
// before the entry points shared their set builder
static const struct { double flops, bytes16; const char* name; } recorded[] = {
    {115200.0, 23040.0, "nonlocal(gram+fold+apply)"},
    {320000.0, 53760.0, "nonlocal_multi(gram+fold+apply)"},
    {51200.0, 30720.0, "nonlocal_split(gram+fold+apply, device-side quadrants)"},
    {4579328.0, 53760.0, "nonlocal_mfma(gram+fold+apply)"},
};
static void expect_recorded(Entry e, int dt) {
  glsdet_plan* plan = glsdet_plan_create();
  glsdet_plan_begin(plan);
  const int rc = Call(e, dt).run();
  glsdet_plan_end(plan);
  int32_t kind = -1;
  double flops = 0, bytes = 0;
  char name[128] = "";
  const int n = glsdet_plan_num_ops(plan);
  if (n == 1) glsdet_plan_op_info(plan, 0, &kind, &flops, &bytes, name, sizeof name);
  const bool ok = rc == 0 && n == 1 && kind == 4 && flops == recorded[e].flops && bytes == recorded[e].bytes16 * (dt == GLSDET_F16 ? 1 : 2) &&
                  !strcmp(name, recorded[e].name);
  printf("%-22s recorded (dtype %d): rc %d, %d op: %d, %.0f, %.0f, \"%s\"%s\n", entry_name[e], dt, rc, n, kind, flops, bytes, name,
         ok ? "" : "   <-- UNEXPECTED");
  if (!ok) ++failures;
  glsdet_plan_destroy(plan);
}

int main() {
  for (int dt = GLSDET_F16; dt <= GLSDET_F32; ++dt) {
    for (int e = SINGLE; e <= MFMA; ++e) {
      common_sweep((Entry)e, dt);
      expect_recorded((Entry)e, dt);
    }
    { Call c(SPLIT, dt); c.split = nullptr; expect_refused("null split", c); }
    { Call c(SPLIT, dt); c.shift = 2; expect_refused("split_shift 2", c); }
    { Call c(SPLIT, dt); c.shift = -1; expect_refused("split_shift -1", c); }
    // what only the matrix-core entry refuses
    { Call c(MFMA, dt); c.ci = 40; expect_refused("ci 40", c); }
    { Call c(MFMA, dt); c.ci = 1312; expect_refused("ci 1312", c); }
    { Call c(MFMA, dt); c.x[0] = view(2, 3, 5, 40, dt, 0x100000); c.o[0] = view(2, 3, 5, 40, dt, 0x2000000); expect_refused("cx 40", c); }
    { Call c(MFMA, dt); c.x[1] = view(2, 4, 5, 96, dt, 0x200008); expect_refused("base not 16-byte aligned", c, GLSDET_E_ALIGN); }
    { Call c(MFMA, dt); c.t[1] = view(2, 4, 5, 192, dt, 0x1100000, 194); expect_refused("stride not 16-byte aligned", c, GLSDET_E_ALIGN); }
    { Call c(MFMA, dt); c.ws = (void*)0x4000010; expect_refused("ws not 256-byte aligned", c, GLSDET_E_ALIGN); }
    { Call c(MFMA, dt); c.ws_bytes -= 1; expect_refused("ws one byte short", c); }
    { Call c(MFMA, dt); c.b[1] = (const float*)(uintptr_t)0x3100404; expect_refused("a misaligned bout", c, GLSDET_E_ALIGN); }
  }
  int64_t prev = 0;
  for (int ci = 32; ci <= 1280; ci += 32) {
    const int64_t cur = glsdet_nonlocal_mfma_workspace_bytes(8, 4, ci, ci);
    if (cur <= prev || cur % 256) ++failures;
    prev = cur;
  }
  if (glsdet_nonlocal_mfma_workspace_bytes(0, 1, 32, 32) || glsdet_nonlocal_mfma_workspace_bytes(1, 5, 32, 32)) ++failures;
  printf("%s\n", failures ? "FAILED" : "all refused");
  return failures ? 1 : 0;
}
