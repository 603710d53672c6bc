// Stand-alone host check of glsdet_nonlocal_mfma's validation and workspace helper, for a sanitizer build on a machine
// without a GPU: every call below is refused before anything is launched and no device pointer is dereferenced.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         tools/probe/nonlocal_mfma_host_check.cpp glsdet_amd/csrc/nonlocal_mfma.hip glsdet_amd/csrc/plan.hip -o nlm_host_check
//   ./nlm_host_check          # prints one line per refusal, exits 0 when all were refused with a message naming nonlocal_mfma
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

struct Call {
  glsdet_view x[5], t[5], o[5];
  const float *w[5], *b[5];
  int n_sets = 2, ci = 64;
  void* ws = (void*)0x600000;
  int64_t ws_bytes;
  explicit Call(int dt) {
    for (int q = 0; q < 5; ++q) {
      x[q] = o[q] = view(2, 3 + (q & 1), 5, 96, dt, 0x100000 + 0x100000 * q);
      t[q] = view(2, 3 + (q & 1), 5, 192, dt, 0x1000000 + 0x100000 * q);
      w[q] = (const float*)(uintptr_t)(0x500000 + 0x10000 * q);
      b[q] = (const float*)(uintptr_t)(0x580000 + 0x400 * q);
    }
    ws_bytes = glsdet_nonlocal_mfma_workspace_bytes(2, 2, 64, 96);
  }
  int run() { return glsdet_nonlocal_mfma(x, t, n_sets, ci, w, b, ws, ws_bytes, o, nullptr); }
};

static int failures = 0;
static void expect_refused(const char* what, Call& c) {
  const int rc = c.run();
  const char* msg = glsdet_last_error();
  const bool ok = rc < 0 && msg && strstr(msg, "nonlocal_mfma");
  printf("%-44s rc %d  %s\n", what, rc, msg ? msg : "(no message)");
  if (!ok) ++failures;
}

int main() {
  for (int dt = GLSDET_F16; dt <= GLSDET_F32; ++dt) {
    { Call c(dt); c.n_sets = 0; expect_refused("n_sets 0", c); }
    { Call c(dt); c.n_sets = 5; expect_refused("n_sets 5", c); }
    { Call c(dt); c.ci = 40; expect_refused("ci 40", c); }
    { Call c(dt); c.ci = 1312; expect_refused("ci 1312", c); }
    { Call c(dt); c.x[0] = c.o[0] = view(2, 3, 5, 40, dt, 0x100000); expect_refused("cx 40", c); }
    { Call c(dt); c.x[1] = c.o[1] = view(3, 4, 5, 96, dt, 0x200000); expect_refused("sets disagree in n", c); }
    { Call c(dt); c.x[1] = c.o[1] = view(2, 4, 5, 128, dt, 0x200000); expect_refused("sets disagree in channels", c); }
    { Call c(dt); c.t[1] = view(2, 4, 5, 160, dt, 0x1100000); expect_refused("tpg.c < 3 ci", c); }
    { Call c(dt); c.x[1] = c.o[1] = view(2, 4, 5, 96, dt, 0x200008); expect_refused("base not 16-byte aligned", c); }
    { Call c(dt); c.t[1] = view(2, 4, 5, 192, dt, 0x1100000, 194); expect_refused("stride not 16-byte aligned", c); }
    { Call c(dt); c.t[1] = view(2, 4, 5, 192, 1 - dt, 0x1100000); expect_refused("tpg of another dtype", c); }
    { Call c(dt); c.o[1] = view(2, 4, 5, 96, 1 - dt, 0x700000); expect_refused("out of another dtype", c); }
    { Call c(dt); c.x[1] = c.o[1] = view(2, 0, 5, 96, dt, 0x200000); expect_refused("an empty window", c); }
    { Call c(dt); c.t[1] = view(2, 4, 5, 192, dt, 0x1100000, 0, -2); expect_refused("a view outside its allocation", c); }
    { Call c(dt); c.ws = (void*)0x600010; expect_refused("ws not 256-byte aligned", c); }
    { Call c(dt); c.ws_bytes -= 1; expect_refused("ws one byte short", c); }
    { Call c(dt); c.ws = nullptr; expect_refused("a null ws", c); }
    { Call c(dt); c.w[1] = nullptr; expect_refused("a null wout", c); }
    { Call c(dt); c.b[1] = (const float*)(uintptr_t)0x580404; expect_refused("a misaligned bout", c); }
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
