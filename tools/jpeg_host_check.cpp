// Stand-alone check of the JPEG host code (glsdet_amd/csrc/jpeg_host.h: marker parser + Huffman decoder) for a host
// sanitizer; no HIP, no Python.  Build and run on the CPU:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/jpeg_host_check.cpp -o /tmp/jpeg_host_check && /tmp/jpeg_host_check [stream.jpg ...]
//
// Without arguments it reads tests/golden/jpeg_sweep_420_rst.jpg (a 17x17 4:2:0 stream with a restart marker after every
// MCU, from Pillow's encoder).  For each stream, held in a heap block of exactly its size with output buffers of
// exactly n_blocks * 64 and 192 elements, so that the sanitizer sees any access outside them:
//   1. the stream itself must decode;
//   2. every proper prefix must be refused;
//   3. every single-byte substitution by 0x00, 0xFF and the complement must decode or be refused;
//   4. 6000 seeded mutations (1..4 bytes changed, sometimes a span removed or doubled) must decode or be refused.
// Exit status 0 and a one-line summary per stream when everything held.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../glsdet_amd/csrc/jpeg_host.h"

static char g_msg[400];

// -> rc of parse, or of entropy_decode when the stream parses
static int decode(const std::vector<unsigned char>& v) {
  unsigned char* data = (unsigned char*)malloc(v.size() ? v.size() : 1);
  if (!v.empty()) memcpy(data, v.data(), v.size());
  glsdet_jpeg::Err e{g_msg, sizeof g_msg};
  static glsdet_jpeg::Parsed P;
  int rc = glsdet_jpeg::parse(data, (int64_t)v.size(), P, e);
  if (rc == 0 && P.d.n_blocks > (1 << 21)) rc = -100;     // a mutated size field: not worth a gigabyte here
  if (rc == 0) {
    const glsdet_jpeg_desc d = P.d;
    int16_t* coef = (int16_t*)malloc((size_t)d.n_blocks * 64 * sizeof(int16_t));
    uint16_t* qtab = (uint16_t*)malloc(192 * sizeof(uint16_t));
    rc = glsdet_jpeg::entropy_decode(data, (int64_t)v.size(), &d, coef, qtab, e);
    free(coef);
    free(qtab);
  }
  free(data);
  return rc;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 16);
}

static int check(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    return 1;
  }
  std::vector<unsigned char> s;
  for (int c; (c = fgetc(f)) != EOF;) s.push_back((unsigned char)c);
  fclose(f);
  if (decode(s) != 0) {
    fprintf(stderr, "%s: refused: %s\n", path, g_msg);
    return 1;
  }
  long ok = 0, refused = 0;
  for (size_t n = 0; n < s.size(); ++n) {
    if (decode(std::vector<unsigned char>(s.begin(), s.begin() + n)) >= 0) {
      fprintf(stderr, "%s: the prefix of %zu bytes was not refused\n", path, n);
      return 1;
    }
  }
  for (size_t i = 0; i < s.size(); ++i) {
    const unsigned char subs[3] = {0x00, 0xFF, (unsigned char)~s[i]};
    for (unsigned char v : subs) {
      if (v == s[i]) continue;
      std::vector<unsigned char> m = s;
      m[i] = v;
      (decode(m) == 0 ? ok : refused)++;
    }
  }
  for (int k = 0; k < 6000; ++k) {
    std::vector<unsigned char> m = s;
    const int kind = rnd() % 8;
    if (kind == 0 && m.size() > 8) {                       // remove a span
      const size_t a = rnd() % m.size(), len = 1 + rnd() % 6;
      m.erase(m.begin() + a, m.begin() + (a + len < m.size() ? a + len : m.size()));
    } else if (kind == 1) {                                // double a span
      const size_t a = rnd() % m.size(), len = 1 + rnd() % 6, b = a + len < m.size() ? a + len : m.size();
      const std::vector<unsigned char> span(m.begin() + a, m.begin() + b);
      m.insert(m.begin() + a, span.begin(), span.end());
    } else {
      for (int j = 1 + (int)(rnd() % 4); j > 0; --j) m[rnd() % m.size()] = (unsigned char)(rnd() % 3 == 0 ? 0xFF : rnd());
    }
    (decode(m) == 0 ? ok : refused)++;
  }
  printf("%s: %zu bytes; %zu prefixes refused; substitutions and mutations: %ld decoded, %ld refused\n", path, s.size(), s.size(),
         ok, refused);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return check("tests/golden/jpeg_sweep_420_rst.jpg");
  int rc = 0;
  for (int i = 1; i < argc; ++i) rc |= check(argv[i]);
  return rc;
}
