// Baseline JPEG decoding, the reference's Image.open(path) / cv2.imread(path) (drone/yolo.py, get_map*.py,
// ufpmp_det_eval.py:93): markers and Huffman on the host (jpeg_host.h), everything at pixel rate here --
//   jpeg_idct_kernel      dequantise + libjpeg jidctint.c (ISLOW) + 128 + saturate -> uint8 component planes
//   jpeg_colour_kernel    jdsample.c fancy upsampling + jdcolor.c YCbCr -> RGB + interleave -> uint8 HWC
// bit for bit what Pillow (libjpeg-turbo, JDCT_ISLOW, fancy upsampling) gives for the same bytes.
#include "common.h"
#include "jpeg_host.h"

namespace glsdet {

#define GLS_JPEG_GRID_CAP 4096          // thread blocks per launch; the kernels stride over the rest

struct JpegGeom {
  int width, height, ncomp, hs, vs;     // hs, vs: luma sampling = the chroma planes' horizontal / vertical factor
  int plane_w[3], plane_h[3];           // padded planes: blocks * 8
  long plane_off[3];                    // byte offset of each plane in the workspace
  long blk_off[3];                      // first block of each component
  int blocks_x[3];
  long n_blocks;
};

// One 1-D pass of jidctint.c on eight inputs, in 64 bit as libjpeg's `long`: with |coef| <= 2048 and q <= 255 an input
// reaches 2^19 and (in0 + in4) << 13 alone 2^33, so 32 bit would overflow on streams the host accepts.
__device__ __forceinline__ void idct_1d(const long in[8], long out[8]) {
  long z1 = (in[2] + in[6]) * 4433;
  const long tmp2 = z1 - in[6] * 15137;
  const long tmp3 = z1 + in[2] * 6270;
  const long tmp0 = (in[0] + in[4]) * 8192;     // << 13 without shifting a negative value
  const long tmp1 = (in[0] - in[4]) * 8192;
  const long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  long t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
  z1 = t0 + t3;
  long z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const long z5 = (z3 + z4) * 9633;
  t0 *= 2446;
  t1 *= 16819;
  t2 *= 25172;
  t3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  out[0] = tmp10 + t3;
  out[7] = tmp10 - t3;
  out[1] = tmp11 + t2;
  out[6] = tmp11 - t2;
  out[2] = tmp12 + t1;
  out[5] = tmp12 - t1;
  out[3] = tmp13 + t0;
  out[4] = tmp13 - t0;
}

// 256 threads = 32 blocks of 8x8, one block per 8 lanes.  Lane r of a block loads coefficient row r (16 bytes) and its
// row of the table, dequantises, and hands the row to LDS; the same lane then runs the COLUMN pass on column r (pass 1:
// the order fixes the rounding), writes the column back, and finally runs the ROW pass on row r and stores its 8 pixels.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qtab,
                                                        unsigned char* __restrict__ planes, const JpegGeom g) {
  __shared__ int tile[32][8][9];        // +1 column of padding: the column reads walk rows
  const int lb = threadIdx.x >> 3, r = threadIdx.x & 7;
  const long groups = (g.n_blocks + 31) / 32;
  for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {      // uniform per thread block: the barriers are safe
    const long blk = grp * 32 + lb;
    const bool live = blk < g.n_blocks;
    int c = 0;
    if (blk >= g.blk_off[1] && g.ncomp == 3) c = blk >= g.blk_off[2] ? 2 : 1;
    if (live) {
      const u32x4 cw = *reinterpret_cast<const u32x4*>(coef + blk * 64 + r * 8);
      const u32x4 qw = *reinterpret_cast<const u32x4*>(qtab + c * 64 + r * 8);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned cv = cw[i], qv = qw[i];
        tile[lb][r][2 * i] = (int)(short)(cv & 0xffff) * (int)(qv & 0xffff);
        tile[lb][r][2 * i + 1] = (int)(short)(cv >> 16) * (int)(qv >> 16);
      }
    }
    __syncthreads();
    long in[8], out[8];
    if (live) {
#pragma unroll
      for (int k = 0; k < 8; ++k) in[k] = tile[lb][k][r];
      idct_1d(in, out);
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int k = 0; k < 8; ++k) tile[lb][k][r] = (int)((out[k] + (1L << 10)) >> 11);
    }
    __syncthreads();
    if (live) {
#pragma unroll
      for (int k = 0; k < 8; ++k) in[k] = tile[lb][r][k];
      idct_1d(in, out);
      unsigned lo = 0, hi = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        long v = ((out[k] + (1L << 17)) >> 18) + 128;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        if (k < 4) lo |= (unsigned)v << (8 * k);
        else hi |= (unsigned)v << (8 * (k - 4));
      }
      const long b = blk - g.blk_off[c];
      const int bx = (int)(b % g.blocks_x[c]), by = (int)(b / g.blocks_x[c]);
      // plane offsets and widths are multiples of 8 and the workspace is 16-byte aligned: an aligned 8-byte store
      uint2* dst = reinterpret_cast<uint2*>(planes + g.plane_off[c] + ((long)by * 8 + r) * g.plane_w[c] + (long)bx * 8);
      *dst = make_uint2(lo, hi);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the chroma sample of output pixel (x, y): jdsample.c on the dw x dh real samples of plane p (row pitch pw)
__device__ __forceinline__ int chroma_at(const unsigned char* __restrict__ p, int pw, int dw, int dh, int hs, int vs, int x,
                                         int y) {
  if (hs == 1) return p[(long)y * pw + x];                            // 4:4:4 (vs is 1 too)
  const int c = x >> 1;
  if (dw <= 2) return p[(long)(vs == 2 ? y >> 1 : y) * pw + c];       // box replication
  const int cn = clamp_i((x & 1) ? c + 1 : c - 1, 0, dw - 1);         // an edge column is its own neighbour
  if (vs == 1) {                                                      // h2v1
    const unsigned char* row = p + (long)y * pw;
    return (3 * row[c] + row[cn] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int r = y >> 1;                                               // h2v2
  const int rn = clamp_i((y & 1) ? r + 1 : r - 1, 0, dh - 1);
  const unsigned char *r0 = p + (long)r * pw, *r1 = p + (long)rn * pw;
  const int s = 3 * r0[c] + r1[c], sn = 3 * r0[cn] + r1[cn];
  return (3 * s + sn + ((x & 1) ? 7 : 8)) >> 4;
}

// One thread owns 4 horizontally adjacent pixels = 12 bytes: three dword stores where the row start is 4-byte aligned
// (x is a multiple of 4, so 3*x is), byte stores otherwise and for the tail of a row.  Plain vector stores only.
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const unsigned char* __restrict__ planes, unsigned char* __restrict__ dst,
                                                          long dst_row_bytes, int order, const JpegGeom g) {
  const int quads = (g.width + 3) >> 2;
  const long total = (long)g.height * quads;
  const int dw = (g.width + g.hs - 1) / g.hs, dh = (g.height + g.vs - 1) / g.vs;
  const unsigned char* py = planes + g.plane_off[0];
  const unsigned char* pcb = planes + g.plane_off[1];
  const unsigned char* pcr = planes + g.plane_off[2];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int y = (int)(i / quads), x0 = (int)(i % quads) * 4;
    const int n = g.width - x0 < 4 ? g.width - x0 : 4;
    unsigned char px[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= n) {
        px[3 * j] = px[3 * j + 1] = px[3 * j + 2] = 0;
        continue;
      }
      const int x = x0 + j;
      const int Y = py[(long)y * g.plane_w[0] + x];
      int R = Y, G = Y, B = Y;
      if (g.ncomp == 3) {
        const int cb = chroma_at(pcb, g.plane_w[1], dw, dh, g.hs, g.vs, x, y) - 128;
        const int cr = chroma_at(pcr, g.plane_w[2], dw, dh, g.hs, g.vs, x, y) - 128;
        R = clamp_i(Y + ((91881 * cr + 32768) >> 16), 0, 255);
        G = clamp_i(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255);
        B = clamp_i(Y + ((116130 * cb + 32768) >> 16), 0, 255);
      }
      px[3 * j] = (unsigned char)(order ? B : R);
      px[3 * j + 1] = (unsigned char)G;
      px[3 * j + 2] = (unsigned char)(order ? R : B);
    }
    unsigned char* o = dst + (long)y * dst_row_bytes + 3L * x0;
    if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
      unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
      for (int k = 0; k < 3; ++k)
        o4[k] = (unsigned)px[4 * k] | ((unsigned)px[4 * k + 1] << 8) | ((unsigned)px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
    } else {
      for (int k = 0; k < 3 * n; ++k) o[k] = px[k];
    }
  }
}

}  // namespace glsdet

using namespace glsdet;

static glsdet_jpeg::Err jpeg_err() {
  static thread_local char buf[400];
  buf[0] = 0;
  return glsdet_jpeg::Err{buf, sizeof buf};
}

extern "C" int glsdet_jpeg_parse(const unsigned char* data, int64_t nbytes, glsdet_jpeg_desc* d) {
  if (!d) GLS_FAIL(GLSDET_E_ARG, "jpeg_parse: null descriptor");
  static thread_local glsdet_jpeg::Parsed P;
  const glsdet_jpeg::Err e = jpeg_err();
  const int rc = glsdet_jpeg::parse(data, nbytes, P, e);
  if (rc) GLS_FAIL(rc, "%s", e.buf);
  *d = P.d;
  return 0;
}

extern "C" int glsdet_jpeg_entropy_decode(const unsigned char* data, int64_t nbytes, const glsdet_jpeg_desc* d, int16_t* coef,
                                          uint16_t* qtab) {
  const glsdet_jpeg::Err e = jpeg_err();
  const int rc = glsdet_jpeg::entropy_decode(data, nbytes, d, coef, qtab, e);
  if (rc) GLS_FAIL(rc, "%s", e.buf);
  return 0;
}

// The geometry from width, height, ncomp, hs, vs alone; refuses a descriptor whose derived fields differ.
static int jpeg_geom(const glsdet_jpeg_desc* d, JpegGeom& g, const char* what) {
  if (!d) GLS_FAIL(GLSDET_E_ARG, "%s: null descriptor", what);
  glsdet_jpeg_desc c = *d;
  const glsdet_jpeg::Err e = jpeg_err();
  if (glsdet_jpeg::layout(c, e)) GLS_FAIL(GLSDET_E_ARG, "%s: %s", what, e.buf);
  bool same = c.mcus_x == d->mcus_x && c.mcus_y == d->mcus_y && c.n_blocks == d->n_blocks;
  for (int i = 0; i < 3; ++i)
    same = same && c.blocks_x[i] == d->blocks_x[i] && c.blocks_y[i] == d->blocks_y[i] && c.hs[i] == d->hs[i] && c.vs[i] == d->vs[i];
  if (!same) GLS_FAIL(GLSDET_E_ARG, "%s: inconsistent descriptor: the block counts do not follow from %d x %d, %d components", what,
                      d->width, d->height, d->ncomp);
  g.width = c.width;
  g.height = c.height;
  g.ncomp = c.ncomp;
  g.hs = c.hs[0];
  g.vs = c.vs[0];
  g.n_blocks = (long)c.n_blocks;
  long off = 0, blk = 0;
  for (int i = 0; i < 3; ++i) {
    g.plane_w[i] = c.blocks_x[i] * 8;
    g.plane_h[i] = c.blocks_y[i] * 8;
    g.blocks_x[i] = c.blocks_x[i] > 0 ? c.blocks_x[i] : 1;
    g.plane_off[i] = off;
    g.blk_off[i] = blk;
    off += (long)g.plane_w[i] * g.plane_h[i];
    blk += (long)c.blocks_x[i] * c.blocks_y[i];
  }
  return 0;
}

extern "C" int64_t glsdet_jpeg_workspace_bytes(const glsdet_jpeg_desc* d) {
  JpegGeom g;
  if (jpeg_geom(d, g, "jpeg_workspace_bytes")) return 0;
  return (g.n_blocks * 64 + 15) / 16 * 16;
}

extern "C" int glsdet_jpeg_reconstruct(const glsdet_jpeg_desc* d, const int16_t* coef, const uint16_t* qtab, void* ws,
                                       int64_t ws_bytes, unsigned char* dst, int64_t dst_row_bytes, int32_t order, void* stream) {
  JpegGeom g;
  int rc;
  if ((rc = jpeg_geom(d, g, "jpeg_reconstruct"))) return rc;
  if (!coef || !qtab || !ws || !dst) GLS_FAIL(GLSDET_E_ARG, "jpeg_reconstruct: null argument");
  if (((uintptr_t)coef & 15) || ((uintptr_t)qtab & 15) || ((uintptr_t)ws & 15))
    GLS_FAIL(GLSDET_E_ALIGN, "jpeg_reconstruct: coef, qtab and the workspace must be 16-byte aligned");
  if (ws_bytes < g.n_blocks * 64)
    GLS_FAIL(GLSDET_E_CAPACITY, "jpeg_reconstruct: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)(g.n_blocks * 64));
  if (dst_row_bytes < 3L * g.width)
    GLS_FAIL(GLSDET_E_ARG, "jpeg_reconstruct: dst_row_bytes %lld is below 3 * width = %d", (long long)dst_row_bytes, 3 * g.width);
  if (order != 0 && order != 1) GLS_FAIL(GLSDET_E_ARG, "jpeg_reconstruct: order %d (0 RGB, 1 BGR)", order);
  unsigned char* planes = (unsigned char*)ws;
  OpRecord op = make_op(1, 0, 128.0 * g.n_blocks + 64.0 * g.n_blocks * 2 + 3.0 * g.width * g.height, "jpeg_idct+upsample_colour");
  op.launch = [=](hipStream_t st) -> int {
    long g1 = (g.n_blocks + 31) / 32, g2 = ((long)g.height * ((g.width + 3) / 4) + 255) / 256;
    if (g1 > GLS_JPEG_GRID_CAP) g1 = GLS_JPEG_GRID_CAP;
    if (g2 > GLS_JPEG_GRID_CAP) g2 = GLS_JPEG_GRID_CAP;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)g1), dim3(256), 0, st, coef, qtab, planes, g);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)g2), dim3(256), 0, st, (const unsigned char*)planes, dst,
                       (long)dst_row_bytes, (int)order, g);
    GLS_HIP(hipGetLastError());
    return 0;
  };
  return submit(std::move(op), stream);
}
