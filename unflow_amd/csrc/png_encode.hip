// PNG encode on the device (core/png_device.py): the row filters, the half of a PNG writer the host cannot vectorise.
//
// unflow_png_filter turns a list of images that already sit in device buffers (the estimator's out_u16, occ, vis) into finished
// PNG scanlines — filter byte, then the filtered row — in one launch; deflate, the chunk CRCs and the file writes stay on the
// host, on a thread pool.  The five candidates of a byte depend on RAW neighbours only (left, up, upper left), never on another
// candidate, so unlike reconstruction (csrc/png_decode.hip) every byte of an image is independent work:
//
//   * one workgroup per (table entry, row); the grid is (max_h, n) and a workgroup beyond its entry's h returns;
//   * the raw bytes of the row and of the row above are formed ONCE into LDS from the surface (a base pointer, strides and a sample
//     kind: no staging copy): u8 as it is, u8 x 255 for the 0 / 1 masks, int16 / uint16 samples as big-endian byte pairs.  Both
//     rows have PNG_PAD zero bytes in front, so the missing neighbours of the first pixel (and the whole row above the first row)
//     read as 0 without a branch.  At most 2 * (PNG_PAD + row bytes): 15 KB for a 1242-pixel 16-bit RGB row;
//   * pass 1: a thread sums the five costs (sum of b < 128 ? b : 256 - b over the candidate's bytes) over a strided run of
//     bytes; wave reductions, one LDS step across the waves, and every thread forms the same argmin (lowest number on a tie);
//   * pass 2: the chosen candidate goes to the output buffer with 16-byte stores between the first and the last 16-byte boundary
//     of the scanline, and with byte stores before and behind them — a scanline is 1 + w * bpp bytes, so consecutive rows start
//     at every alignment.
//
// Integer arithmetic only and no atomics: the output is bit-reproducible.  Compulsory traffic: the source bytes once (the row
// above was the previous workgroup's row: L2) and the scanlines once (DESIGN 7.11 has the measured time).
#include "common.h"

namespace {

constexpr int PNG_PAD = 16;                    // zero bytes in front of an LDS row: x - bpp for x < bpp, bpp <= 8
constexpr int PNG_FILTER_THREADS = 256;
constexpr int PNG_FILTER_WAVES = PNG_FILTER_THREADS / 64;
constexpr int PNG_FILTER_DESC = UNFLOW_PNG_FILTER_FIELDS;

struct SurfaceList {
  unflow_png_surface s[UNFLOW_PNG_SURFACES_MAX];
};

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Row `y` of an image -> its w * bpp raw PNG bytes at `row` (LDS).  y < 0: zeros (the row above the first).
__device__ __forceinline__ void form_row(const unflow_png_surface& sf, long image, int y, int w, unsigned char* row) {
  const int n_el = w * sf.channels;
  const long first = image * sf.image_stride + (long)y * sf.row_stride;
  if (sf.kind == UNFLOW_PNG_U16BE) {
    const unsigned short* src = reinterpret_cast<const unsigned short*>(sf.base) + first;
    unsigned short* to = reinterpret_cast<unsigned short*>(row);          // row is 16-byte aligned
    for (int i = threadIdx.x; i < n_el; i += PNG_FILTER_THREADS) {
      const unsigned v = y < 0 ? 0u : src[i];
      to[i] = (unsigned short)(((v & 255u) << 8) | (v >> 8));              // high byte first
    }
  } else {
    const unsigned char* src = reinterpret_cast<const unsigned char*>(sf.base) + first;
    const unsigned mul = sf.kind == UNFLOW_PNG_U8X255 ? 255u : 1u;
    for (int i = threadIdx.x; i < n_el; i += PNG_FILTER_THREADS) row[i] = (unsigned char)(y < 0 ? 0u : src[i] * mul);
  }
}

// The five filtered values of raw byte x (PNG specification 9.2): None, Sub, Up, Average on the 9-bit sum, Paeth with ties in
// the order left, up, upper left.  cur / up have PNG_PAD zero bytes in front.
__device__ __forceinline__ void candidates(const unsigned char* cur, const unsigned char* up, int x, int bpp, unsigned out[5]) {
  const int v = cur[x], a = cur[x - bpp], b = up[x], c = up[x - bpp];
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  out[0] = (unsigned)v;
  out[1] = (unsigned)(v - a) & 255u;
  out[2] = (unsigned)(v - b) & 255u;
  out[3] = (unsigned)(v - ((a + b) >> 1)) & 255u;
  out[4] = (unsigned)(v - paeth) & 255u;
}

// Byte s of the scanline under filter f: the filter byte, then the filtered row.
__device__ __forceinline__ unsigned scan_byte(const unsigned char* cur, const unsigned char* up, int s, int bpp, int f) {
  if (s == 0) return (unsigned)f;
  unsigned c[5];
  candidates(cur, up, s - 1, bpp, c);
  unsigned r = c[0];
  r = f == 1 ? c[1] : r;
  r = f == 2 ? c[2] : r;
  r = f == 3 ? c[3] : r;
  r = f == 4 ? c[4] : r;
  return r;
}

__global__ __launch_bounds__(PNG_FILTER_THREADS) void png_filter_kernel(SurfaceList list, int n_surfaces,
                                                                        const long* __restrict__ table,
                                                                        unsigned char* __restrict__ out, long out_bytes,
                                                                        int max_row_bytes, int pitch) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];      // 2 rows of `pitch` bytes: PNG_PAD zeros, the row
  __shared__ int red[PNG_FILTER_WAVES][5];
  const long* d = table + (long)blockIdx.y * PNG_FILTER_DESC;
  const long si = d[0], image = d[1], h = d[2], w = d[3], dst = d[4];
  // an entry that does not fit its surface or the output buffer is skipped (the host validates; this is the memory-safety net)
  if (si < 0 || si >= n_surfaces) return;
  const unflow_png_surface& sf = list.s[si];
  const int bpp = sf.channels * (sf.kind == UNFLOW_PNG_U16BE ? 2 : 1);
  if (image < 0 || image >= sf.images || h <= 0 || h > sf.H || w <= 0 || w > sf.W) return;
  const long n = w * bpp;
  if (n > max_row_bytes || dst < 0 || dst > out_bytes || h * (n + 1) > out_bytes - dst) return;
  const int y = blockIdx.x;
  if (y >= h) return;

  unsigned char* cur = lds + PNG_PAD;
  unsigned char* up = lds + pitch + PNG_PAD;
  if (threadIdx.x < PNG_PAD / 4) {
    reinterpret_cast<unsigned*>(lds)[threadIdx.x] = 0u;
    reinterpret_cast<unsigned*>(lds + pitch)[threadIdx.x] = 0u;
  }
  form_row(sf, image, y, (int)w, cur);
  form_row(sf, image, y - 1, (int)w, up);
  __syncthreads();

  int cost[5] = {0, 0, 0, 0, 0};
  for (int x = threadIdx.x; x < (int)n; x += PNG_FILTER_THREADS) {
    unsigned c[5];
    candidates(cur, up, x, bpp, c);
#pragma unroll
    for (int k = 0; k < 5; k++) cost[k] += (int)(c[k] < 128u ? c[k] : 256u - c[k]);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const int t = wave_sum_int(cost[k]);
    if (lane == 0) red[wave][k] = t;
  }
  __syncthreads();
  int f = 0, best = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < 5; k++) {
    int t = 0;
#pragma unroll
    for (int v = 0; v < PNG_FILTER_WAVES; v++) t += red[v][k];
    if (t < best) best = t, f = k;                                         // strict: the lowest filter number wins a tie
  }

  // pass 2: scanline bytes [0, len) -> line; [head, head + 16 * body) is the 16-byte aligned part
  const int len = (int)n + 1;
  unsigned char* line = out + dst + (long)y * len;
  const int head = min((int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(line) & 15u)) & 15u), len);
  const int body = (len - head) >> 4;
  for (int v = threadIdx.x; v < body; v += PNG_FILTER_THREADS) {
    const int s0 = head + (v << 4);
    unsigned q[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      unsigned t = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) t |= scan_byte(cur, up, s0 + 4 * j + k, bpp, f) << (8 * k);
      q[j] = t;
    }
    *reinterpret_cast<uint4*>(line + s0) = make_uint4(q[0], q[1], q[2], q[3]);
  }
  const int tail0 = head + (body << 4);
  const int edge = head + (len - tail0);                                    // at most 15 + 15 bytes
  if ((int)threadIdx.x < edge) {
    const int s = (int)threadIdx.x < head ? (int)threadIdx.x : tail0 + ((int)threadIdx.x - head);
    line[s] = (unsigned char)scan_byte(cur, up, s, bpp, f);
  }
}

}  // namespace

UNFLOW_API int unflow_png_filter(const unflow_png_surface* surfaces, int n_surfaces, const long* table, int n, int max_h,
                                 int max_row_bytes, unsigned char* out, long out_bytes, unflow_stream_t stream) {
  if (!surfaces || !table || !out) return UNFLOW_ERR_NULL;
  if (n_surfaces <= 0 || n_surfaces > UNFLOW_PNG_SURFACES_MAX || n <= 0 || n > 65535 || max_h <= 0 || max_row_bytes <= 0 ||
      out_bytes <= 0)
    return UNFLOW_ERR_SHAPE;
  if (max_row_bytes > UNFLOW_PNG_FILTER_MAX_ROW_BYTES) return UNFLOW_ERR_UNSUPPORTED;
  SurfaceList list{};
  for (int k = 0; k < n_surfaces; k++) {
    const unflow_png_surface& s = surfaces[k];
    if (!s.base) return UNFLOW_ERR_NULL;
    if (s.kind != UNFLOW_PNG_U8 && s.kind != UNFLOW_PNG_U8X255 && s.kind != UNFLOW_PNG_U16BE) return UNFLOW_ERR_UNSUPPORTED;
    if (s.channels < 1 || s.channels > 4 || s.images <= 0 || s.H <= 0 || s.W <= 0) return UNFLOW_ERR_SHAPE;
    if (s.row_stride < (long)s.W * s.channels || s.image_stride < (long)(s.H - 1) * s.row_stride + (long)s.W * s.channels)
      return UNFLOW_ERR_SHAPE;
    if (s.kind == UNFLOW_PNG_U16BE && (reinterpret_cast<uintptr_t>(s.base) & 1) != 0) return UNFLOW_ERR_UNSUPPORTED;
    list.s[k] = s;
  }
  const int pitch = PNG_PAD + ((max_row_bytes + 15) & ~15);
  const dim3 grid(max_h, n);
  png_filter_kernel<<<grid, PNG_FILTER_THREADS, 2 * pitch, as_stream(stream)>>>(list, n_surfaces, table, out, out_bytes,
                                                                               max_row_bytes, pitch);
  return launch_status();
}
