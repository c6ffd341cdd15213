// Sequence inference (core/inference.py FlowEstimator(..., sequence=True)): the frame a clip's next replay starts from — and,
// further down, the row copy of bidirectional sequence mode (sequence='bidirectional', unflow_sequence_mirror).
//
// In sequence mode the engine keeps F = B + 1 sample rows of the network input and of FlowNetC's feature tower; pair i is
// (row i, row i + 1).  A replay computes rows [1, F) from its new frames; row 0 is the LAST frame of the previous replay,
// which that replay left in row `src` (= the number of frames it staged).  unflow_sequence_carry copies that row to row 0 in
// every buffer of a small list, in one launch, before the input kernel overwrites rows [1, F).
//
// src is read from device memory (the host rewrites it with the geometry tables), so one captured graph serves full and
// short batches; src = 0 (the first replay of a clip: nothing to carry) is a no-op.  A buffer of the list is
// {base, pixels per row, bytes per pixel to copy, pixel stride in bytes}: bytes < stride copies one channel segment of a concat
// buffer (the conv2 segment of cat2) and leaves the other channels of row 0 alone.  The widest vector access that base, bytes
// and stride allow is used (16 bytes for every buffer of the engine: segments start at multiples of 4 channels, plane rows are
// padded to 64 bytes); plain global loads and stores, no buffer descriptors.
#include "common.h"

namespace {

struct CarryList {
  unflow_carry_buf b[UNFLOW_CARRY_MAX];
};

template <typename V>
__device__ __forceinline__ void carry_rows(char* __restrict__ base, int pixels, int bytes, int stride, int src) {
  const int per = bytes / (int)sizeof(V);              // vectors per pixel
  const int n = pixels * per;                          // < 2^31 (the host checks)
  const char* from = base + (long)src * pixels * stride;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int px = i / per, c = i - px * per;
    const long off = (long)px * stride + (long)c * (long)sizeof(V);
    *reinterpret_cast<V*>(base + off) = *reinterpret_cast<const V*>(from + off);
  }
}

__global__ __launch_bounds__(256) void sequence_carry_kernel(CarryList list, const int* __restrict__ src_row, int max_row) {
  const int src = *src_row;
  if (src <= 0 || src > max_row) return;               // nothing to carry / a row the buffers do not have
  const unflow_carry_buf e = list.b[blockIdx.y];
  char* base = reinterpret_cast<char*>(e.base);
  const unsigned long a = reinterpret_cast<unsigned long>(e.base) | (unsigned long)e.bytes | (unsigned long)e.stride;
  if ((a & 15) == 0) carry_rows<uint4>(base, (int)e.pixels, e.bytes, e.stride, src);
  else if ((a & 7) == 0) carry_rows<uint2>(base, (int)e.pixels, e.bytes, e.stride, src);
  else if ((a & 3) == 0) carry_rows<unsigned>(base, (int)e.pixels, e.bytes, e.stride, src);
  else carry_rows<unsigned short>(base, (int)e.pixels, e.bytes, e.stride, src);
}

// Bidirectional sequence mode: the decoder of the backward block concatenates its channels with conv2's output of the pair's
// FIRST frame, which for backward pair i is frame i + 1 — a row the tower wrote elsewhere.  unflow_sequence_mirror copies n
// consecutive sample rows [src0, src0 + n) to rows [dst0, dst0 + n) of every buffer of a list (the carry's descriptor; bytes <
// stride: one channel segment, the neighbouring channels of the destination rows stay).  Rows of a buffer are contiguous, so the
// n rows are ONE range of n * pixels pixels: a flat grid-stride copy, four independent 16-byte loads in flight per thread before
// the first store.  src0, dst0 and n are launch arguments (fixed per engine: a captured graph keeps them).
template <typename V>
__device__ __forceinline__ void mirror_rows(char* __restrict__ base, long row_pixels, int bytes, int stride, int src0, int dst0,
                                            int rows) {
  const unsigned per = (unsigned)bytes / (unsigned)sizeof(V);   // vectors per pixel
  const long n = (long)rows * row_pixels * per;                  // < 2^31 (the host checks)
  const char* from = base + (long)src0 * row_pixels * stride;
  char* to = base + (long)dst0 * row_pixels * stride;
  const long T = (long)gridDim.x * blockDim.x;
  auto off = [&](long i) {
    const unsigned px = (unsigned)i / per, c = (unsigned)i - px * per;
    return (long)px * stride + (long)c * (long)sizeof(V);
  };
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * T < n; i += 4 * T) {
    const long o0 = off(i), o1 = off(i + T), o2 = off(i + 2 * T), o3 = off(i + 3 * T);
    const V v0 = *reinterpret_cast<const V*>(from + o0);
    const V v1 = *reinterpret_cast<const V*>(from + o1);
    const V v2 = *reinterpret_cast<const V*>(from + o2);
    const V v3 = *reinterpret_cast<const V*>(from + o3);
    *reinterpret_cast<V*>(to + o0) = v0;
    *reinterpret_cast<V*>(to + o1) = v1;
    *reinterpret_cast<V*>(to + o2) = v2;
    *reinterpret_cast<V*>(to + o3) = v3;
  }
  for (; i < n; i += T) {
    const long o = off(i);
    *reinterpret_cast<V*>(to + o) = *reinterpret_cast<const V*>(from + o);
  }
}

__global__ __launch_bounds__(256) void sequence_mirror_kernel(CarryList list, int src0, int dst0, int rows) {
  const unflow_carry_buf e = list.b[blockIdx.y];
  char* base = reinterpret_cast<char*>(e.base);
  const unsigned long a = reinterpret_cast<unsigned long>(e.base) | (unsigned long)e.bytes | (unsigned long)e.stride;
  if ((a & 15) == 0) mirror_rows<uint4>(base, e.pixels, e.bytes, e.stride, src0, dst0, rows);
  else if ((a & 7) == 0) mirror_rows<uint2>(base, e.pixels, e.bytes, e.stride, src0, dst0, rows);
  else if ((a & 3) == 0) mirror_rows<unsigned>(base, e.pixels, e.bytes, e.stride, src0, dst0, rows);
  else mirror_rows<unsigned short>(base, e.pixels, e.bytes, e.stride, src0, dst0, rows);
}

}  // namespace

UNFLOW_API int unflow_sequence_mirror(const unflow_carry_buf* bufs, int n_bufs, int src0, int dst0, int n, int max_row,
                                      unflow_stream_t stream) {
  if (!bufs) return UNFLOW_ERR_NULL;
  if (n_bufs <= 0 || n_bufs > UNFLOW_CARRY_MAX || n < 1 || src0 < 0 || dst0 < 0) return UNFLOW_ERR_SHAPE;
  if ((long)src0 + n - 1 > max_row || (long)dst0 + n - 1 > max_row) return UNFLOW_ERR_SHAPE;     // a row the buffers do not have
  if ((src0 <= dst0 ? dst0 - src0 : src0 - dst0) < n) return UNFLOW_ERR_SHAPE;                   // overlapping ranges
  CarryList list{};
  long most = 0;
  for (int k = 0; k < n_bufs; k++) {
    const unflow_carry_buf& e = bufs[k];
    if (!e.base) return UNFLOW_ERR_NULL;
    if (e.pixels <= 0 || e.bytes <= 0 || e.stride < e.bytes) return UNFLOW_ERR_SHAPE;
    if (((reinterpret_cast<uintptr_t>(e.base) | (uintptr_t)e.bytes | (uintptr_t)e.stride) & 1) != 0) return UNFLOW_ERR_UNSUPPORTED;
    if (e.pixels * (long)n * (long)(e.bytes / 2) > 0x7fffffffL) return UNFLOW_ERR_SHAPE;
    list.b[k] = e;
    most = max(most, e.pixels * (long)n * (long)((e.bytes + 15) / 16));
  }
  // four vectors per thread and pass; at most 2048 workgroups over the whole list
  const dim3 grid(min(stream_grid((most + 3) / 4), max(1, 2048 / n_bufs)), n_bufs);
  sequence_mirror_kernel<<<grid, 256, 0, as_stream(stream)>>>(list, src0, dst0, n);
  return launch_status();
}

UNFLOW_API int unflow_sequence_carry(const unflow_carry_buf* bufs, int n_bufs, const int* src_row, int max_row,
                                     unflow_stream_t stream) {
  if (!bufs || !src_row) return UNFLOW_ERR_NULL;
  if (n_bufs <= 0 || n_bufs > UNFLOW_CARRY_MAX || max_row < 1) return UNFLOW_ERR_SHAPE;
  CarryList list{};
  long most = 0;
  for (int k = 0; k < n_bufs; k++) {
    const unflow_carry_buf& e = bufs[k];
    if (!e.base) return UNFLOW_ERR_NULL;
    if (e.pixels <= 0 || e.bytes <= 0 || e.stride < e.bytes) return UNFLOW_ERR_SHAPE;
    if (((reinterpret_cast<uintptr_t>(e.base) | (uintptr_t)e.bytes | (uintptr_t)e.stride) & 1) != 0) return UNFLOW_ERR_UNSUPPORTED;
    if (e.pixels * (long)(e.bytes / 2) > 0x7fffffffL) return UNFLOW_ERR_SHAPE;
    list.b[k] = e;
    most = max(most, e.pixels * (long)((e.bytes + 15) / 16));
  }
  const dim3 grid(min(stream_grid(most), 512), n_bufs);
  sequence_carry_kernel<<<grid, 256, 0, as_stream(stream)>>>(list, src_row, max_row);
  return launch_status();
}
