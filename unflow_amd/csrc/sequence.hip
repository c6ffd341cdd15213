// Sequence inference (core/inference.py FlowEstimator(..., sequence=True)): the frame a clip's next replay starts from.
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

}  // namespace

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
