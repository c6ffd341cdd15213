// TEST INFRASTRUCTURE ONLY: stand-in for the launch helpers the reference's GPU sources take from TensorFlow, on the HIP runtime.
// Every kernel that asks GetCudaLaunchConfig for a grid walks its work with CUDA_1D_KERNEL_LOOP, so any grid is correct; this one
// is capped at 256 threads x 4096 blocks.
#ifndef REF_SHIM_CUDA_KERNEL_HELPER_H_
#define REF_SHIM_CUDA_KERNEL_HELPER_H_

#include <hip/hip_runtime.h>

#include <tensorflow/core/framework/tensor_types.h>

#define cudaMemset hipMemset

#define CUDA_1D_KERNEL_LOOP(var, count)                                               \
  for (int var = (int)(blockIdx.x * blockDim.x + threadIdx.x); var < (int)(count);   \
       var += (int)(blockDim.x * gridDim.x))

namespace tensorflow {

struct CudaLaunchConfig {
  int virtual_thread_count;
  int thread_per_block;
  int block_count;
};

inline CudaLaunchConfig GetCudaLaunchConfig(int work, const Eigen::GpuDevice&) {
  CudaLaunchConfig cfg;
  cfg.virtual_thread_count = work;
  cfg.thread_per_block = 256;
  const int wanted = (work + 255) / 256;
  cfg.block_count = wanted < 1 ? 1 : (wanted > 4096 ? 4096 : wanted);
  return cfg;
}

template <typename T>
__device__ inline T CudaAtomicAdd(T* where, T what) {
  return atomicAdd(where, what);
}

template <typename T>
__global__ void SetZero(const int count, T* where) {
  CUDA_1D_KERNEL_LOOP(at, count) { where[at] = T(0); }
}

}  // namespace tensorflow

#endif
