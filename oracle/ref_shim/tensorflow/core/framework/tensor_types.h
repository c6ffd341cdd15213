// TEST INFRASTRUCTURE ONLY: stand-in for TTypes<T, 4>::Tensor / ConstTensor and the two Eigen device names.  The reference's GPU
// sources touch a tensor only through data(), dimension(i) and size(), and the device only through stream().
#ifndef REF_SHIM_TENSOR_TYPES_H_
#define REF_SHIM_TENSOR_TYPES_H_

#include <hip/hip_runtime.h>

namespace Eigen {
struct ThreadPoolDevice {};
struct GpuDevice {
  hipStream_t queue;
  hipStream_t stream() const { return queue; }
};
}  // namespace Eigen

namespace tensorflow {

template <typename T, int RANK>
struct RefShimView {
  T* base;
  long extent[RANK];
  T* data() const { return base; }
  long dimension(int axis) const { return extent[axis]; }
  long size() const {
    long total = 1;
    for (int axis = 0; axis < RANK; axis++) total *= extent[axis];
    return total;
  }
};

template <typename T, int RANK>
struct TTypes {
  typedef RefShimView<T, RANK> Tensor;
  typedef RefShimView<const T, RANK> ConstTensor;
};

}  // namespace tensorflow

#endif
