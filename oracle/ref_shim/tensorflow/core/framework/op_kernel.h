// TEST INFRASTRUCTURE ONLY: stand-in for what correlation_op.h takes from TensorFlow's op framework.  Its attribute constructor is
// never called here (oracle/ref_glue.hip fills CorrelationAttrs field by field), so the checking macros expand to nothing and the
// construction context is a name only.
#ifndef REF_SHIM_OP_KERNEL_H_
#define REF_SHIM_OP_KERNEL_H_

#include <cmath>

namespace tensorflow {
class OpKernelConstruction;
}  // namespace tensorflow

#define OP_REQUIRES(...)
#define OP_REQUIRES_OK(...)

#endif
