// TEST INFRASTRUCTURE ONLY: correlation_op.h includes this TensorFlow header and uses nothing from it.
#ifndef REF_SHIM_OP_H_
#define REF_SHIM_OP_H_

namespace tensorflow {}

#endif
