// TEST INFRASTRUCTURE ONLY: the reference's GPU sources include this TensorFlow header and use nothing from it.
#ifndef REF_SHIM_REGISTER_TYPES_H_
#define REF_SHIM_REGISTER_TYPES_H_

namespace tensorflow {}

#endif
