// TEST INFRASTRUCTURE ONLY: stand-in for the one name the reference's GPU sources take from this TensorFlow header.
// Written from the list of names those sources use; holds no TensorFlow text.
#ifndef REF_SHIM_PLATFORM_TYPES_H_
#define REF_SHIM_PLATFORM_TYPES_H_

namespace tensorflow {
typedef int int32;
}  // namespace tensorflow

#endif
