// Host side of a launch: dispatch.h plus the two helpers that need HIP types.
#pragma once
#include <hip/hip_runtime.h>
#include "dispatch.h"

namespace mlgnn {

inline hipStream_t as_stream(void* stream) { return static_cast<hipStream_t>(stream); }

// raise the kernel's dynamic-LDS limit to `bytes` (needed above 64 KiB); the caller returns a failure
template <class K>
hipError_t allow_dynamic_lds(K kernel, int bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

}  // namespace mlgnn
