// A wave-uniform pointer into memory that nothing writes while the kernel runs, as the constant address space: the loads through it are
// scalar loads, issued where their values are used (see kernarg_lin_params, factor_stage.hpp).  How the batched kernels read their
// per-call tables (pass_layout.hpp: BatchPair; forest.hpp: ForestTree, ForestFeat).
#pragma once
#include <hip/hip_runtime.h>

namespace sga {
template <typename T>
__device__ __forceinline__ const T* uniform_const(const T* ptr) {
  using C = const __attribute__((address_space(4))) T;
  C* a = (C*)ptr;
  asm volatile("" : "+s"(a));
  return (const T*)a;
}
}  // namespace sga
