// conv_launch.h — how the convolution translation units (conv_igemm.hip, conv_patch.hip,
// conv_lowp.hip, conv_wgrad.hip) turn a run-time flag into a kernel instantiation and launch it.
#pragma once
#include "common.h"

#include <type_traits>

namespace unet_conv {

// f(std::true_type | std::false_type) for a run-time bool: how a launcher picks the ACT / bf16
// instantiation of its kernel
template <typename F>
int with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
template <typename F>
int with_bools(bool a, bool b, F&& f) {
  return with_bool(a, [&](auto ca) { return with_bool(b, [&](auto cb) { return f(ca, cb); }); });
}

// One launch of the kernel instantiation Kern: raises its dynamic-LDS limit (remembered per
// instantiation and device), goes through the recording hipLaunchKernelGGL and reports a failed
// launch under `label`.
template <auto Kern, typename... Args>
int launch_kernel(const char* label, dim3 grid, unsigned threads, size_t lds, hipStream_t stream,
                  const Args&... args) {
  if (lds) UNET_SET_DYN_LDS(Kern, lds);
  hipLaunchKernelGGL(Kern, grid, dim3(threads), lds, stream, args...);
  UNET_CHECK_LAUNCH(label);
  return UNET_OK;
}

}  // namespace unet_conv
