// Launch plumbing shared by the units ("source layout"): the one place where a run-time window size becomes a template
// argument, and the per-device opt-in to more dynamic LDS than the default 64 KB.  It defines no kernel and includes no project header:
// the status codes of include/voxelba.h come first (vba_ctx.hpp includes both).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstddef>
#include <type_traits>

namespace vba {

constexpr int kMaxDevices = 64;            // devices whose opt-in is remembered

// f(std::integral_constant<int, W>{}) for the W in [LO, HI] equal to w, and its status; VBA_ERR_UNSUPPORTED_WINDOW, f not called, for
// any other w.  `constexpr int W = decltype(wc)::value;` in a generic lambda names the constant.
template <int LO, int HI, class F>
int for_window(int w, F &&f) {
  if constexpr (LO > HI) return VBA_ERR_UNSUPPORTED_WINDOW;
  else if (w == LO) return f(std::integral_constant<int, LO>{});
  else return for_window<LO + 1, HI>(w, f);
}

// hipFuncAttributeMaxDynamicSharedMemorySize of ONE kernel, asked for once per device (the attribute is per device, a process may
// hold contexts on several): a function-local static in front of the launch, one instance per kernel instantiation.  Contexts launch
// from several threads (vba_hba_global's workers), hence the atomics; two threads that both find the flag clear both ask, which is
// harmless.  A refused opt-in is returned and not remembered.  A device index outside [0, kMaxDevices) asks every time.
struct LdsOptIn {
  std::atomic<bool> done[kMaxDevices] = {};
  hipError_t operator()(int device, const void *kernel, size_t bytes) {
    const bool known = device >= 0 && device < kMaxDevices;
    if (known && done[device].load(std::memory_order_acquire)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (known && e == hipSuccess) done[device].store(true, std::memory_order_release);
    return e;
  }
};

}  // namespace vba
