// One translation unit per warm-start instantiation of the whole-control-step kernel (ik_rollout.h, WARM): compiled with
//   -DPINKHIP_TU_NV=<NV> -DPINKHIP_TU_W=<W>       (Makefile, WROLLOUT list)
#include <hip/hip_runtime.h>

// clang-format off
#define PINKHIP_NO_ELEMENTWISE_KERNELS
#include "wave.h"
#include "ik_rollout.h"
#include "launchers.h"
// clang-format on

#if !defined(PINKHIP_TU_NV) || !defined(PINKHIP_TU_W)
#error "tu_wrollout.hip is compiled once per (NV, W): see the Makefile"
#endif

namespace pinkhip {

hipError_t PINKHIP_LAUNCH_WROLLOUT_NAME(PINKHIP_TU_NV, PINKHIP_TU_W)(hipStream_t stream, const RolloutArgs &a) {
  constexpr int NV = PINKHIP_TU_NV, W = PINKHIP_TU_W, G = kWave / W;
  static_assert(sweep_lds_doubles(NV, 0, W) == SweepLds<NV, 0, W>::stride, "dispatch.h restates the LDS layout");
  static_assert(packed_lds_doubles(NV, 0) == LdsP<NV>::stride(0), "dispatch.h restates the LDS layout");
  const size_t lds = 8 * static_cast<size_t>(a.k.lds_pitch) * G + 16;
  const dim3 grid(static_cast<unsigned>((a.k.B + G - 1) / G)), block(kWave);
  hipLaunchKernelGGL((ik_rollout_warm_kernel<NV, W>), grid, block, lds, stream, a);
  return hipGetLastError();
}

}  // namespace pinkhip
