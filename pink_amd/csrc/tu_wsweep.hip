// One translation unit per warm-start instantiation of the sweep-tableau stack + solve kernel (ik_sweep.h, WARM): compiled
// with  -DPINKHIP_TU_NV=<NV> -DPINKHIP_TU_MD=0 -DPINKHIP_TU_W=<W>       (Makefile, WSWEEP list)
#include <hip/hip_runtime.h>

// clang-format off
#include "wave.h"
#include "ik_sweep.h"
#include "launchers.h"
// clang-format on

#if !defined(PINKHIP_TU_NV) || !defined(PINKHIP_TU_MD) || !defined(PINKHIP_TU_W)
#error "tu_wsweep.hip is compiled once per (NV, 0, W): see the Makefile"
#endif

namespace pinkhip {

hipError_t PINKHIP_LAUNCH_WSWEEP_NAME(PINKHIP_TU_NV, PINKHIP_TU_MD, PINKHIP_TU_W)(hipStream_t stream, const KernelArgs &a) {
  constexpr int NV = PINKHIP_TU_NV, MD = PINKHIP_TU_MD, W = PINKHIP_TU_W, G = kWave / W;
  static_assert(MD == 0, "warm starts are box-only");
  const dim3 grid(static_cast<unsigned>((a.B + G - 1) / G)), block(kWave);
  // LDS: that of the cold twin (tu_sweep.hip)
  using SL = SweepLds<NV, MD, W>;
  static_assert(sweep_lds_doubles(NV, MD, W) == SL::stride, "dispatch.h restates the LDS layout");
  static_assert(NV <= W || sweep_kernel_lds_doubles<NV, MD, W>(0) >= SweepLds<(NV <= W ? NV : W), 0, W>::stride + 2 * W + 8, "LDS of the elimination");
  KernelArgs k = a;
  k.lds_pitch = sweep_kernel_lds_doubles<NV, MD, W>(0);
  const size_t lds = 8 * static_cast<size_t>(k.lds_pitch) * G + 16;
  hipLaunchKernelGGL((ik_solve_sweep_warm_kernel<NV, MD, W>), grid, block, lds, stream, k);
  return hipGetLastError();
}

}  // namespace pinkhip
