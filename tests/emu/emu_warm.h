// Warm-start twins of the tableau kernels under the CPU wave emulator -- TEST INFRASTRUCTURE ONLY (see wave_emu.h).
// The per-lane entry points of ik_solve_sweep_warm_kernel / ik_rollout_warm_kernel (tu_wsweep.hip / tu_wrollout.hip),
// registered by emu_warm_part.cpp under KIND_SWEEP_WARM / KIND_ROLLOUT_WARM of emu_registry.h.
#pragma once
#include "emu_lanes.h"

namespace pinkemu {

template <int NV, int MD, int W>
void lane_main_sweep_warm(void *p) {
  KernelArgs k = *static_cast<const KernelArgs *>(p);
  k.lds_pitch = pinkhip::sweep_kernel_lds_doubles<NV, MD, W>(0);  // as tu_wsweep.hip's launcher
  pinkhip::ik_solve_sweep_body<NV, MD, W, true>(k, pinkhip::block_id());
}
template <int NV, int W>
void lane_main_rollout_warm(void *p) {
  pinkhip::ik_rollout_instance<NV, 0, W, true>(*static_cast<const pinkhip::RolloutArgs *>(p), pinkhip::block_id());
}

}  // namespace pinkemu
