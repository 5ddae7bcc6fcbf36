// Per-lane entry points of the kernels under the CPU wave emulator -- TEST INFRASTRUCTURE ONLY (see wave_emu.h).
// The heavy instantiations (the families of dispatch.h's PINKHIP_FAMILIES) are compiled in emu_part.cpp, one slice of the
// tables per translation unit so that the slices build in parallel, and found through emu_registry.h.
#pragma once
#include "wave_emu.h"
// clang-format off
#include "../pink_amd/csrc/ik_common.h"
#include "../pink_amd/csrc/dispatch.h"
#include "../pink_amd/csrc/ik_kernels_packed.h"
#include "../pink_amd/csrc/ik_sweep.h"
#include "../pink_amd/csrc/ik_sweepx.h"
#include "../pink_amd/csrc/ik_stack_mfma.h"
#include "../pink_amd/csrc/ik_frame_task.h"
#include "../pink_amd/csrc/ik_kinematics.h"
#include "../pink_amd/csrc/ik_com.h"
#include "../pink_amd/csrc/ik_manip.h"
#include "../pink_amd/csrc/ik_rolling.h"
#include "../pink_amd/csrc/ik_rollout.h"
#include "../pink_amd/csrc/ik_barrier_rows.h"
#include "../pink_amd/csrc/model_tables.h"
#include "../pink_amd/csrc/host_tables.h"
// clang-format on

#include <string>

#include "emu_registry.h"

namespace pinkemu {

using pinkhip::KernelArgs;

// The per-lane entry point of an entry of the family of plans of KIND (dispatch.h PINKHIP_FAMILIES): the family's kernel
// (`__global__` is a plain function here) on the arguments as the library's launcher prepares them
template <int KIND, int NV, int MD, int W>
void lane_main(void *p) {
  using F = pinkhip::Family<KIND, NV, MD, W>;
  const typename F::Args &a = *static_cast<const typename F::Args *>(p);
  if constexpr (KIND == pinkhip::PLAN_PACKED) {  // (both DENSE variants behind one entry)
    if (a.md != 0) return pinkhip::Family<KIND, NV, MD, W, true>::kernel(a);
  }
  F::kernel(F::prepared(a));
}

template <int TP>
void lane_main_stack_small(void *p) {
  pinkhip::ik_stack_small_instance<TP>(*static_cast<const KernelArgs *>(p), pinkhip::block_id());
}

template <int NT>
void lane_main_stack_mfma(void *p) {
  const KernelArgs *a = static_cast<const KernelArgs *>(p);
  if constexpr (NT >= 3) {
    if (pinkhip::stack_staged_ok(a->nv, a->Kd, a->J)) {  // same rule as pinkhip.hip
      pinkhip::ik_stack_mfma_instance<NT, true>(*a, pinkhip::block_id());
      return;
    }
  }
  pinkhip::ik_stack_mfma_instance<NT>(*a, pinkhip::block_id());
}

template <int W>
void lane_main_frame(void *p) {
  pinkhip::ik_frame_task_instance<W>(*static_cast<const pinkhip::FrameTaskArgs *>(p), pinkhip::block_id());
}

template <int W>
void lane_main_fk(void *p) {
  pinkhip::ik_fk_instance<W>(*static_cast<const pinkhip::FkArgs *>(p), pinkhip::block_id());
}

template <int W>
void lane_main_fk_fused(void *p) {
  pinkhip::ik_fk_instance<W, true>(*static_cast<const pinkhip::FkArgs *>(p), pinkhip::block_id());
}

template <int W>
void lane_main_step(void *p) {
  pinkhip::ik_fk_instance<W, true, true>(*static_cast<const pinkhip::FkArgs *>(p), pinkhip::block_id());
}

template <int W>
void lane_main_com(void *p) {
  pinkhip::ik_com_instance<W>(*static_cast<const pinkhip::ComArgs *>(p), pinkhip::block_id());
}

template <int W>
void lane_main_manip(void *p) {
  pinkhip::ik_manip_instance<W>(*static_cast<const pinkhip::ManipArgs *>(p), pinkhip::block_id());
}

template <int W>
void lane_main_rolling(void *p) {
  pinkhip::ik_rolling_instance<W>(*static_cast<const pinkhip::RollingArgs *>(p), pinkhip::block_id());
}

template <int W>
void lane_main_barrier_rows(void *p) {
  pinkhip::ik_barrier_rows_instance<W>(*static_cast<const pinkhip::BarrierRowsArgs *>(p), pinkhip::block_id());
}

}  // namespace pinkemu
