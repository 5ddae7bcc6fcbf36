// Whole-step kernels with sphere-pair rows under the CPU wave emulator -- TEST INFRASTRUCTURE ONLY (see wave_emu.h).
// The per-lane entry point of ik_rollout_pairs_kernel (tu_rpairs.hip), registered by the slices of emu_pairs_part.cpp in a
// registry of their own (emu_pairs.cpp): the key is the entry {NV, MD, W} of PINKHIP_RPAIRS_TABLE.
#pragma once
#include "emu_lanes.h"

namespace pinkemu {

void emu_pairs_register(int nv, int md, int w, LaneEntry fn);
LaneEntry emu_pairs_lookup(int nv, int md, int w);

template <int NV, int MD, int W>
void lane_main_rollout_pairs(void *p) {
  const pinkhip::RolloutPairsArgs *a = static_cast<const pinkhip::RolloutPairsArgs *>(p);
  pinkhip::ik_rollout_instance<NV, MD, W, false, true>(a->r, pinkhip::block_id(), &a->p);
}

}  // namespace pinkemu
