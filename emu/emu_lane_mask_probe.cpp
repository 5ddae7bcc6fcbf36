// The lane-mask probe of tests/wave/lane_mask_probe_kernel.h on the emulator's primitives (wave_emu.h: lane_pred is a bit
// test) -- TEST INFRASTRUCTURE ONLY.  Same entry as tests/wave/lane_mask_probe.hip, so tests/test_lane_mask_primitives.py
// holds both implementations to the same NumPy reference.
#include "wave_emu.h"
// clang-format off
#include "../tests/wave/lane_mask_probe_kernel.h"
// clang-format on

namespace {

template <int W>
void mask_probe_lane_main(void *p) {
  lanemaskprobe::probe_lane<W>(*static_cast<const lanemaskprobe::Args *>(p), pinkhip::block_id());
}

}  // namespace

extern "C" {

int pinkhip_emu_lane_mask_probe_slots(int W) { return lanemaskprobe::slots(W); }

int pinkhip_emu_lane_mask_probe_run(int W, int sets, const int *mask_lo, const int *mask_hi, const int *bits, const int *lane,
                                    const int *pred, const int *ival, const int *keybits, int *out) {
  if ((W != 16 && W != 32 && W != 64) || sets < 1) return -1;
  lanemaskprobe::Args a{mask_lo, mask_hi, bits, lane, pred, ival, keybits, out};
  const pinkhip::LaneFn fn = W == 16 ? mask_probe_lane_main<16> : W == 32 ? mask_probe_lane_main<32> : mask_probe_lane_main<64>;
  for (long long s = 0; s < sets; ++s) pinkhip::emu_run_block(s, fn, &a);
  return 0;
}

}  // extern "C"
