// The wave-primitive probe of tests/wave/wave_probe_kernel.h on the emulator's cross-lane primitives (wave_emu.h) --
// TEST INFRASTRUCTURE ONLY.  Same entry as tests/wave/wave_probe.hip, so tests/test_wave_primitives.py holds both
// implementations to the same NumPy reference.
#include "wave_emu.h"
// clang-format off
#include "../tests/wave/wave_probe_kernel.h"
// clang-format on

namespace {

template <int W>
void probe_lane_main(void *p) {
  waveprobe::probe_lane<W>(*static_cast<const waveprobe::Args *>(p), pinkhip::block_id());
}

}  // namespace

extern "C" {

int pinkhip_emu_wave_probe_slots_d(int W) { return waveprobe::slots_d(W); }
int pinkhip_emu_wave_probe_slots_i() { return waveprobe::kSlotsI; }

int pinkhip_emu_wave_probe_run(int W, int sets, const double *v, const double *x, const double *acc, const double *key,
                               const int *pred, const int *gsrc, const int *isrc, const int *lsrc, const int *gint,
                               const int *ival, const int *on, double *out_d, int *out_i) {
  if ((W != 8 && W != 16 && W != 32 && W != 64) || sets < 1) return -1;
  waveprobe::Args a{v, x, acc, key, pred, gsrc, isrc, lsrc, gint, ival, on, out_d, out_i};
  const pinkhip::LaneFn fn = W == 8 ? probe_lane_main<8> : W == 16 ? probe_lane_main<16> : W == 32 ? probe_lane_main<32> : probe_lane_main<64>;
  for (long long s = 0; s < sets; ++s) pinkhip::emu_run_block(s, fn, &a);
  return 0;
}

}  // extern "C"
