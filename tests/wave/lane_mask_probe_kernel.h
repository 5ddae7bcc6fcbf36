// The lane-mask primitives of pink_amd/csrc/wave.h -- lane_pred and the mask builders -- applied to one wave-uniform mask,
// one per-group bit field and one [64] predicate per wavefront, every lane's result stored -- TEST CODE ONLY
// (tests/test_lane_mask_primitives.py).  Included after wave.h (lane_mask_probe.hip: the inverse ballot) or after
// emu/wave_emu.h (emu/emu_lane_mask_probe.cpp: plain bit tests), so that both face the same NumPy reference.
//
// One workgroup of one wavefront per input set; every index below is (set, slot, lane) with slot a compile-time constant.
#pragma once
#include <utility>

namespace lanemaskprobe {

struct Args {
  const int *mask_lo, *mask_hi;  // [sets]: the two halves of the wave-uniform mask
  const int *bits;               // [sets]: per-group bit field (bit g = group g)
  const int *lane;               // [sets]: K in [0, W), the lane of mask_groups_of_lane
  const int *pred;               // [sets][64]: arbitrary per lane (its ballot is the mask of mask_groups_of_lane)
  const int *ival;               // [sets][64]: arbitrary per lane
  const int *keybits;            // [sets][64]: the bits of a float key (key32_packf against key32_packf_quiet)
  int *out;                      // [sets][slots(W)][64]
};

enum {
  S_LANE_PRED,        // lane_pred(mask)
  S_SELECT,           // lane_pred(mask) ? ival : ~ival  (the mask as the condition of a select)
  S_BRANCH,           // ival + 1 inside `if (lane_pred(mask))`, ival elsewhere  (... of a branch)
  S_BALLOT_LO,        // wave_ballot(lane_pred(mask)): the mask itself
  S_BALLOT_HI,
  S_GROUPS,           // lane_pred(mask_groups<W>(bits))
  S_GROUPS_OF_LANE,   // lane_pred(mask_groups_of_lane<W>(wave_ballot(pred), K))
  S_ON_COUNT,         // lanes_on(lane_pred(mask_groups<W>(bits))) { lanes of this group with pred set }, -1 where off
  S_KEY_PACKF,        // the bits of key32_packf(key, lane in group)
  S_KEY_QUIET,        // ... of key32_packf_quiet: the same bits for every key but a signalling NaN
  kFixed
};
// ... then two tables of W slots, slot J: lane_pred(mask_lane<W>(J)) and lane_pred(mask_lanes_below<W>(J)), and one slot
// for mask_lanes_below<W>(W)
enum { T_LANE, T_BELOW, kTables };
constexpr int slots(int W) { return kFixed + kTables * W + 1; }

template <class F, int... J>
__device__ __forceinline__ void for_each_lane(F &&f, std::integer_sequence<int, J...>) {
  (f(std::integral_constant<int, J>{}), ...);
}

template <int W>
__device__ __forceinline__ void probe_lane(const Args &a, long long set) {
  using namespace pinkhip;
  const int lane = lane_id();
  const long long in = set * kWave + lane;
  // (read per wavefront and made scalars: lane_pred wants a wave-uniform mask)
  const unsigned lo = static_cast<unsigned>(wave_uniform(a.mask_lo[set])), hi = static_cast<unsigned>(wave_uniform(a.mask_hi[set]));
  const unsigned long long mask = (static_cast<unsigned long long>(hi) << 32) | lo;
  const unsigned bits = static_cast<unsigned>(wave_uniform(a.bits[set]));
  const int K = wave_uniform(a.lane[set]) & (W - 1);
  const bool pred = a.pred[in] != 0;
  const int ival = a.ival[in];
  int *o = a.out + set * slots(W) * kWave + lane;

  const bool p = lane_pred(mask);
  o[S_LANE_PRED * kWave] = p ? 1 : 0;
  o[S_SELECT * kWave] = p ? ival : ~ival;
  int br = ival;
  if (p) br = ival + 1;
  o[S_BRANCH * kWave] = br;
  const unsigned long long back = wave_ballot(p);
  o[S_BALLOT_LO * kWave] = static_cast<int>(back & 0xffffffffull);
  o[S_BALLOT_HI * kWave] = static_cast<int>(back >> 32);
  const bool gon = lane_pred(mask_groups<W>(bits));
  o[S_GROUPS * kWave] = gon ? 1 : 0;
  o[S_GROUPS_OF_LANE * kWave] = lane_pred(mask_groups_of_lane<W>(wave_ballot(pred), K)) ? 1 : 0;
  // a body under lanes_on, written with selects on the predicate as wave.h asks (the emulator runs it in every lane)
  int cnt = -1;
  if (lanes_on(gon)) {
    const double c = group_sum<W>((gon && pred) ? 1.0 : 0.0);
    cnt = gon ? static_cast<int>(c) : cnt;
  }
  o[S_ON_COUNT * kWave] = cnt;
  float key;
  const int kb = a.keybits[in];
  __builtin_memcpy(&key, &kb, 4);
  const float k1 = key32_packf(key, lane & (W - 1)), k2 = key32_packf_quiet(key, lane & (W - 1));
  int b1, b2;
  __builtin_memcpy(&b1, &k1, 4);
  __builtin_memcpy(&b2, &k2, 4);
  o[S_KEY_PACKF * kWave] = b1;
  o[S_KEY_QUIET * kWave] = b2;

  int *t = o + kFixed * kWave;
  for_each_lane(
      [&](auto j) {
        constexpr int J = decltype(j)::value;
        t[(T_LANE * W + J) * kWave] = lane_pred(mask_lane<W>(J)) ? 1 : 0;
        t[(T_BELOW * W + J) * kWave] = lane_pred(mask_lanes_below<W>(J)) ? 1 : 0;
      },
      std::make_integer_sequence<int, W>{});
  t[(kTables * W) * kWave] = lane_pred(mask_lanes_below<W>(W)) ? 1 : 0;
}

}  // namespace lanemaskprobe
