// Every group primitive of pink_amd/csrc/wave.h applied to one [64] input per wavefront, every lane's result stored --
// TEST CODE ONLY (tests/test_wave_primitives.py).  Included after wave.h (wave_probe.hip: the device's DPP / permlane /
// bpermute / EXEC code) or after emu/wave_emu.h (emu/emu_wave_probe.cpp: the emulator's rendezvous of 64 lanes), so that
// both implementations face the same NumPy reference.
//
// One workgroup of one wavefront per input set.  Nothing a lane reads or writes is addressed through an input value: every
// index below is (set, slot, lane) with slot a compile-time constant.
#pragma once
#include <utility>

namespace waveprobe {

struct Args {
  // [sets][64] each
  const double *v, *x, *acc, *key;
  const int *pred;  // arbitrary per lane
  const int *gsrc;  // group-uniform, in [0, W): the source lane of group_bcast / group_bcast_i
  const int *isrc;  // group-uniform, in [-1, W): the lane of bcast_indicator (-1: none)
  const int *lsrc;  // arbitrary per lane, in [0, 64): the source lane of lane_shfl
  const int *gint;  // group-uniform: groups_max / groups_min, the factor of bcast_scale
  const int *ival;  // arbitrary per lane
  const int *on;    // group-uniform predicate: lanes_on, bcast_select
  double *out_d;    // [sets][slots_d(W)][64]
  int *out_i;       // [sets][kSlotsI][64]
};

// double slots
enum {
  D_GROUP_SUM,
  D_GROUP_MIN,
  D_GROUP_SCAN,
  D_GROUP_BCAST,
  D_LANE_SHFL,
  D_ROW_PAIR_A,
  D_ROW_PAIR_B,
  D_WAVE_SUM,
  D_WAVE_MIN,
  D_ON_SUM,   // lanes_on(on) { group_sum of the group's own values }, v where off
  D_ON_MIN,   // ... group_min
  D_ON_SCAN,  // ... group_scan_sum
  kFixedD
};
// ... then, for W >= 16 (broadcast-FMA groups are whole rows of 16 lanes), five tables of W slots, slot J = source lane J:
enum { T_VALUE, T_FMA, T_INDICATOR, T_SELECT, T_SCALE, kTables };
constexpr int slots_d(int W) { return kFixedD + (W >= 16 ? kTables * W : 0); }

enum {
  I_FIRST_LANE,
  I_GROUP_BCAST_I,
  I_GROUPS_MAX,
  I_GROUPS_MIN,
  I_WAVE_ANY,
  I_MIN32_PAYLOAD,
  I_MIN32_BITS,
  I_KEY32_BITS,  // key32_pack(key, lane in group) itself
  I_LANE_SHFL_I,
  I_BALLOT_LO,
  I_BALLOT_HI,
  I_ON_FIRST_LANE,  // lanes_on(on) { group_first_lane(pred) }, -1 where off
  kSlotsI
};

template <class F, int... J>
__device__ __forceinline__ void for_each_lane(F &&f, std::integer_sequence<int, J...>) {
  (f(std::integral_constant<int, J>{}), ...);
}

inline __device__ int float_bits(float f) {
  int b;
  __builtin_memcpy(&b, &f, 4);
  return b;
}

template <int W>
__device__ __forceinline__ void probe_lane(const Args &a, long long set) {
  using namespace pinkhip;
  const int lane = lane_id(), li = lane & (W - 1);
  const long long in = set * kWave + lane;
  const double v = a.v[in], x = a.x[in], acc = a.acc[in], key = a.key[in];
  const bool pred = a.pred[in] != 0, on = a.on[in] != 0;
  const int gsrc = a.gsrc[in], isrc = a.isrc[in], lsrc = a.lsrc[in] & (kWave - 1), gint = a.gint[in], ival = a.ival[in];
  double *od = a.out_d + set * slots_d(W) * kWave + lane;
  int *oi = a.out_i + set * kSlotsI * kWave + lane;

  od[D_GROUP_SUM * kWave] = group_sum<W>(v);
  od[D_GROUP_MIN * kWave] = group_min<W>(v);
  od[D_GROUP_SCAN * kWave] = group_scan_sum<W>(v);
  od[D_GROUP_BCAST * kWave] = group_bcast<W>(v, gsrc);
  od[D_LANE_SHFL * kWave] = lane_shfl(v, lsrc);
  double ra, rb;
  row_pair(v, ra, rb);
  od[D_ROW_PAIR_A * kWave] = ra;
  od[D_ROW_PAIR_B * kWave] = rb;
  od[D_WAVE_SUM * kWave] = wave_sum(v);
  od[D_WAVE_MIN * kWave] = wave_min(v);

  // a body under lanes_on: written with selects on `on` as wave.h asks (that is what the emulator runs), reduced inside
  // the groups that are on while the lanes of the others are switched off on the device
  double s_on = v, m_on = v, c_on = v;
  int f_on = -1;
  if (lanes_on(on)) {
    const double s = group_sum<W>(on ? v : 0.0);
    const double m = group_min<W>(on ? v : INFINITY);
    const double c = group_scan_sum<W>(on ? v : 0.0);
    const int f = group_first_lane<W>(on && pred);
    s_on = on ? s : s_on;
    m_on = on ? m : m_on;
    c_on = on ? c : c_on;
    f_on = on ? f : f_on;
  }
  od[D_ON_SUM * kWave] = s_on;
  od[D_ON_MIN * kWave] = m_on;
  od[D_ON_SCAN * kWave] = c_on;

  if constexpr (W >= 16) {
    const Bcast<W> bv = bcast_prepare<W>(v);
    const Bcast<W> bx = bcast_prepare<W>(x);
    const Bcast<W> bi = bcast_indicator<W>(isrc);
    const Bcast<W> bs = bcast_select<W>(on, bv, bx);
    const Bcast<W> bc = bcast_scale<W>(bv, static_cast<double>(gint));
    double *t = od + kFixedD * kWave;
    for_each_lane(
        [&](auto j) {
          constexpr int J = decltype(j)::value;
          t[(T_VALUE * W + J) * kWave] = value_bcast<W, J>(bv);
          t[(T_FMA * W + J) * kWave] = fma_bcast<W, J>(acc, bv, x);
          t[(T_INDICATOR * W + J) * kWave] = value_bcast<W, J>(bi);
          t[(T_SELECT * W + J) * kWave] = value_bcast<W, J>(bs);
          t[(T_SCALE * W + J) * kWave] = value_bcast<W, J>(bc);
        },
        std::make_integer_sequence<int, W>{});
  }

  oi[I_FIRST_LANE * kWave] = group_first_lane<W>(pred);
  oi[I_GROUP_BCAST_I * kWave] = group_bcast_i<W>(ival, gsrc);
  oi[I_GROUPS_MAX * kWave] = groups_max<W>(gint);
  oi[I_GROUPS_MIN * kWave] = groups_min<W>(gint);
  oi[I_WAVE_ANY * kWave] = wave_any(pred) ? 1 : 0;
  const float k32 = key32_pack(key, li);
  const float m32 = group_min32<W>(k32);
  oi[I_MIN32_PAYLOAD * kWave] = key32_payload(m32);
  oi[I_MIN32_BITS * kWave] = float_bits(m32);
  oi[I_KEY32_BITS * kWave] = float_bits(k32);
  oi[I_LANE_SHFL_I * kWave] = lane_shfl_i(ival, lsrc);
  const unsigned long long ballot = wave_ballot(pred);
  oi[I_BALLOT_LO * kWave] = static_cast<int>(ballot & 0xffffffffull);
  oi[I_BALLOT_HI * kWave] = static_cast<int>(ballot >> 32);
  oi[I_ON_FIRST_LANE * kWave] = f_on;
}

}  // namespace waveprobe
