// Host harness of the whole-step kernel with sphere-pair rows on the CPU wave emulator -- TEST INFRASTRUCTURE ONLY (see
// wave_emu.h).  Mirrors pinkhip_rollout_step_pairs_device on host memory: the library's own validation, argument fill and
// choice of instantiation (host_plan.h, plan_rollout_pairs), the emulator's block loop.
#include "emu_pairs.h"
#include "../../pink_amd/csrc/host_plan.h"

#include <cstdlib>
#include <map>
#include <string>
#include <tuple>

namespace pinkemu {
namespace {
std::map<std::tuple<int, int, int>, LaneEntry> &pairs_registry() {
  static std::map<std::tuple<int, int, int>, LaneEntry> r;
  return r;
}
}  // namespace
void emu_pairs_register(int nv, int md, int w, LaneEntry fn) { pairs_registry()[std::make_tuple(nv, md, w)] = fn; }
LaneEntry emu_pairs_lookup(int nv, int md, int w) {
  auto it = pairs_registry().find(std::make_tuple(nv, md, w));
  return it == pairs_registry().end() ? nullptr : it->second;
}
}  // namespace pinkemu

namespace {

std::string g_pairs_err;

// (what pinkhip_emu_model_create of emu_kernels.cpp hands out)
struct EmuModel {
  pinkhip::ModelImage image;
  pinkhip::ModelDev dev;
};

}  // namespace

extern "C" {
int pinkhip_emu_rollout_step_pairs(const pinkhip_desc *d, void *mp, const pinkhip_rollout_step *st, const pinkhip_sphere_pairs *sp) {
  if (!d || !mp || !st) {
    g_pairs_err = "null descriptor / model / args";
    return PINKHIP_E_INVALID;
  }
  const EmuModel *m = static_cast<const EmuModel *>(mp);
  int rc = pinkhip::pairs_fault(*d, sp, g_pairs_err);
  if (rc) return rc;
  pinkhip::HostTables t;
  pinkhip::RolloutPairsArgs pa{};
  pinkhip::LaunchPlan p;
  g_pairs_err = pinkhip::build_tables(*d, t);
  if (!g_pairs_err.empty()) return PINKHIP_E_INVALID;
  pinkhip::fill_desc(*d, t, pinkhip::host_table_ptrs(t), pa.r.k);
  rc = pinkhip::plan_rollout_pairs(*d, m->dev, m->image.has_relative, *st, sp, std::getenv("PINKHIP_SOLVER"), pa, p, g_pairs_err);
  if (rc) return rc;
  if (p.kind == pinkhip::PLAN_NONE) return PINKHIP_OK;
  const pinkhip::LaneFn fn = pinkemu::emu_pairs_lookup(p.NV, p.MD, p.W);
  if (!fn) {
    g_pairs_err = "the emulator has no entry point for the planned instantiation";
    return PINKHIP_E_INVALID;
  }
  for (long long b = 0; b < p.blocks; ++b) pinkhip::emu_run_block(b, fn, &pa);
  return PINKHIP_OK;
}
// Test infrastructure: the plan of that call -- out = {kind (host_plan.h PlanKind), NV, MD, W, dense, blocks}; nothing runs
int pinkhip_emu_plan_rollout_pairs(const pinkhip_desc *d, void *mp, const pinkhip_rollout_step *st, const pinkhip_sphere_pairs *sp, int out[6]) {
  if (!d || !mp || !st) {
    g_pairs_err = "null descriptor / model / args";
    return PINKHIP_E_INVALID;
  }
  const EmuModel *m = static_cast<const EmuModel *>(mp);
  pinkhip::HostTables t;
  pinkhip::RolloutPairsArgs pa{};
  pinkhip::LaunchPlan p;
  g_pairs_err = pinkhip::build_tables(*d, t);
  if (!g_pairs_err.empty()) return PINKHIP_E_INVALID;
  pinkhip::fill_desc(*d, t, pinkhip::host_table_ptrs(t), pa.r.k);
  const int rc = pinkhip::plan_rollout_pairs(*d, m->dev, m->image.has_relative, *st, sp, std::getenv("PINKHIP_SOLVER"), pa, p, g_pairs_err);
  if (rc) return rc;
  const int v[6] = {p.kind, p.NV, p.MD, p.W, p.dense, static_cast<int>(p.blocks)};
  for (int i = 0; i < 6; ++i) out[i] = v[i];
  return PINKHIP_OK;
}
const char *pinkhip_emu_pairs_last_error(void) { return g_pairs_err.c_str(); }
}
