// Host harness that runs the HIP kernel source on the CPU wave emulator.
// TEST INFRASTRUCTURE ONLY (see wave_emu.h).  Exposes the same struct-based
// signature as the host entry points of include/pinkhip.h.
#include "emu_lanes.h"
#include "../pink_amd/csrc/host_plan.h"

#include <cstdlib>
#include <map>
#include <string>
#include <tuple>

namespace pinkemu {
namespace {
std::map<std::tuple<int, int, int, int>, LaneEntry> &registry() {
  static std::map<std::tuple<int, int, int, int>, LaneEntry> r;
  return r;
}
}  // namespace
void emu_register(int kind, int nv, int md, int w, LaneEntry fn) { registry()[std::make_tuple(kind, nv, md, w)] = fn; }
LaneEntry emu_lookup(int kind, int nv, int md, int w) {
  auto it = registry().find(std::make_tuple(kind, nv, md, w));
  return it == registry().end() ? nullptr : it->second;
}
}  // namespace pinkemu

using namespace pinkemu;

namespace {

using pinkhip::KernelArgs;
using pinkhip::LaunchPlan;

std::string g_err;

struct EmuModel {
  pinkhip::ModelImage image;
  pinkhip::ModelDev dev;
};

struct EmuCom {
  pinkhip::ComImage image;
  pinkhip::ComDev dev;
};

// The descriptor part of the kernel arguments, as prepare() of pinkhip.hip fills it: here the tables stay where
// build_tables put them (`t` must outlive the run)
int prepare(const pinkhip_desc *d, pinkhip::HostTables &t, KernelArgs &a) {
  if (!d) {
    g_err = "null descriptor";
    return PINKHIP_E_INVALID;
  }
  g_err = pinkhip::build_tables(*d, t);
  if (!g_err.empty()) return PINKHIP_E_INVALID;
  pinkhip::fill_desc(*d, t, pinkhip::host_table_ptrs(t), a);
  return PINKHIP_OK;
}

// The per-lane entry point of a plan (NULL: none -- an error, as a plan without a launcher is in the library)
pinkhip::LaneFn entry_of(const LaunchPlan &p) {
  switch (p.kind) {
    case pinkhip::PLAN_STACK_SMALL: return p.W == 8 ? lane_main_stack_small<4> : lane_main_stack_small<1>;
    case pinkhip::PLAN_STACK_MFMA:
      switch (p.NV / 16) {
        case 1: return lane_main_stack_mfma<1>;
        case 2: return lane_main_stack_mfma<2>;
        case 3: return lane_main_stack_mfma<3>;
        case 4: return lane_main_stack_mfma<4>;
      }
      return nullptr;
    default: return emu_lookup(p.kind, p.NV, p.MD, p.W);  // (the table families; packed: both DENSE variants behind one entry)
  }
}

int run_plan(const LaunchPlan &p, void *args) {
  if (p.kind == pinkhip::PLAN_NONE) return PINKHIP_OK;
  const pinkhip::LaneFn fn = entry_of(p);
  if (!fn) {
    g_err = "the emulator has no entry point for the planned instantiation";
    return PINKHIP_E_INVALID;
  }
  for (long long b = 0; b < p.blocks; ++b) pinkhip::emu_run_block(b, fn, args);
  return PINKHIP_OK;
}

// The kinematics kernels: one group of `width` lanes per robot, the smallest of 8 / 32 / 64 that holds them (launch_grouped
// of pinkhip.hip)
int run_fk(int width, long long B, pinkhip::LaneFn fn8, pinkhip::LaneFn fn32, pinkhip::LaneFn fn64, void *args) {
  const int per = width <= 8 ? 8 : width <= 32 ? 2 : 1;
  const pinkhip::LaneFn fn = width <= 8 ? fn8 : width <= 32 ? fn32 : fn64;
  for (long long b = 0; b < (B + per - 1) / per; ++b) pinkhip::emu_run_block(b, fn, args);
  return PINKHIP_OK;
}

// Stack + solve as pinkhip_solve_device / pinkhip_solve_warm_device (warm_call) run it, on host memory
int solve(const pinkhip_desc *d, const pinkhip_problem *in, const pinkhip_result *out, bool warm_call, const pinkhip_warm *warm) {
  pinkhip::HostTables t;
  KernelArgs a{};
  LaunchPlan p;
  int rc = prepare(d, t, a);
  if (!rc) rc = pinkhip::set_solve(*d, in, out, warm_call, warm, a, g_err);
  if (!rc) rc = pinkhip::plan_solve(a, std::getenv("PINKHIP_SOLVER"), std::getenv("PINKHIP_FORCE_DENSE") != nullptr, warm_call, p, g_err);
  return rc ? rc : run_plan(p, &a);
}

// The whole control step as pinkhip_rollout_step_device / pinkhip_rollout_step_warm_device run it
int rollout_step(const pinkhip_desc *d, void *mp, const pinkhip_rollout_step *st, const pinkhip_warm *warm) {
  if (!mp || !st) {
    g_err = "null handle / model / args";
    return PINKHIP_E_INVALID;
  }
  const EmuModel *m = static_cast<const EmuModel *>(mp);
  pinkhip::HostTables t;
  pinkhip::RolloutArgs ra{};
  LaunchPlan p;
  int rc = prepare(d, t, ra.k);
  if (!rc) rc = pinkhip::plan_rollout(*d, m->dev, m->image.has_relative, *st, warm, std::getenv("PINKHIP_SOLVER"), ra, p, g_err);
  return rc ? rc : run_plan(p, &ra);
}

// The whole control step with sphere-pair rows as pinkhip_rollout_step_pairs_device plans it (+ run: and runs it)
int rollout_step_pairs(const pinkhip_desc *d, void *mp, const pinkhip_rollout_step *st, const pinkhip_sphere_pairs *sp, bool run, LaunchPlan &p) {
  if (!d || !mp || !st) {
    g_err = "null descriptor / model / args";
    return PINKHIP_E_INVALID;
  }
  const EmuModel *m = static_cast<const EmuModel *>(mp);
  int rc = run ? pinkhip::pairs_fault(*d, sp, g_err) : 0;  // (before the descriptor's tables are touched, as the library)
  if (rc) return rc;
  pinkhip::HostTables t;
  pinkhip::RolloutPairsArgs pa{};
  rc = prepare(d, t, pa.r.k);
  if (!rc) rc = pinkhip::plan_rollout_pairs(*d, m->dev, m->image.has_relative, *st, sp, std::getenv("PINKHIP_SOLVER"), pa, p, g_err);
  return rc || !run ? rc : run_plan(p, &pa);
}

void plan_out(const LaunchPlan &p, int out[6]) {
  const int v[6] = {p.kind, p.NV, p.MD, p.W, p.dense, static_cast<int>(p.blocks)};
  for (int i = 0; i < 6; ++i) out[i] = v[i];
}

}  // namespace

extern "C" {
// kinematics entry points mirroring pinkhip_model_create / _fk_device / ... on host memory
int pinkhip_emu_model_create(const pinkhip_model_desc *d, void **out) {
  EmuModel *m = new EmuModel();
  g_err = pinkhip::build_model_image(*d, m->image);
  if (!g_err.empty()) {
    delete m;
    return PINKHIP_E_INVALID;
  }
  m->dev = pinkhip::model_view<pinkhip::ModelDev>(m->image, m->image.bytes.data());
  *out = m;
  return PINKHIP_OK;
}
int pinkhip_emu_model_destroy(void *m) {
  delete static_cast<EmuModel *>(m);
  return PINKHIP_OK;
}
int pinkhip_emu_fk(void *mp, long long B, const double *q, double *T_frames, double *J_body) {
  EmuModel *m = static_cast<EmuModel *>(mp);
  pinkhip::FkArgs a{m->dev, B, q, T_frames, J_body};
  return run_fk(pinkhip::fk_group_width(m->dev), B, lane_main_fk<8>, lane_main_fk<32>, lane_main_fk<64>, &a);
}
int pinkhip_emu_fk_frame_tasks(void *mp, long long B, const double *q, const double *T_target, double *T_frames,
                               double *e, long long sE, double *J, long long sJ) {
  EmuModel *m = static_cast<EmuModel *>(mp);
  pinkhip::FkArgs a{m->dev, B, q, T_frames, nullptr};
  a.T_target = T_target;
  a.e_out = e;
  a.J_out = J;
  a.sE = sE;
  a.sJo = sJ;
  return run_fk(pinkhip::fk_group_width(m->dev), B, lane_main_fk_fused<8>, lane_main_fk_fused<32>, lane_main_fk_fused<64>, &a);
}
// centre-of-mass rows, mirroring pinkhip_com_create / _com_destroy / _com_task_device on host memory
int pinkhip_emu_com_create(void *mp, int nj, const double *mass, const double *com, void **out) {
  if (!mp || !out) return pinkhip::refuse(g_err, PINKHIP_E_INVALID, "null model / out");
  *out = nullptr;
  const EmuModel *m = static_cast<const EmuModel *>(mp);
  EmuCom *c = new EmuCom();
  const int *parent = reinterpret_cast<const int *>(m->image.bytes.data() + m->image.off_parent);
  const int rc = pinkhip::build_com_image(m->image.nj, parent, nj, mass, com, c->image, g_err);
  if (rc) {
    delete c;
    return rc;
  }
  c->dev = pinkhip::com_view(c->image, c->image.bytes.data());
  *out = c;
  return PINKHIP_OK;
}
// Test infrastructure: pinkhip_com_create's checks on a tree given as its parent array, without a device model in front of
// them (a model of more than 64 joints cannot be created: nv <= PINKHIP_MAX_NV)
int pinkhip_emu_com_image_check(int model_nj, const int *parent, int nj, const double *mass, const double *com) {
  pinkhip::ComImage im;
  g_err.clear();
  return pinkhip::build_com_image(model_nj, parent, nj, mass, com, im, g_err);
}
int pinkhip_emu_com_destroy(void *c) {
  delete static_cast<EmuCom *>(c);
  return PINKHIP_OK;
}
int pinkhip_emu_com_task(void *mp, void *cp, long long B, const double *q, const double *target, int target_batched, double *e,
                         long long sE, double *J, long long sJ, int row0, double *com_out) {
  if (!mp || !cp) return pinkhip::refuse(g_err, PINKHIP_E_INVALID, "null handle / model / mass tables");
  const EmuModel *m = static_cast<const EmuModel *>(mp);
  const EmuCom *c = static_cast<const EmuCom *>(cp);
  if (c->image.nj != m->dev.nj) return pinkhip::refuse(g_err, PINKHIP_E_INVALID, "mass tables of another model");
  pinkhip::ComArgs a{m->dev, c->dev, B, q, target, target_batched, e, J, sE, sJ, row0, com_out};
  if (const char *bad = pinkhip::com_task_fault(a)) return pinkhip::refuse(g_err, PINKHIP_E_INVALID, bad);
  if (B == 0) return PINKHIP_OK;
  return run_fk(pinkhip::fk_group_width(m->dev), B, lane_main_com<8>, lane_main_com<32>, lane_main_com<64>, &a);
}
// the ManipulabilityTask row, mirroring pinkhip_manipulability_task_device on host memory
int pinkhip_emu_manipulability_task(void *mp, long long B, const double *q, int frame, int reference_frame, int row_mask, double rate,
                                    double *e, long long sE, double *J, long long sJ, int row0, double *m_out) {
  if (!mp) return pinkhip::refuse(g_err, PINKHIP_E_INVALID, "null handle / model");
  const EmuModel *m = static_cast<const EmuModel *>(mp);
  pinkhip::ManipArgs a{m->dev, B, q, frame, reference_frame, row_mask, __builtin_popcount(row_mask & 63), rate, e, J, sE, sJ, row0, m_out};
  if (const char *bad = pinkhip::manip_task_fault(a)) return pinkhip::refuse(g_err, PINKHIP_E_INVALID, bad);
  if (const char *bad = pinkhip::manip_path_fault(m->dev.nj, m->dev.parent, m->dev.jtype, m->dev.frame_joint[frame]))
    return pinkhip::refuse(g_err, PINKHIP_E_UNSUPPORTED, bad);
  if (B == 0) return PINKHIP_OK;
  return run_fk(pinkhip::fk_group_width(m->dev), B, lane_main_manip<8>, lane_main_manip<32>, lane_main_manip<64>, &a);
}
// Test infrastructure: the path check on a tree given as its tables, without a device model in front of it (a model of more
// than 64 joints cannot be created: nv <= PINKHIP_MAX_NV)
int pinkhip_emu_manipulability_path_check(int nj, const int *parent, const int *jtype, int frame_joint) {
  g_err.clear();
  if (const char *bad = pinkhip::manip_path_fault(nj, parent, jtype, frame_joint)) return pinkhip::refuse(g_err, PINKHIP_E_UNSUPPORTED, bad);
  return PINKHIP_OK;
}
// the RollingTask / OmniwheelTask rows, mirroring pinkhip_rolling_tasks_device on host memory
int pinkhip_emu_rolling_tasks(void *mp, long long B, const double *q, int n, const int *slot, const int *kind, const double *radius,
                              double *e, long long sE, double *J, long long sJ, int row0, double *height_out) {
  if (!mp) return pinkhip::refuse(g_err, PINKHIP_E_INVALID, "null handle / model");
  const EmuModel *m = static_cast<const EmuModel *>(mp);
  pinkhip::RollingArgs a{m->dev, B, q, 0, {}, {}, {}, e, J, sE, sJ, row0, height_out};
  if (const char *bad = pinkhip::rolling_set_wheels(a, n, slot, kind, radius)) return pinkhip::refuse(g_err, PINKHIP_E_INVALID, bad);
  int code = PINKHIP_E_INVALID;
  if (const char *bad = pinkhip::rolling_task_fault(a, m->dev.frame_root_joint, code)) return pinkhip::refuse(g_err, code, bad);
  if (B == 0) return PINKHIP_OK;
  return run_fk(pinkhip::rolling_group_width(m->dev.nj), B, lane_main_rolling<8>, lane_main_rolling<32>, lane_main_rolling<64>, &a);
}
// Test infrastructure: the joint-count refusal on a bare count, without a device model in front of it (a model of more than
// 64 joints cannot be created: nv <= PINKHIP_MAX_NV)
int pinkhip_emu_rolling_joint_check(int nj) {
  g_err.clear();
  pinkhip::RollingArgs a{};
  a.m.nj = nj;
  a.m.nf = 1;
  a.n = 1;
  a.radius[0] = 0.1;
  const int root_joint[1] = {-1};
  int code = PINKHIP_OK;
  if (const char *bad = pinkhip::rolling_task_fault(a, root_joint, code)) return pinkhip::refuse(g_err, code, bad);
  return PINKHIP_OK;
}
// the barrier rows, mirroring pinkhip_barrier_rows_device on host memory
int pinkhip_emu_barrier_rows(void *mp, long long B, const double *q, double dt, const pinkhip_barrier_rows *rows,
                             const pinkhip_sphere_pairs *pairs, double *Gd, long long sG, double *hd, long long sH, int row0, double *dist_out) {
  if (!mp) return pinkhip::refuse(g_err, PINKHIP_E_INVALID, "null handle / model");
  const EmuModel *m = static_cast<const EmuModel *>(mp);
  pinkhip::BarrierRowsArgs a;
  if (const int rc = pinkhip::plan_barrier_rows(m->dev, B, q, dt, rows, pairs, Gd, sG, hd, sH, row0, dist_out, a, g_err)) return rc;
  if (B == 0) return PINKHIP_OK;
  return run_fk(pinkhip::barrier_rows_group_width(m->dev.nj), B, lane_main_barrier_rows<8>, lane_main_barrier_rows<32>, lane_main_barrier_rows<64>, &a);
}
// Test infrastructure: the joint-count refusal on a bare count, without a device model in front of it (a model of more than
// 64 joints cannot be created: nv <= PINKHIP_MAX_NV)
int pinkhip_emu_barrier_rows_joint_check(int nj) {
  g_err.clear();
  pinkhip::ModelDev md{};
  md.nj = nj;
  md.nv = 1;
  const int frame[1] = {0};
  const double one[1] = {1.0};
  pinkhip_barrier_rows rows{1, frame, frame, frame, one, one, one};
  pinkhip::BarrierRowsArgs a;
  return pinkhip::plan_barrier_rows(md, 0, nullptr, 1e-3, &rows, nullptr, nullptr, 0, nullptr, 0, 0, nullptr, a, g_err);
}
int pinkhip_emu_step(void *mp, long long B, const pinkhip_step *st) {
  EmuModel *m = static_cast<EmuModel *>(mp);
  pinkhip::FkArgs a = pinkhip::step_args(m->dev, B, *st);
  return run_fk(pinkhip::fk_group_width(m->dev), B, lane_main_step<8>, lane_main_step<32>, lane_main_step<64>, &a);
}
int pinkhip_emu_rollout_step(const pinkhip_desc *d, void *mp, const pinkhip_rollout_step *st) { return rollout_step(d, mp, st, nullptr); }
int pinkhip_emu_rollout_step_warm(const pinkhip_desc *d, void *mp, const pinkhip_rollout_step *st, const pinkhip_warm *warm) {
  if (!warm) {
    g_err = "null warm-start arguments";
    return PINKHIP_E_INVALID;
  }
  return rollout_step(d, mp, st, warm);
}
int pinkhip_emu_limits_posture(void *mp, long long B, double dt, double gain, const double *q,
                               const double *q_target, int target_batched, double *lb, double *ub, double *e,
                               int K, int e_off) {
  EmuModel *m = static_cast<EmuModel *>(mp);
  pinkhip::LimitsPostureArgs a{m->dev, B, dt, gain, q, q_target, target_batched, lb, ub, e, K, e_off};
  for (long long t = 0; t < B * m->dev.nv; ++t) pinkhip::ik_limits_posture_thread(a, t);
  return PINKHIP_OK;
}
int pinkhip_emu_check_limits(void *mp, long long B, const double *q, double tol, long long *first_bad) {
  EmuModel *m = static_cast<EmuModel *>(mp);
  // the device kernel takes an atomic minimum over its threads; in a plain loop the first hit is the minimum
  *first_bad = -1;
  const int start = m->image.root_nv == 6 ? 7 : m->image.root_nv;
  for (long long t = 0; t < B * m->dev.nq && *first_bad < 0; ++t) {
    const int i = static_cast<int>(t % m->dev.nq);
    if (i < start) continue;
    const double lo = m->dev.q_min[i], up = m->dev.q_max[i];
    if (up > lo + tol && (q[t] < lo - tol || q[t] > up + tol)) *first_bad = t;
  }
  return PINKHIP_OK;
}
int pinkhip_emu_integrate(void *mp, long long B, double *q, const double *dq) {
  EmuModel *m = static_cast<EmuModel *>(mp);
  pinkhip::IntegrateArgs a{m->dev, B, q, dq};
  for (long long t = 0; t < B * m->dev.nj; ++t) pinkhip::ik_integrate_thread(a, t);
  return PINKHIP_OK;
}
int pinkhip_emu_pose_targets(long long B, const double *pq, double *T) {
  pinkhip::PoseTargetsArgs a{B, pq, T};
  for (long long t = 0; t < B; ++t) pinkhip::ik_pose_targets_thread(a, t);
  return PINKHIP_OK;
}
int pinkhip_emu_integrate_checked(void *mp, long long B, double *q, const double *dq, const int *status,
                                  int *first_failure, int step) {
  EmuModel *m = static_cast<EmuModel *>(mp);
  pinkhip::IntegrateArgs a{m->dev, B, q, dq, status, first_failure, step};
  for (long long t = 0; t < B * m->dev.nj; ++t) pinkhip::ik_integrate_thread(a, t);
  return PINKHIP_OK;
}
int pinkhip_emu_frame_task_strided(long long B, int nv, const double *T_frame, long long sTf, const double *T_target,
                                   long long sTt, const double *J_body, long long sJb, double *e_out, long long sE,
                                   double *J_out, long long sJo) {
  pinkhip::FrameTaskArgs a{B, nv, T_frame, T_target, J_body, e_out, J_out, sTf, sTt, sJb, sE, sJo};
  pinkhip::LaneFn fn;
  int G;
  if (nv <= 8) { fn = lane_main_frame<8>; G = 8; }
  else if (nv <= 16) { fn = lane_main_frame<16>; G = 4; }
  else if (nv <= 32) { fn = lane_main_frame<32>; G = 2; }
  else { fn = lane_main_frame<64>; G = 1; }
  for (long long b = 0; b < (B + G - 1) / G; ++b) pinkhip::emu_run_block(b, fn, &a);
  return PINKHIP_OK;
}
int pinkhip_emu_frame_task_host(long long B, int nv, const double *T_frame, const double *T_target,
                                const double *J_body, double *e_out, double *J_out) {
  return pinkhip_emu_frame_task_strided(B, nv, T_frame, 0, T_target, 0, J_body, 0, e_out, 0, J_out, 0);  // (0: densely packed)
}
int pinkhip_emu_solve_host(const pinkhip_desc *d, const pinkhip_problem *in, const pinkhip_result *out) { return solve(d, in, out, false, nullptr); }
int pinkhip_emu_solve_warm_host(const pinkhip_desc *d, const pinkhip_problem *in, const pinkhip_result *out, const pinkhip_warm *warm) {
  return solve(d, in, out, true, warm);
}
int pinkhip_emu_stack_host(const pinkhip_desc *d, const pinkhip_problem *in, double *H_out, double *c_out) {
  pinkhip::HostTables t;
  KernelArgs a{};
  LaunchPlan p;
  int rc = prepare(d, t, a);
  if (rc) return rc;
  const char *bad = pinkhip::problem_fault(*d, in);
  if (!bad && d->B > 0 && (!H_out || !c_out)) bad = "H_out/c_out must not be NULL";
  if (bad) return pinkhip::refuse(g_err, PINKHIP_E_INVALID, bad);
  pinkhip::set_problem(a, *in);
  a.H_out = H_out;
  a.c_out = c_out;
  // (the library switches to four tiles per wave at B >= 65536; the emulator exercises both on small batches)
  rc = pinkhip::plan_stack(a, (d->B % 2) == 1, p, g_err);
  return rc ? rc : run_plan(p, &a);
}
// Test infrastructure: the plan of a stack + solve call for `d` under the current PINKHIP_SOLVER / PINKHIP_FORCE_DENSE --
// out = {kind (host_plan.h PlanKind), NV, MD, W, dense, blocks}
int pinkhip_emu_plan_solve(const pinkhip_desc *d, int out[6]) {
  pinkhip::HostTables t;
  KernelArgs a{};
  LaunchPlan p;
  int rc = prepare(d, t, a);
  if (!rc) rc = pinkhip::plan_solve(a, std::getenv("PINKHIP_SOLVER"), std::getenv("PINKHIP_FORCE_DENSE") != nullptr, false, p, g_err);
  if (!rc) plan_out(p, out);
  return rc;
}
// ... of a whole control step (warm: its warm-start twin, NULL: pinkhip_rollout_step_device), in the same form; nothing runs
int pinkhip_emu_plan_rollout(const pinkhip_desc *d, void *mp, const pinkhip_rollout_step *st, const pinkhip_warm *warm, int out[6]) {
  if (!d || !mp || !st) {
    g_err = "null descriptor / model / args";
    return PINKHIP_E_INVALID;
  }
  const EmuModel *m = static_cast<const EmuModel *>(mp);
  pinkhip::HostTables t;
  pinkhip::RolloutArgs ra{};
  LaunchPlan p;
  int rc = prepare(d, t, ra.k);
  if (!rc) rc = pinkhip::plan_rollout(*d, m->dev, m->image.has_relative, *st, warm, std::getenv("PINKHIP_SOLVER"), ra, p, g_err);
  if (!rc) plan_out(p, out);
  return rc;
}
int pinkhip_emu_rollout_step_pairs(const pinkhip_desc *d, void *mp, const pinkhip_rollout_step *st, const pinkhip_sphere_pairs *sp) {
  LaunchPlan p;
  return rollout_step_pairs(d, mp, st, sp, true, p);
}
// ... the plan of that call, in the same form; nothing runs
int pinkhip_emu_plan_rollout_pairs(const pinkhip_desc *d, void *mp, const pinkhip_rollout_step *st, const pinkhip_sphere_pairs *sp, int out[6]) {
  LaunchPlan p;
  const int rc = rollout_step_pairs(d, mp, st, sp, false, p);
  if (!rc) plan_out(p, out);
  return rc;
}
// Test infrastructure: the tables of PINKHIP_FAMILIES as this library was compiled with them, one line per entry --
// "<prefix> <kind> <dense> <NV> <MD> <W> <1: emu_lookup finds a lane entry for it and has_entry knows it>"
const char *pinkhip_emu_table_text(void) {
  static std::string text;
  text.clear();
#define PINKHIP_ROW(NV, MD, W) \
  text += prefix + (" " + std::to_string(K)) + " " + std::to_string(D) + " " #NV " " #MD " " #W + (pinkhip::has_entry(K, NV, MD, W) && emu_lookup(K, NV, MD, W) ? " 1\n" : " 0\n");
#define PINKHIP_FAMILY(KIND, DENSE, PREFIX, ARGS, TABLE) \
  {                                                      \
    const int K = pinkhip::KIND, D = DENSE;              \
    const std::string prefix = #PREFIX;                  \
    TABLE(PINKHIP_ROW)                                   \
  }
  PINKHIP_FAMILIES(PINKHIP_FAMILY)
#undef PINKHIP_FAMILY
#undef PINKHIP_ROW
  return text.c_str();
}
const char *pinkhip_emu_last_error(void) { return g_err.c_str(); }
const char *pinkhip_emu_warm_last_error(void) { return g_err.c_str(); }
const char *pinkhip_emu_pairs_last_error(void) { return g_err.c_str(); }
}
