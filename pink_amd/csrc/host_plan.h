// Host-side launch plan: from a validated pinkhip_desc and the arguments of a call to the filled kernel arguments and
// the instantiation that runs them.  Plain C++ (no HIP runtime calls, no device code), shared by the host side of the
// library (pinkhip.hip) and by the host harness of the CPU wave emulator of the test suite (emu/emu_kernels.cpp),
// so that the two can never disagree about validation, argument set-up or routing.  What differs stays with each
// side: where the broadcast tables live and how a plan becomes a launch (the library's launchers, the emulator's
// registry of per-lane entry points).
//
// Not for kernel translation units.  Include it behind wave.h (the emulator: wave_emu.h) and the kernel headers.
#pragma once

#include <cstring>
#include <string>

#include "dispatch.h"
#include "host_tables.h"
#include "ik_barrier_rows.h"
#include "ik_rollout.h"

namespace pinkhip {

// ---- 1. the descriptor part of KernelArgs --------------------------------------------------------------------------

// Where the seven broadcast tables of a descriptor live (device memory for the library, the HostTables themselves for
// the emulator)
struct TablePtrs {
  const double *row_gain, *row_lm, *barrier_safe_gain;
  const int *dtask_col0, *dtask_row0, *dtask_k, *barrier_rows;
};

inline TablePtrs host_table_ptrs(const HostTables &t) {
  return TablePtrs{t.row_gain.data(), t.row_lm.data(), t.barrier_safe_gain.data(), t.dtask_col0.data(), t.dtask_row0.data(),
                   t.dtask_k.data(), t.barrier_rows.data()};
}

// Everything the kernels take from the descriptor `d` and its tables `t` (as built by build_tables), which live at `p`
inline void fill_desc(const pinkhip_desc &d, const HostTables &t, const TablePtrs &p, KernelArgs &a) {
  a.B = d.B;
  a.nv = d.nv;
  a.Kd = d.Kd;
  a.K = d.K;
  a.md = d.md;
  a.n_eq = d.n_eq;
  a.n_dtasks = static_cast<int>(t.dtask_k.size());
  a.n_barriers = static_cast<int>(t.barrier_safe_gain.size());
  a.cost_batched = d.cost_is_batched;
  a.max_iter = d.max_iter;
  a.damping = d.damping;
  a.dt = d.dt;
  a.rank_deficient = rank_deficient_by_construction(d) ? 1 : 0;
  a.n_free_lead = (d.n_free_lead > 0 && d.n_free_lead <= d.nv) ? d.n_free_lead : 0;
  a.out_scale = 1.0;
  a.row_gain = p.row_gain;
  a.row_lm = p.row_lm;
  a.barrier_safe_gain = p.barrier_safe_gain;
  a.dtask_col0 = p.dtask_col0;
  a.dtask_row0 = p.dtask_row0;
  a.dtask_k = p.dtask_k;
  a.barrier_rows = p.barrier_rows;
}

// The functions below return PINKHIP_OK or an error code with its text in `err`.

inline int refuse(std::string &err, int code, const char *why) {
  err = why;
  return code;
}

// What is missing from the problem streams of `d` (NULL: nothing)
inline const char *problem_fault(const pinkhip_desc &d, const pinkhip_problem *in) {
  if (!in) return "null problem";
  if (d.B == 0) return nullptr;
  if (d.Kd > 0 && !in->J) return "J is NULL but Kd > 0";
  if (d.K > 0 && (!in->e || !in->cost)) return "e/cost NULL but K > 0";
  if (!in->lb || !in->ub) return "lb/ub must not be NULL";
  if (d.md > 0 && (!in->Gd || !in->hd)) return "Gd/hd NULL but md > 0";
  return nullptr;
}

inline void set_problem(KernelArgs &a, const pinkhip_problem &in) {
  a.J = in.J;
  a.e = in.e;
  a.cost = in.cost;
  a.lb = in.lb;
  a.ub = in.ub;
  a.Gd = in.Gd;
  a.hd = in.hd;
  a.c_extra = in.c_extra;
}

// The streams of a stack + solve call: problem, results and (warm entry points: `warm_call`) the active sets
inline int set_solve(const pinkhip_desc &d, const pinkhip_problem *in, const pinkhip_result *out, bool warm_call, const pinkhip_warm *warm,
                     KernelArgs &a, std::string &err) {
  if (const char *bad = problem_fault(d, in)) return refuse(err, PINKHIP_E_INVALID, bad);
  if (!out || (d.B > 0 && (!out->dq || !out->status))) return refuse(err, PINKHIP_E_INVALID, "dq/status must not be NULL");
  if (warm_call && !warm) return refuse(err, PINKHIP_E_INVALID, "null warm-start arguments");
  set_problem(a, *in);
  a.dq = out->dq;
  a.status = out->status;
  a.iters = out->iters;
  if (warm) {
    a.active_in = warm->active_in;
    a.active_out = warm->active_out;
  }
  return PINKHIP_OK;
}

// The kernel arguments of the two-launch control step (pinkhip_step_device) of B robots of the model `m`
inline FkArgs step_args(const ModelDev &m, long long B, const pinkhip_step &st) {
  FkArgs a{m, B, st.q, st.T_frames, nullptr};
  a.T_target = st.T_target;
  a.e_out = st.e;
  a.J_out = st.J;
  a.sE = st.sE;
  a.sJo = st.sJ;
  a.q_rw = st.q;
  a.dq_prev = st.dq_prev;
  a.status = st.status;
  a.first_failure = st.first_failure;
  a.step = st.step;
  a.dt = st.dt;
  a.config_limit_gain = st.config_limit_gain;
  a.root_box = st.root_box;
  a.q_target = st.q_target;
  a.target_batched = st.target_batched;
  a.lb = st.lb;
  a.ub = st.ub;
  a.e_off = st.e_off;
  return a;
}

// ---- 2. which kernel runs a filled KernelArgs ----------------------------------------------------------------------

// (PlanKind, LaunchPlan and make_plan: dispatch.h, beside the tables the kinds are launched from)

// What the warm entry points refuse beyond the validation of their cold twins (NULL: nothing)
inline const char *warm_refusal(const KernelArgs &a, const char *solver_env) {
  if (a.md > 0) return "warm starts are box-only (md == 0): dense rows run the dual method, which needs a dual-feasible start";
  if (a.rank_deficient) return "the task stack is rank deficient by construction: it is solved by the Goldfarb-Idnani kernel, which takes no active set";
  if (solver_env && std::strcmp(solver_env, "packed") == 0) return "PINKHIP_SOLVER=packed: the Goldfarb-Idnani kernel takes no active set";
  return nullptr;
}

// Stack only: fp64 MFMA tiles.  `four_tiles`: the nv <= 8 kernel with four tiles per wavefront instead of one
inline int plan_stack(const KernelArgs &a, bool four_tiles, LaunchPlan &p, std::string &err) {
  p = LaunchPlan{};
  if (a.B == 0) return PINKHIP_OK;
  if (a.B > 0x7fffffffLL) return refuse(err, PINKHIP_E_INVALID, "B exceeds the grid limit 2^31-1");
  if (a.nv <= 8 && a.n_barriers == 0) {  // two instances per MFMA tile
    p = make_plan(PLAN_STACK_SMALL, 8, 0, four_tiles ? 8 : 32, 0, a.B);
  } else if (a.nv >= 1 && a.nv <= 64) {  // NT = ceil(nv / 16) tiles, one instance per wavefront
    p = make_plan(PLAN_STACK_MFMA, 16 * ((a.nv + 15) / 16), 0, 64, 0, a.B);
  } else {
    return refuse(err, PINKHIP_E_INVALID, "unsupported nv");
  }
  return PINKHIP_OK;
}

// The sweep-tableau stack + solve kernels address the task rows of a wavefront's 64 / W instances with ONE 32-bit byte offset
// per lane from a scalar base (ik_stack_rows.h: WaveSplit, FULL_CHUNKS): those rows must lie within 4 GiB.  (2 GiB of task
// rows per instance at W = 32: no stack of Pink's comes near it; a batch that does runs the Goldfarb-Idnani kernel, which
// addresses in 64 bits per lane.)
inline bool rows_within_lane_offset(const KernelArgs &a, int W) {
  return W > 0 && (64 / W) * static_cast<long long>(a.Kd) * a.nv * 8 < (1LL << 32);
}

// Stack + solve: the instantiation chosen by dispatch.h.  The sweep-tableau kernel (ik_sweep.h) serves every problem it
// is instantiated for -- with virtual dense rows where that packs more QPs into a wavefront (ik_sweepx.h, prefer_sweepx)
// -- and the Goldfarb-Idnani kernel (ik_kernels_packed.h) the rest: 8-lane groups (nv <= 8), more dense rows than lanes
// are left.  solver_env: the value of PINKHIP_SOLVER (development / tests: "packed" / "sweep" / "sweepx" force one kernel
// for every problem it serves), force_dense: PINKHIP_FORCE_DENSE (development: the dense-row instantiation on a batch
// without dense rows), warm: the call brings an active set (pinkhip_warm).
inline int plan_solve(const KernelArgs &a, const char *solver_env, bool force_dense, bool warm, LaunchPlan &p, std::string &err) {
  p = LaunchPlan{};
  SweepChoice wc{0, 0, 0};
  if (warm) {
    if (const char *why = warm_refusal(a, solver_env)) return refuse(err, PINKHIP_E_UNSUPPORTED, why);
    wc = select_sweep_warm(a.nv, a.n_free_lead);
    if (!wc.NV) return refuse(err, PINKHIP_E_UNSUPPORTED, "no warm-start instantiation of the stack + solve kernel holds this nv");
  }
  if (a.B == 0) return PINKHIP_OK;
  if (a.B > 0x7fffffffLL) return refuse(err, PINKHIP_E_INVALID, "B exceeds the grid limit 2^31-1");
  if (warm) {
    if (!rows_within_lane_offset(a, wc.W)) return refuse(err, PINKHIP_E_UNSUPPORTED, "the task rows of a wavefront exceed 4 GiB: no warm start");
    p = make_plan(PLAN_SWEEP_WARM, wc.NV, wc.MD, wc.W, 0, a.B);
    return PINKHIP_OK;
  }
  const SweepChoice sc = select_sweep(a.nv, a.md, a.n_free_lead);
  const bool sweep = (solver_env ? (std::strcmp(solver_env, "packed") != 0 && sc.NV != 0)
                                 : (prefer_sweep(a.nv, a.md, a.B, a.n_free_lead) && !a.rank_deficient)) &&
                     rows_within_lane_offset(a, sc.W);
  const SweepChoice xc = select_sweepx(a.nv, a.md);
  const bool sweepx = solver_env ? (std::strcmp(solver_env, "sweepx") == 0 && xc.NV != 0) : (prefer_sweepx(a.nv, a.md) && !a.rank_deficient);
  const PackedChoice pc = select_packed(a.nv, a.md);
  if (sweepx) {
    p = make_plan(PLAN_SWEEPX, xc.NV, xc.MD, xc.W, 0, a.B);
  } else if (sweep) {
    p = make_plan(PLAN_SWEEP, sc.NV, sc.MD, sc.W, 0, a.B);
  } else if (pc.NV) {
    p = make_plan(PLAN_PACKED, pc.NV, 0, pc.W, (a.md == 0 && !force_dense) ? 0 : 1, a.B);
  } else {
    return refuse(err, PINKHIP_E_INVALID, "unsupported nv / md");
  }
  return PINKHIP_OK;
}

// ---- 3. the whole-step kernel --------------------------------------------------------------------------------------

// Validates the arguments `st` (+ `warm`: the warm-start twin of the box-only kernel) of a whole control step of the
// model `md` (has_relative: it has relative frame slots) against the descriptor `d`, completes `ra` -- whose k holds
// fill_desc(d) -- and picks the instantiation.
// (pairs: the step of pinkhip_rollout_step_pairs_device, validated by plan_rollout_pairs -- the last pairs->n_rows dense
// rows are formed from it, the barrier_* tables describe the rows in front of them)
inline int plan_rollout_step(const pinkhip_desc &d, const ModelDev &md, bool has_relative, const pinkhip_rollout_step &st, const pinkhip_warm *warm,
                             const pinkhip_sphere_pairs *pairs, const char *solver_env, RolloutArgs &ra, LaunchPlan &p, std::string &err) {
  p = LaunchPlan{};
  const int n_prow = pairs ? pairs->n_rows : 0;
  LaunchPlan chosen{};
  if (warm) {
    if (const char *why = warm_refusal(ra.k, solver_env)) return refuse(err, PINKHIP_E_UNSUPPORTED, why);
    ra.k.active_in = warm->active_in;
    ra.k.active_out = warm->active_out;
  }
  if (d.B == 0) return PINKHIP_OK;
  const int n_crow = st.n_const_rows;
  if (n_crow < 0 || (n_crow > 0 && (!st.const_rows || !st.const_q0 || !st.const_b)))
    return refuse(err, PINKHIP_E_INVALID, "n_const_rows must be >= 0 and come with const_rows / const_q0 / const_b");
  const int n_eqf = st.n_constraint_frames;
  if (n_eqf < 0 || n_eqf > kRolloutMaxEqFrames || (n_eqf > 0 && (!st.constraint_frame || !st.constraint_gain)))
    return refuse(err, PINKHIP_E_INVALID, "n_constraint_frames must lie in [0, 2] and come with constraint_frame / constraint_gain");
  if (d.nv != md.nv || d.n_eq != 6 * n_eqf)
    return refuse(err, PINKHIP_E_INVALID, "descriptor does not describe this model's task stack (nv, n_eq = 6 n_constraint_frames)");
  if (st.n_limit_rows < 0 || 6 * n_eqf + st.n_limit_rows > d.md - n_prow || (st.n_limit_rows > 0 && (!st.limit_rows || !st.limit_h)))
    return refuse(err, PINKHIP_E_INVALID, "n_limit_rows must lie in [0, md - n_eq] and come with limit_rows / limit_h");
  if (d.md - n_prow > 6 * n_eqf + st.n_limit_rows &&
      (!st.barrier_frame || !st.barrier_axis || !st.barrier_sign || !st.barrier_bound || !st.barrier_gain || !st.barrier_frame2))
    return refuse(err, PINKHIP_E_INVALID, "barrier rows need the barrier_* tables, barrier_frame2 included (-1 for the rows of a position barrier)");
  if ((st.root_box || st.n_limit_rows) && md.root_nv != 6) return refuse(err, PINKHIP_E_INVALID, "a floating-base velocity limit needs a free-flyer root joint");
  {
    const std::string why = rollout_task_layout(d, md.nf, md.nv, md.root_nv, n_crow, st.posture_task, st.diag_error != nullptr, ra.post_row0, ra.post_k);
    if (!why.empty()) return refuse(err, PINKHIP_E_INVALID, why.c_str());
  }
  if (!st.q || !st.cost || !st.dq || !st.status || (md.nf > 0 && !st.T_target) || (ra.post_k && !st.q_target)) return refuse(err, PINKHIP_E_INVALID, "null pointer");
  if (!(st.config_limit_gain > 0.0 && st.config_limit_gain <= 1.0) || st.step < 0 || st.step >= (1 << 23))
    return refuse(err, PINKHIP_E_INVALID, "bad limit gain / step");
  const int fkd = rollout_fk_doubles(md.nj, md.nf, n_crow);
  ra.n_crow = n_crow;
  ra.crow_A = st.const_rows;
  ra.crow_q0 = st.const_q0;
  ra.crow_b = st.const_b;
  ra.diag_e = st.diag_error;
  if (d.md > 0) {
    const int pd = pairs ? rollout_pairs_doubles(pairs->n_spheres, pairs->n_pairs, pairs->n_rows) : 0;
    const SweepChoice dc = pairs ? select_rollout_pairs(md.nv, md.nj, fkd, d.md, md.nf, n_eqf, pd) : select_rollout_dense(md.nv, md.nj, fkd, d.md, md.nf, n_eqf);
    if (dc.NV == 0 || md.nf > 32)
      return refuse(err, PINKHIP_E_UNSUPPORTED, pairs ? "no whole-step instantiation with sphere-pair rows fits this model"
                                                      : "no whole-step instantiation with barrier rows fits this model");
    chosen = make_plan(pairs ? PLAN_ROLLOUT_PAIRS : PLAN_ROLLOUT_DENSE, dc.NV, dc.MD, dc.W, 0, d.B);
    ra.k.lds_pitch = rollout_lds_doubles(dc.NV, dc.W, fkd, dc.MD, md.nf, n_eqf) + pd;
    ra.bar_frame = st.barrier_frame;
    ra.bar_axis = st.barrier_axis;
    ra.bar_sign = st.barrier_sign;
    ra.bar_bound = st.barrier_bound;
    ra.bar_gain = st.barrier_gain;
    ra.n_lim = st.n_limit_rows;
    ra.lim_rows = st.limit_rows;
    ra.lim_h = st.limit_h;
    ra.n_eqf = n_eqf;
    ra.eq_frame = st.constraint_frame;
    ra.eq_gain = st.constraint_gain;
    ra.bar_frame2 = st.barrier_frame2;
  } else {
    const PackedChoice pc = warm ? select_rollout_warm(md.nv, md.nj, fkd)
                                 : select_rollout(md.nv, md.nj, fkd, n_crow > 0 || st.diag_error != nullptr || st.acc_limit != nullptr || has_relative);
    if (pc.NV == 0 || md.nf > 32) return refuse(err, PINKHIP_E_UNSUPPORTED, "no whole-step instantiation fits this model");
    chosen = make_plan(warm ? PLAN_ROLLOUT_WARM : PLAN_ROLLOUT, pc.NV, 0, pc.W, 0, d.B);
    ra.k.lds_pitch = rollout_lds_doubles(pc.NV, pc.W, fkd);
  }
  ra.k.cost = st.cost;
  ra.k.out_scale = (st.dq_scale != 0.0) ? st.dq_scale : 1.0;
  if (st.dq_scale != 0.0 && st.dq_scale != 1.0 && st.integrate)
    return refuse(err, PINKHIP_E_INVALID, "dq_scale rescales what is written to dq: not together with integrate (the next step reads dq)");
  ra.k.dq = st.dq;
  ra.k.status = st.status;
  ra.k.iters = st.iters;
  FkArgs &f = ra.fk;
  f.m = md;
  f.B = d.B;
  f.q = st.q;
  f.q_rw = st.q;
  f.T_frames = st.T_frames;
  f.T_target = st.T_target;
  f.sTb = st.sT_b;
  f.sTf = (st.sT_b || st.sT_f) ? st.sT_f : 12;
  f.dt = d.dt;
  f.config_limit_gain = st.config_limit_gain;
  f.root_box = st.root_box;
  f.acc_limit = st.acc_limit;
  f.q_target = ra.post_k ? st.q_target : nullptr;
  f.target_batched = st.target_batched;
  ra.integrate = st.integrate;
  ra.first_failure = st.first_failure;
  ra.step = st.step;
  p = chosen;
  return PINKHIP_OK;
}

inline int plan_rollout(const pinkhip_desc &d, const ModelDev &md, bool has_relative, const pinkhip_rollout_step &st, const pinkhip_warm *warm,
                        const char *solver_env, RolloutArgs &ra, LaunchPlan &p, std::string &err) {
  return plan_rollout_step(d, md, has_relative, st, warm, nullptr, solver_env, ra, p, err);
}

// What every call that takes sphere pairs refuses about the tables of `sp` themselves (0: nothing): the limits of the on-chip
// stage (pair_rows of ik_rollout.h, the sphere-pair stage of ik_barrier_rows.h)
inline int pairs_tables_fault(const pinkhip_sphere_pairs *sp, std::string &err) {
  if (!sp) return refuse(err, PINKHIP_E_INVALID, "null sphere pairs");
  if (sp->n_spheres < 1 || sp->n_pairs < 1) return refuse(err, PINKHIP_E_INVALID, "sphere pairs need at least one sphere and one pair");
  if (sp->n_spheres > kPairsMaxSpheres) return refuse(err, PINKHIP_E_UNSUPPORTED, "more than 32 spheres");
  if (sp->n_pairs > kPairsMaxPairs) return refuse(err, PINKHIP_E_UNSUPPORTED, "more than 64 sphere pairs");
  if (sp->n_rows < 1 || sp->n_rows > sp->n_pairs) return refuse(err, PINKHIP_E_INVALID, "n_rows must lie in [1, n_pairs]");
  if (!sp->sphere_joint || !sp->sphere_centre || !sp->sphere_radius || !sp->column_mask || !sp->pair_sphere)
    return refuse(err, PINKHIP_E_INVALID, "sphere pairs: null table");
  if (!(sp->d_min >= 0.0) || !(sp->gain == sp->gain)) return refuse(err, PINKHIP_E_INVALID, "sphere pairs: bad d_min / gain");
  return PINKHIP_OK;
}

// What pinkhip_rollout_step_pairs_device refuses about its sphere pairs `sp` before anything else is looked at (0: nothing):
// the limits of the on-chip stage, and rows that are not the last barrier group of the descriptor's dense rows
inline int pairs_fault(const pinkhip_desc &d, const pinkhip_sphere_pairs *sp, std::string &err) {
  if (const int rc = pairs_tables_fault(sp, err)) return rc;
  if (d.n_barriers < 1 || !d.barrier_rows || d.barrier_rows[d.n_barriers] != d.md || d.barrier_rows[d.n_barriers - 1] != d.md - sp->n_rows)
    return refuse(err, PINKHIP_E_INVALID, "the sphere-pair rows must be the last barrier group of the dense rows (barrier_rows)");
  return PINKHIP_OK;
}

inline void fill_pairs(const pinkhip_sphere_pairs &sp, PairsArgs &p) {
  p.n_spheres = sp.n_spheres;
  p.n_pairs = sp.n_pairs;
  p.n_rows = sp.n_rows;
  p.sphere_joint = sp.sphere_joint;
  p.sphere_centre = sp.sphere_centre;
  p.sphere_radius = sp.sphere_radius;
  p.column_mask = sp.column_mask;
  p.pair_sphere = sp.pair_sphere;
  p.d_min = sp.d_min;
  p.gain = sp.gain;
}

// pinkhip_barrier_rows_device: what it refuses before anything is enqueued (0: nothing, `a` filled), for the library and
// the emulator alike
inline int plan_barrier_rows(const ModelDev &md, long long B, const double *q, double dt, const pinkhip_barrier_rows *rows,
                             const pinkhip_sphere_pairs *pairs, double *Gd, long long sG, double *hd, long long sH, int row0,
                             double *dist_out, BarrierRowsArgs &a, std::string &err) {
  if (B < 0 || B > 0x7fffffffLL) return refuse(err, PINKHIP_E_INVALID, "bad B");
  if (row0 < 0) return refuse(err, PINKHIP_E_INVALID, "row0 must not be negative");
  if (!(dt > 0.0) || !std::isfinite(dt)) return refuse(err, PINKHIP_E_INVALID, "dt must be positive and finite");
  const int n = rows ? rows->n_rows : 0;
  if (n < 0) return refuse(err, PINKHIP_E_INVALID, "negative number of rows");
  if (n == 0 && !pairs) return refuse(err, PINKHIP_E_INVALID, "no rows at all");
  if (n > 0 && (!rows->frame || !rows->axis || !rows->frame2 || !rows->sign || !rows->bound || !rows->gain))
    return refuse(err, PINKHIP_E_INVALID, "barrier rows: null table");
  if (pairs)
    if (const int rc = pairs_tables_fault(pairs, err)) return rc;
  const long long total = (long long)n + (pairs ? pairs->n_rows : 0);
  if (total > PINKHIP_MAX_MD) return refuse(err, PINKHIP_E_UNSUPPORTED, "more than PINKHIP_MAX_MD barrier rows in one call");
  if (md.nj > 64) return refuse(err, PINKHIP_E_UNSUPPORTED, "barrier rows need nj <= 64 (one lane per joint)");
  a = BarrierRowsArgs{};
  a.m = md;
  a.B = B;
  a.q = q;
  a.dt = dt;
  a.n_rows = n;
  if (n > 0) {
    a.frame = rows->frame, a.axis = rows->axis, a.frame2 = rows->frame2;
    a.sign = rows->sign, a.bound = rows->bound, a.gain = rows->gain;
  }
  if (pairs) fill_pairs(*pairs, a.p);
  a.Gd = Gd, a.hd = hd, a.sG = sG, a.sH = sH, a.row0 = row0, a.dist_out = dist_out;
  if (B == 0) return PINKHIP_OK;
  if (!q || !Gd || !hd) return refuse(err, PINKHIP_E_INVALID, "null pointer");
  if (sH < row0 + total || sG < (row0 + total) * md.nv) return refuse(err, PINKHIP_E_INVALID, "strides smaller than the rows");
  return PINKHIP_OK;
}

// The whole control step with sphere-pair rows: validation, the fill of `pa` -- whose r.k holds fill_desc(d) -- and the
// entry of PINKHIP_RPAIRS_TABLE that runs it
inline int plan_rollout_pairs(const pinkhip_desc &d, const ModelDev &md, bool has_relative, const pinkhip_rollout_step &st,
                              const pinkhip_sphere_pairs *sp, const char *solver_env, RolloutPairsArgs &pa, LaunchPlan &p, std::string &err) {
  p = LaunchPlan{};
  if (const int rc = pairs_fault(d, sp, err)) return rc;
  fill_pairs(*sp, pa.p);
  return plan_rollout_step(d, md, has_relative, st, nullptr, sp, solver_env, pa.r, p, err);
}

}  // namespace pinkhip
