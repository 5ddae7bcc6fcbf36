// Host harness of the warm-start entry points on the CPU wave emulator -- TEST INFRASTRUCTURE ONLY (see wave_emu.h).
// pinkhip_emu_solve_warm_host / pinkhip_emu_rollout_step_warm next to emu_kernels.cpp's cold ones: the same argument
// set-up as pinkhip_solve_warm_device / pinkhip_rollout_step_warm_device (pinkhip.hip), on host memory.
#include "emu_warm.h"

#include <cstdlib>
#include <string>

using namespace pinkemu;

// (the emulator's model object, as emu_kernels.cpp defines it: pinkhip_emu_model_create hands it out as a void *)
struct EmuModel {
  pinkhip::ModelImage image;
  pinkhip::ModelDev dev;
};

namespace {

using pinkhip::KernelArgs;

std::string g_werr;

// what the warm entry points refuse (pinkhip.hip, warm_refusal)
bool refused(const pinkhip_desc *d, const KernelArgs &a) {
  const char *force = std::getenv("PINKHIP_SOLVER");
  if (d->md > 0 || a.rank_deficient || (force && std::string(force) == "packed")) {
    g_werr = "warm starts: box-only stacks of full rank on the tableau kernels";
    return true;
  }
  return false;
}

// the table part of the kernel arguments (prepare() of pinkhip.hip)
bool fill(const pinkhip_desc *d, pinkhip::HostTables &t, KernelArgs &a) {
  g_werr = pinkhip::build_tables(*d, t);
  if (!g_werr.empty()) return false;
  a.B = d->B;
  a.nv = d->nv;
  a.Kd = d->Kd;
  a.K = d->K;
  a.md = d->md;
  a.n_eq = d->n_eq;
  a.n_dtasks = static_cast<int>(t.dtask_k.size());
  a.n_barriers = d->n_barriers;
  a.cost_batched = d->cost_is_batched;
  a.max_iter = d->max_iter;
  a.damping = d->damping;
  a.dt = d->dt;
  a.rank_deficient = pinkhip::rank_deficient_by_construction(*d) ? 1 : 0;
  a.n_free_lead = (d->n_free_lead > 0 && d->n_free_lead <= d->nv) ? d->n_free_lead : 0;
  a.out_scale = 1.0;
  a.row_gain = t.row_gain.data();
  a.row_lm = t.row_lm.data();
  a.dtask_col0 = t.dtask_col0.data();
  a.dtask_row0 = t.dtask_row0.data();
  a.dtask_k = t.dtask_k.data();
  a.barrier_rows = t.barrier_rows.data();
  a.barrier_safe_gain = t.barrier_safe_gain.data();
  return true;
}

}  // namespace

extern "C" {

int pinkhip_emu_solve_warm_host(const pinkhip_desc *d, const pinkhip_problem *in, const pinkhip_result *out, const pinkhip_warm *warm) {
  if (!d || !in || !out || !warm) {
    g_werr = "null argument";
    return PINKHIP_E_INVALID;
  }
  pinkhip::HostTables t;
  KernelArgs a{};
  if (!fill(d, t, a)) return PINKHIP_E_INVALID;
  if (refused(d, a)) return PINKHIP_E_UNSUPPORTED;
  const pinkhip::SweepChoice sc = pinkhip::select_sweep_warm(a.nv, a.n_free_lead);
  LaneEntry fn = sc.NV ? emu_lookup(KIND_SWEEP_WARM, sc.NV, 0, sc.W) : nullptr;
  if (!fn) {
    g_werr = "no warm-start instantiation of the stack + solve kernel holds this nv";
    return PINKHIP_E_UNSUPPORTED;
  }
  a.J = in->J;
  a.e = in->e;
  a.cost = in->cost;
  a.lb = in->lb;
  a.ub = in->ub;
  a.Gd = in->Gd;
  a.hd = in->hd;
  a.c_extra = in->c_extra;
  a.dq = out->dq;
  a.status = out->status;
  a.iters = out->iters;
  a.active_in = warm->active_in;
  a.active_out = warm->active_out;
  const long long G = 64 / sc.W, blocks = (d->B + G - 1) / G;
  for (long long b = 0; b < blocks; ++b) pinkhip::emu_run_block(b, fn, &a);
  return PINKHIP_OK;
}

int pinkhip_emu_rollout_step_warm(const pinkhip_desc *d, void *mp, const pinkhip_rollout_step *st, const pinkhip_warm *warm) {
  if (!d || !mp || !st || !warm) {
    g_werr = "null argument";
    return PINKHIP_E_INVALID;
  }
  EmuModel *m = static_cast<EmuModel *>(mp);
  pinkhip::HostTables t;
  pinkhip::RolloutArgs ra{};
  KernelArgs &a = ra.k;
  if (!fill(d, t, a)) return PINKHIP_E_INVALID;
  if (refused(d, a)) return PINKHIP_E_UNSUPPORTED;
  if (d->nv != m->dev.nv || d->n_eq != 0 || st->n_constraint_frames != 0) {
    g_werr = "descriptor does not describe this model's box-only task stack";
    return PINKHIP_E_INVALID;
  }
  a.out_scale = (st->dq_scale != 0.0) ? st->dq_scale : 1.0;
  a.cost = st->cost;
  a.dq = st->dq;
  a.status = st->status;
  a.iters = st->iters;
  a.active_in = warm->active_in;
  a.active_out = warm->active_out;
  pinkhip::FkArgs &f = ra.fk;
  f.m = m->dev;
  f.B = d->B;
  f.q = st->q;
  f.q_rw = st->q;
  f.T_frames = st->T_frames;
  f.T_target = st->T_target;
  f.sTb = st->sT_b;
  f.sTf = (st->sT_b || st->sT_f) ? st->sT_f : 12;
  f.dt = d->dt;
  f.config_limit_gain = st->config_limit_gain;
  f.root_box = st->root_box;
  f.acc_limit = st->acc_limit;
  int post_row0 = 0, post_k = 0;
  g_werr = pinkhip::rollout_task_layout(*d, m->dev.nf, m->dev.nv, m->dev.root_nv, st->n_const_rows, st->posture_task, st->diag_error != nullptr, post_row0,
                                        post_k);
  if (!g_werr.empty()) return PINKHIP_E_INVALID;
  f.q_target = post_k ? st->q_target : nullptr;
  f.target_batched = st->target_batched;
  ra.integrate = st->integrate;
  ra.first_failure = st->first_failure;
  ra.step = st->step;
  ra.n_crow = st->n_const_rows;
  ra.crow_A = st->const_rows;
  ra.crow_q0 = st->const_q0;
  ra.crow_b = st->const_b;
  ra.post_row0 = post_row0;
  ra.post_k = post_k;
  ra.diag_e = st->diag_error;
  const int fkd = pinkhip::rollout_fk_doubles(m->dev.nj, m->dev.nf, st->n_const_rows);
  const pinkhip::PackedChoice pc = pinkhip::select_rollout_warm(m->dev.nv, m->dev.nj, fkd);
  LaneEntry fn = pc.NV ? emu_lookup(KIND_ROLLOUT_WARM, pc.NV, 0, pc.W) : nullptr;
  if (!fn || m->dev.nf > 32) {
    g_werr = "no whole-step instantiation fits this model";
    return PINKHIP_E_UNSUPPORTED;
  }
  a.lds_pitch = pinkhip::rollout_lds_doubles(pc.NV, pc.W, fkd);
  const long long G = 64 / pc.W, blocks = (d->B + G - 1) / G;
  for (long long b = 0; b < blocks; ++b) pinkhip::emu_run_block(b, fn, &ra);
  return PINKHIP_OK;
}

const char *pinkhip_emu_warm_last_error(void) { return g_werr.c_str(); }
}
