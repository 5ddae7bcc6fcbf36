// Stand-alone check of pink_amd/csrc/host_plan.h -- TEST INFRASTRUCTURE ONLY.  Walks the launch plan over a grid of
// problems and asserts what must hold of any plan, without restating the dispatch rule:
//   g++ -std=c++17 -fsanitize=address,undefined host_plan_check.cpp -o host_plan_check && ./host_plan_check
// (tests/test_abi.py builds and runs it as a child process).
#include "emu_lanes.h"
#include "../pink_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pinkhip;

namespace {

// The case under test and what the plan made of it: printed when a check fails
struct {
  int nv, md, lead, nj, nf, n_eqf, rc;
  long long B;
  const char *solver;
  bool warm;
  LaunchPlan p;
  std::string err;
} c;
long long n_checked = 0;

#define CHECK(cond)                                                                                                                       \
  do {                                                                                                                                    \
    ++n_checked;                                                                                                                          \
    if (!(cond)) {                                                                                                                        \
      std::printf("FAILED %s (line %d): nv %d md %d n_free_lead %d B %lld PINKHIP_SOLVER %s%s, nj %d nf %d n_eqf %d -> rc %d '%s', kind %d <%d, %d, %d> blocks %lld\n", \
                  #cond, __LINE__, c.nv, c.md, c.lead, c.B, c.solver ? c.solver : "unset", c.warm ? " warm" : "", c.nj, c.nf, c.n_eqf, c.rc, c.err.c_str(),  \
                  c.p.kind, c.p.NV, c.p.MD, c.p.W, c.p.blocks);                                                                           \
      std::exit(1);                                                                                                                       \
    }                                                                                                                                     \
  } while (0)

// Is {NV, MD, W} an entry of the table its kind is launched from (dispatch.h has_entry)?
bool in_table(const LaunchPlan &p) {
  switch (p.kind) {
    case PLAN_STACK_SMALL: return p.NV == 8 && (p.W == 8 || p.W == 32);
    case PLAN_STACK_MFMA: return p.W == 64 && p.NV % 16 == 0 && p.NV >= 16 && p.NV <= 64;
  }
  return has_entry(p.kind, p.NV, p.MD, p.W);
}

// One digest (FNV-1a, 64 bits) over everything walked: the inputs of every plan and rc, kind, NV, MD, W, dense, blocks
unsigned long long digest = 1469598103934665603ULL;
void mix(long long v) {
  for (int i = 0; i < 8; ++i) digest = (digest ^ ((static_cast<unsigned long long>(v) >> (8 * i)) & 0xff)) * 1099511628211ULL;
}
void mix_plan() {
  for (long long v : {(long long)c.nv, (long long)c.md, (long long)c.lead, (long long)c.nj, (long long)c.nf, (long long)c.n_eqf, c.B,
                      (long long)(c.solver ? c.solver[0] + 256 * c.solver[std::string(c.solver).size() - 1] : 0), (long long)c.warm, (long long)c.rc,
                      (long long)c.p.kind, (long long)c.p.NV, (long long)c.p.MD, (long long)c.p.W, (long long)c.p.dense, c.p.blocks})
    mix(v);
}

// What must hold of every plan c.p that launches something for the c.B instances of c.nv coordinates (the leading `lead`
// of them free) and c.md dense rows
void check_plan(int lead) {
  const LaunchPlan &p = c.p;
  CHECK(c.rc == PINKHIP_OK && c.err.empty() && in_table(p));
  CHECK(c.nv <= p.NV && c.md <= (p.kind == PLAN_PACKED ? p.W : p.MD));
  // (only the tableau kernels eliminate: the others hold NV > W coordinates on their lanes)
  CHECK((p.kind != PLAN_SWEEP && p.kind != PLAN_SWEEP_WARM) || p.NV <= p.W || lead >= p.NV - p.W);
  CHECK(p.blocks * (64 / p.W) >= c.B && c.B > (p.blocks - 1) * (64 / p.W));
}

void walk_solve_plans() {
  for (c.nv = 1; c.nv <= 64; ++c.nv)
    for (int md : {0, 1, 2, 3, 6, 8, 9, 14, 16, 64})
      for (int lead : {0, 2})
        for (double damping : {1e-12, 1e-4}) {  // (no task rows: the first is rank deficient by construction)
          if (md > PINKHIP_MAX_MD) continue;
          c.md = md, c.lead = lead;
          pinkhip_desc d{};
          d.nv = c.nv, d.md = md, d.n_free_lead = lead, d.damping = damping, d.dt = 0.01, d.max_iter = 100;
          HostTables t;
          KernelArgs a{};
          c.err = build_tables(d, t);
          CHECK(c.err.empty());
          fill_desc(d, t, host_table_ptrs(t), a);
          CHECK(a.rank_deficient == (damping < 1e-9) && a.n_free_lead == (lead <= c.nv ? lead : 0) && a.n_barriers == 0);
          for (long long B : {0LL, 1LL, 3LL, 16384LL, 16385LL, 65536LL, 0x7fffffffLL, 0x80000000LL}) {
            a.B = c.B = B;
            for (const char *solver : {static_cast<const char *>(nullptr), "sweep", "sweepx", "packed"})
              for (bool warm : {false, true}) {
                c.solver = solver, c.warm = warm, c.err.clear();
                c.rc = plan_solve(a, solver, false, warm, c.p, c.err);
                mix_plan();
                CHECK((c.rc == PINKHIP_OK) == c.err.empty() && (c.rc == PINKHIP_OK || c.p.kind == PLAN_NONE));
                if (warm && (md > 0 || a.rank_deficient || (solver && std::string(solver) == "packed"))) {
                  CHECK(c.rc == PINKHIP_E_UNSUPPORTED);  // what a warm start refuses
                } else if (c.rc == PINKHIP_E_UNSUPPORTED) {
                  CHECK(warm);  // (no warm instantiation for this nv: never for a cold call)
                } else if (B == 0 || B > 0x7fffffffLL) {
                  CHECK(c.rc == (B ? PINKHIP_E_INVALID : PINKHIP_OK) && c.p.kind == PLAN_NONE);
                } else {  // (never "unsupported nv / md": the packed table holds every nv <= 64, md <= 64)
                  CHECK(warm == (c.p.kind == PLAN_SWEEP_WARM));
                  check_plan(a.n_free_lead);
                }
              }
            c.solver = nullptr, c.warm = false;
            if (md == 0 && lead == 0 && damping > 1e-9)  // the stack-only kernels, both variants of the small one
              for (bool four : {false, true}) {
                c.err.clear();
                c.rc = plan_stack(a, four, c.p, c.err);
                mix_plan();
                if (B == 0 || B > 0x7fffffffLL) {
                  CHECK(c.rc == (B ? PINKHIP_E_INVALID : PINKHIP_OK) && c.p.kind == PLAN_NONE);
                } else {
                  CHECK(c.p.kind == PLAN_STACK_SMALL || c.p.kind == PLAN_STACK_MFMA);
                  check_plan(0);
                }
              }
          }
        }
}

// The whole-step plan over synthetic robots: nj joints (a free-flyer root for nv = nj + 5), nf frame tasks + the posture
// task, md dense rows = 6 n_eqf constraint rows + barrier rows
void walk_rollout_plans() {
  static double dbuf[8];
  static int32_t ibuf[8];
  static uint8_t bbuf[8];
  const pinkhip_warm w{bbuf, bbuf};
  int n_ok = 0, n_unsupported = 0;
  c.B = 3, c.lead = 0, c.solver = nullptr;
  for (int nj : {1, 6, 7, 12, 19, 26, 30, 44, 50, 59})
    for (int root_nv : {1, 6})
      for (int nf : {0, 1, 2, 4, 12, 33})
        for (int n_eqf : {0, 1, 2})
          for (int n_bar : {0, 2, 6, 8})
            for (bool warm : {false, true}) {
              const int nv = nj + root_nv - 1, md = 6 * n_eqf + n_bar;
              if (nv > PINKHIP_MAX_NV || 6 * n_eqf > nv || n_eqf > nf) continue;
              c.nv = nv, c.md = md, c.nj = nj, c.nf = nf, c.n_eqf = n_eqf, c.warm = warm;
              ModelDev m{};
              m.nj = nj, m.nv = nv, m.nq = nv + (root_nv == 6), m.nf = nf, m.root_nv = root_nv;
              std::vector<int32_t> rows{0}, kind, col0;
              for (int f = 0; f < nf + (nv > root_nv); ++f) {  // nf frame tasks, then the posture task on the actuated coordinates
                rows.push_back(rows.back() + (f == nf ? nv - root_nv : 6));
                kind.push_back(f == nf ? PINKHIP_TASK_DIAGONAL : PINKHIP_TASK_DENSE);
                col0.push_back(f == nf ? root_nv : 0);
              }
              const std::vector<double> gain(kind.size(), 1.0), lm(kind.size(), 1e-6);
              pinkhip_desc d{};
              d.B = c.B, d.nv = nv, d.T = static_cast<int32_t>(kind.size()), d.Kd = 6 * nf, d.K = rows.back(), d.md = md, d.n_eq = 6 * n_eqf;
              d.task_rows = rows.data(), d.task_kind = kind.data(), d.task_col0 = col0.data(), d.gain = gain.data(), d.lm_damping = lm.data();
              d.damping = 1e-12, d.dt = 0.01, d.max_iter = 100;
              pinkhip_rollout_step st{};
              st.q = st.dq = dbuf, st.cost = st.T_target = st.q_target = dbuf, st.status = ibuf, st.config_limit_gain = 0.5;
              st.posture_task = 0, st.n_constraint_frames = n_eqf, st.constraint_frame = ibuf, st.constraint_gain = dbuf;
              st.barrier_frame = st.barrier_axis = st.barrier_frame2 = ibuf, st.barrier_sign = st.barrier_bound = st.barrier_gain = dbuf;
              HostTables t;
              RolloutArgs ra{};
              c.err = build_tables(d, t);
              CHECK(c.err.empty());
              fill_desc(d, t, host_table_ptrs(t), ra.k);
              const auto plan = [&](const pinkhip_rollout_step &s) {
                c.err.clear();
                c.rc = plan_rollout(d, m, false, s, warm ? &w : nullptr, nullptr, ra, c.p, c.err);
                mix_plan();
                return c.rc;
              };
              plan(st);
              CHECK((c.rc == PINKHIP_OK) == c.err.empty() && (c.rc == PINKHIP_OK || c.p.kind == PLAN_NONE));
              CHECK(c.rc == (warm && md > 0 ? PINKHIP_E_UNSUPPORTED : c.rc) && (c.rc == PINKHIP_OK || c.rc == PINKHIP_E_UNSUPPORTED));
              if (c.rc) {
                ++n_unsupported;
                continue;
              }
              ++n_ok;
              CHECK(c.p.kind == (md ? PLAN_ROLLOUT_DENSE : warm ? PLAN_ROLLOUT_WARM : PLAN_ROLLOUT));
              check_plan(0);
              CHECK(nj <= c.p.W && nf <= 32 && ra.k.lds_pitch > 0 && 8 * ra.k.lds_pitch * (64 / c.p.W) + 16 <= 65536);
              CHECK(ra.fk.B == d.B && ra.fk.m.nj == nj && ra.k.dq == dbuf && ra.post_k == nv - root_nv && ra.n_eqf == (md ? n_eqf : 0));
              // what the device entry point refuses, the shared plan refuses
              pinkhip_rollout_step s2 = st;
              s2.config_limit_gain = 0.0;
              CHECK(plan(s2) == PINKHIP_E_INVALID && c.p.kind == PLAN_NONE);
              s2 = st, s2.dq_scale = 100.0, s2.integrate = 1;
              CHECK(plan(s2) == PINKHIP_E_INVALID && c.p.kind == PLAN_NONE);
              s2 = st, s2.status = nullptr;
              CHECK(plan(s2) == PINKHIP_E_INVALID);
              s2 = st, s2.root_box = dbuf;
              CHECK(plan(s2) == (root_nv == 6 ? PINKHIP_OK : PINKHIP_E_INVALID));
            }
  CHECK(n_ok > 50 && n_unsupported > 0);
}

}  // namespace

int main() {
  walk_solve_plans();
  walk_rollout_plans();
  std::printf("host_plan_check: %lld checks passed, plan digest %016llx\n", n_checked, digest);
  return 0;
}
