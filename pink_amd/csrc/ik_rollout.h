// One kernel per control step: forward kinematics, FrameTask rows, limits, posture error, stacking, QP solve and
// integration for 64/W robots per wavefront -- what the reference does per robot and per step with Pinocchio +
// NumPy + quadprog (pink/solve_ik.py:206-275 followed by configuration.integrate_inplace,
// examples/inverse_kinematics_ur10.py:75-91).
//
// The task Jacobians never exist in memory: the kinematics phase (ik_kinematics.h) leaves, per robot, the world
// twist of each tangent column in that column's lane and two 3 x 3 blocks per FrameTask in LDS; the stacking of
// the solve kernel (ik_stack_rows.h / ik_sweep.h, source policy FkTerms) forms its six rows per task from them with
// 27 FMAs per lane.  Against the two-launch loop (ik_step_kernel writes J, e, lb, ub; ik_solve_packed_kernel reads
// them back) a step moves ~0.3 kB per robot through HBM instead of ~14 kB.  The kinematics scratch and the solve
// kernel's LDS (the stated problem parked for its closing refinement step, written after stacking) overlay each other.
#pragma once

#include "dispatch.h"
#include "ik_kinematics.h"
#include "ik_sweep.h"
#include "ik_sweepx.h"

namespace pinkhip {

struct RolloutArgs {
  KernelArgs k;  // task tables, cost, damping, dt, B, nv, Kd = 6 nf, K; outputs dq / status / iters; J, e, lb, ub unused
  FkArgs fk;     // model, q, targets, limit gain, posture target; T_frames optional; e / J / lb / ub outputs unused
  int integrate;       // apply dq to q at the end of the step (instances whose solve failed keep their q)
  int *first_failure;  // [B] sticky status | (step << 8), may be NULL
  int step;
  // PositionBarrier rows (pink/barriers/position_barrier.py:109-153), k.md of them: row d keeps
  // sign_d (p_frame_d [axis_d] - bound_d) >= 0;  G_d = -sign_d (R J_lin)[axis_d] / dt,  h_d = gain_d sign_d (p - bound)
  // (pink/barriers/barrier.py:246-254), both formed on chip from the world twists of the joint axes
  const int *bar_frame = nullptr, *bar_axis = nullptr;
  const double *bar_sign = nullptr, *bar_bound = nullptr, *bar_gain = nullptr;
  // FloatingBaseVelocityLimit rows that are not axis-aligned (floating_base_velocity_limit.py:128-148): the FIRST n_lim
  // of the k.md dense rows (Pink stacks limits before barriers, solve_ik.py:62-84), constant: row d is lim_rows[6 d ..]
  // on the six tangent coordinates of the root joint, zero elsewhere, with right-hand side lim_h[d].  The bar_*
  // tables are indexed by d - n_lim.
  int n_lim = 0;
  const double *lim_rows = nullptr, *lim_h = nullptr;
  // Equality constraints made of frame tasks (pink/solve_ik.py:125-149: A = J, b = -gain e): the LEADING 6 n_eqf dense rows
  // (k.n_eq of them), in front of the limit rows; constraint c is the FrameTask of model frame eq_frame[c] -- formed like
  // any frame task's rows, which is why the frame sits in the model (with zero cost when it carries no task)
  int n_eqf = 0;
  const int *eq_frame = nullptr;
  const double *eq_gain = nullptr;
  // BodySphericalBarrier rows (pink/barriers/body_spherical_barrier.py:73-143): a barrier row with bar_axis = 3 keeps
  // |p_f - p_f2|^2 - bound >= 0 (bound = d_min^2) with the class-K function h / (1 + |h|) of the reference's class:
  // G = -2 (p_f - p_f2)^T (R J_lin,f - R J_lin,f2) / dt,  h = gain alpha(|p_f - p_f2|^2 - d_min^2)
  const int *bar_frame2 = nullptr;
  // Dense tasks with a constant Jacobian (LinearHolonomicTask / JointCouplingTask on vector-space joints,
  // pink/tasks/linear_holonomic_task.py:103-148: e = A (q (-) q_0) - b, J = A): n_crow rows BEHIND the 6 nf FrameTask
  // rows of the dense block (k.Kd = 6 nf + n_crow); A [n_crow, nv], q_0 [nq], b [n_crow] in device memory
  int n_crow = 0;
  const double *crow_A = nullptr, *crow_q0 = nullptr, *crow_b = nullptr;
  // Diagonal tasks: the one whose error is q (-) q_target (the PostureTask) occupies the rows post_row0 .. + post_k of
  // e; every other diagonal task has batch-constant errors (DampingTask: 0, LowAccelerationTask: -dt v_prev,
  // JointVelocityTask: -dt v*; pink/tasks/damping_task.py, low_acceleration_task.py:46-84, joint_velocity_task.py:59-110)
  // read from diag_e [K - Kd] at row - Kd
  int post_row0 = 0, post_k = 0;
  const double *diag_e = nullptr;
};

// SelfCollisionBarrier rows of pairs of spheres attached to joints (pink/barriers/self_collision_barrier.py:85-224,
// barrier.py:193-254): the LAST n_rows of the k.md dense rows keep dist_k - d_min >= 0 for the n_rows closest of n_pairs
// pairs -- which pairs those are differs from robot to robot and from step to step, so they are selected on chip (pair_rows
// of ik_rollout_instance).  For spheres the nearest points lie on the line of centres and the normal is parallel to it: the
// reference's row n^T J_p1 + (r_1 x n)^T J_w1 - n^T J_p2 - (r_2 x n)^T J_w2 is n . (v(c_1) - v(c_2)) with v(c) the world
// velocity of the sphere CENTRE carried by its joint -- no nearest point and no radius enters the Jacobian.
struct PairsArgs {
  int n_spheres = 0, n_pairs = 0, n_rows = 0;
  const int *sphere_joint = nullptr;        // [n_spheres]
  const double *sphere_centre = nullptr;    // [n_spheres, 3], joint frame
  const double *sphere_radius = nullptr;    // [n_spheres]
  const unsigned *column_mask = nullptr;    // [nv]: bit s = the joint of tangent column i is sphere s's joint or an ancestor of it
  const int *pair_sphere = nullptr;         // [n_pairs, 2]
  double d_min = 0.0, gain = 0.0;
};

// (the arguments of the existing kernels stay what they are: r sits at offset 0 of the kernarg segment)
struct RolloutPairsArgs {
  RolloutArgs r;
  PairsArgs p;
};

// doubles of kinematics scratch per robot: joint poses, ancestor pointers, U / V blocks, frame errors (+ the errors of
// n_crow constant rows), joint scalars
__device__ __host__ inline int rollout_fk_doubles(int nj, int nf, int n_crow = 0) { return fk_lds_doubles(nj, nf) + 6 * nf + ((n_crow + 1) & ~1); }

template <int W, bool PAIRS = false>
struct FkTerms {
  static constexpr bool kOnTheFly = true;
  static constexpr bool kKeep = true;
  double lb = 0.0, ub = 0.0, x = 0.0;
  int status = 0;
  double lin[3], ang[3], post_e = 0.0, qv = 0.0;
  unsigned anc = 0, ancr = 0;  // bit f: this column's joint is an ancestor of frame f / of the root frame of relative slot f
  double *es = nullptr;        // LDS: errors of the dense rows [6 nf + n_crow]
  const double *UV = nullptr;  // LDS: U (9), V (9) per frame, pitch 36
  int nf = 0, n_crow = 0, col = 0, nvc = 0;  // frames, constant rows, this lane's tangent column, row pitch of crow_A
  const double *crow_A = nullptr;
  int post_row0 = 0, post_k = 0, Kd = 0;
  const double *diag_e = nullptr;
  // this lane's entries (tangent column li) of the six rows of FrameTask f -- or, behind the frames, of the next six
  // constant rows (their Jacobian is a table)
  __device__ __forceinline__ void frame_rows(int f, double (&six)[6]) const {
    if (f >= nf) {
      const int r0 = 6 * (f - nf);
#pragma unroll
      for (int i = 0; i < 6; ++i) six[i] = (r0 + i < n_crow) ? crow_A[(long long)(r0 + i) * nvc + col] : 0.0;
      return;
    }
    const double *u = UV + 36 * f;
    // (-1: ancestor of the frame only, +1: of the root frame of a relative slot only, 0: of both or neither)
    const double sgn = (double)((int)((ancr >> f) & 1u) - (int)((anc >> f) & 1u));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double top = u[3 * i] * lin[0] + u[3 * i + 1] * lin[1] + u[3 * i + 2] * lin[2] + u[9 + 3 * i] * ang[0] +
                         u[9 + 3 * i + 1] * ang[1] + u[9 + 3 * i + 2] * ang[2];
      const double bot = u[3 * i] * ang[0] + u[3 * i + 1] * ang[1] + u[3 * i + 2] * ang[2];
      six[i] = sgn * top;
      six[i + 3] = sgn * bot;
    }
  }
  __device__ __forceinline__ double error(int k) const { return es[k]; }
  __device__ __forceinline__ double diag_error(int r) const {
    if (r >= post_row0 && r < post_row0 + post_k) return post_e;
    return diag_e ? diag_e[r - Kd] : 0.0;
  }
  // dense rows = position barriers: this lane's entry (tangent column li) of row d, and the row's right-hand side.
  // World velocity of the frame origin p_f per unit of this column's joint velocity: lin + ang x p_f (zero unless the
  // joint is an ancestor of the frame) = column li of R J_lin (position_barrier.py:136-145).
  const int *bar_frame = nullptr, *bar_axis = nullptr;
  const double *bar_sign = nullptr, *bar_bound = nullptr, *bar_gain = nullptr;
  // LDS: frame f's world position at pfs[3 f .. 3 f + 2] -- a copy behind the area the kinematics scratch shares with
  // the solvers' working sets (dispatch.h, rollout_tail_doubles): the Goldfarb-Idnani code of the hand-over forms the
  // barrier rows while it is already writing its staged copy of them (its Gs overlaid the frame poses: the right-hand
  // side of a barrier row read back an entry of G -- scripts/gpu_fuzz_rollout.py seed 24680, "inconsistent")
  const double *pfs = nullptr;
  double inv_dt = 0.0;
  int n_lim = 0, root_sub = -1;  // constant rows of the floating-base limit; this lane's coordinate of the root joint
  const double *lim_rows = nullptr, *lim_h = nullptr;
  // equality rows of constraint frame tasks: 24 doubles per constraint in the tail of the robot's LDS (a copy, like pfs):
  // U (9), V (9) of the frame and its six errors
  int n_eqr = 0;  // 6 x constraints
  const int *eq_frame = nullptr;
  const double *eq_gain = nullptr, *eqs = nullptr;
  const int *bar_frame2 = nullptr;
  // PAIRS: the dense rows from pair_row0 on are sphere-pair rows.  LDS (tail): world centres of the spheres pcs [3 s ..],
  // five doubles per selected pair in pslots: the normal n (zero: the row is zero), the right-hand side, and the two
  // sphere indices a + 32 b; pmask: bit s = this lane's column moves sphere s
  int pair_row0 = 0;
  unsigned pmask = 0;
  const double *pcs = nullptr, *pslots = nullptr;
  // world velocity of frame f's origin per unit velocity of this lane's tangent column (zero unless an ancestor)
  __device__ __forceinline__ void origin_velocity(int f, double (&v)[3]) const {
    const double *pf = pfs + 3 * f;
    const double on = (((anc >> f) & 1u) != 0) ? 1.0 : 0.0;
    v[0] = on * (lin[0] + ang[1] * pf[2] - ang[2] * pf[1]);
    v[1] = on * (lin[1] + ang[2] * pf[0] - ang[0] * pf[2]);
    v[2] = on * (lin[2] + ang[0] * pf[1] - ang[1] * pf[0]);
  }
  __device__ __forceinline__ double dense_col(int d) const {
    if constexpr (PAIRS) {
      if (d >= pair_row0) {  // G = -J / dt,  J_i = n . ([i moves a] (lin + ang x c_a) - [i moves b] (lin + ang x c_b))
        const double *s = pslots + 5 * (d - pair_row0);
        const int ab = (int)s[4], sa = ab & 31, sb = (ab >> 5) & 31;
        const double ma = (double)((pmask >> sa) & 1u), mb = (double)((pmask >> sb) & 1u);
        const double *ca = pcs + 3 * sa, *cb = pcs + 3 * sb;
        const double wx = ma * ca[0] - mb * cb[0], wy = ma * ca[1] - mb * cb[1], wz = ma * ca[2] - mb * cb[2], mm = ma - mb;
        const double vx = mm * lin[0] + ang[1] * wz - ang[2] * wy, vy = mm * lin[1] + ang[2] * wx - ang[0] * wz,
                     vz = mm * lin[2] + ang[0] * wy - ang[1] * wx;
        return -inv_dt * (s[0] * vx + s[1] * vy + s[2] * vz);
      }
    }
    if (d < n_eqr) {
      // row i of the FrameTask Jacobian of constraint c (frame_rows(), from the tail copy of U, V)
      const int c = d / 6, i = d - 6 * c, f = eq_frame[c];
      const double *u = eqs + 24 * c;
      const double sgn = (double)((int)((ancr >> f) & 1u) - (int)((anc >> f) & 1u));
      const int r = i < 3 ? i : i - 3;
      const double bot = u[3 * r] * ang[0] + u[3 * r + 1] * ang[1] + u[3 * r + 2] * ang[2];
      const double top = u[3 * r] * lin[0] + u[3 * r + 1] * lin[1] + u[3 * r + 2] * lin[2] + u[9 + 3 * r] * ang[0] + u[9 + 3 * r + 1] * ang[1] +
                         u[9 + 3 * r + 2] * ang[2];
      return sgn * (i < 3 ? top : bot);
    }
    d -= n_eqr;
    if (d < n_lim) return root_sub >= 0 ? lim_rows[6 * d + root_sub] : 0.0;
    d -= n_lim;
    const int f = bar_frame[d], i = bar_axis[d];
    double v[3];
    origin_velocity(f, v);
    if (i == 3) {  // BodySphericalBarrier: -2 (p_f - p_f2) . (v_f - v_f2) / dt
      const int f2 = bar_frame2[d];
      double w[3];
      origin_velocity(f2, w);
      const double *p1 = pfs + 3 * f, *p2 = pfs + 3 * f2;
      return -2.0 * inv_dt * ((p1[0] - p2[0]) * (v[0] - w[0]) + (p1[1] - p2[1]) * (v[1] - w[1]) + (p1[2] - p2[2]) * (v[2] - w[2]));
    }
    const double vi = i == 0 ? v[0] : (i == 1 ? v[1] : v[2]);
    return -bar_sign[d] * vi * inv_dt;
  }
  __device__ __forceinline__ double dense_h(int d) const {
    if constexpr (PAIRS) {
      if (d >= pair_row0) return pslots[5 * (d - pair_row0) + 3];
    }
    if (d < n_eqr) {
      const int c = d / 6;
      return -eq_gain[c] * eqs[24 * c + 18 + (d - 6 * c)];  // b = -gain e (pink/solve_ik.py:147)
    }
    d -= n_eqr;
    if (d < n_lim) return lim_h[d];
    d -= n_lim;
    if (bar_axis[d] == 3) {
      const double *p1 = pfs + 3 * bar_frame[d], *p2 = pfs + 3 * bar_frame2[d];
      const double dx = p1[0] - p2[0], dy = p1[1] - p2[1], dz = p1[2] - p2[2];
      const double hb = dx * dx + dy * dy + dz * dz - bar_bound[d];
      return bar_gain[d] * hb / (1.0 + fabs(hb));  // (barrier.py:246-254 with the class's gain function)
    }
    return bar_gain[d] * bar_sign[d] * (pfs[3 * bar_frame[d] + bar_axis[d]] - bar_bound[d]);
  }
};

// WARM (box-only): the tableau starts from KernelArgs::active_in and leaves its final set in active_out (ik_sweep.h)
// PAIRS: `a` is the member r of a RolloutPairsArgs whose member p is *pp; the last pp->n_rows dense rows are sphere-pair rows
template <int NV, int MD, int W, bool WARM = false, bool PAIRS = false>
__device__ __forceinline__ void ik_rollout_instance(const RolloutArgs &a, long long block, const PairsArgs *pp = nullptr) {
  static_assert(!WARM || MD == 0, "warm starts are box-only");
  static_assert(!PAIRS || MD > 0, "sphere-pair rows are dense rows");
  using Terms = FkTerms<W, PAIRS>;
  constexpr int G = kWave / W;
  const ModelDev &m = a.fk.m;
  const int lane = lane_id();
  const int g = lane / W, li = lane & (W - 1);
  long long b = block * G + g;
  const bool valid = b < a.k.B;
  if (!valid) b = a.k.B - 1;
  // kinematics scratch at the start of this robot's share of LDS: the solve (which keeps stacking and the
  // factorisation in registers) first writes there after its last read of it; the share is the larger of the two
  double *sm = shared_base() + (long long)g * a.k.lds_pitch;
  // (PAIRS: the tail of the robot's share ends with the sphere-pair area, rollout_pairs_doubles)
  auto tail_doubles = [&](const RolloutArgs &ra, const PairsArgs *pa) {
    int n = rollout_tail_doubles(ra.fk.m.nf, ra.n_eqf);
    if constexpr (PAIRS) n += rollout_pairs_doubles(pa->n_spheres, pa->n_pairs, pa->n_rows);
    return n;
  };
  auto make_terms = [&](const RolloutArgs &ra, const PairsArgs *pa) {
    const ModelDev &mm = ra.fk.m;
    Terms tt;
    tt.es = sm + fk_lds_doubles(mm.nj, mm.nf);
    tt.UV = sm + 12 * (mm.nj + mm.nf) + ((mm.nj + 1) & ~1);  // = Jls of ik_fk_instance
    tt.nf = mm.nf, tt.n_crow = ra.n_crow, tt.col = li < mm.nv ? li : 0, tt.nvc = mm.nv, tt.crow_A = ra.crow_A;
    tt.post_row0 = ra.post_row0, tt.post_k = ra.post_k, tt.Kd = ra.k.Kd, tt.diag_e = ra.diag_e;
    if constexpr (MD > 0) {
      tt.bar_frame = ra.bar_frame, tt.bar_axis = ra.bar_axis;
      tt.bar_sign = ra.bar_sign, tt.bar_bound = ra.bar_bound, tt.bar_gain = ra.bar_gain;
      tt.pfs = sm + ra.k.lds_pitch - tail_doubles(ra, pa);
      tt.inv_dt = 1.0 / ra.k.dt;
      tt.n_lim = ra.n_lim, tt.lim_rows = ra.lim_rows, tt.lim_h = ra.lim_h;
      tt.n_eqr = 6 * ra.n_eqf, tt.eq_frame = ra.eq_frame, tt.eq_gain = ra.eq_gain, tt.bar_frame2 = ra.bar_frame2;
      tt.eqs = tt.pfs + ((3 * mm.nf + 1) & ~1);
      if (ra.n_lim > 0 && mm.root_nv == 6) {  // (the free-flyer is the first joint after the universe: columns 0 .. 5)
        const int jt = mm.dof_joint[li < mm.nv ? li : 0];
        if (li < mm.nv && mm.jtype[jt] == JOINT_FREE_FLYER) tt.root_sub = li - mm.idx_v[jt];
      }
      if constexpr (PAIRS) {
        tt.pair_row0 = ra.k.md - pa->n_rows;
        tt.pmask = li < mm.nv ? pa->column_mask[li] : 0u;
        tt.pcs = sm + ra.k.lds_pitch - rollout_pairs_doubles(pa->n_spheres, pa->n_pairs, pa->n_rows);
        tt.pslots = tt.pcs + 3 * pa->n_spheres + pa->n_pairs;
      }
    }
    return tt;
  };
  // (frame positions out of the shared area: fMo of ik_fk_instance holds frame f's pose at sm[12 (nj + f) ..])
  auto keep_frame_positions = [&](const RolloutArgs &ra, const PairsArgs *pa) {
    if constexpr (MD > 0) {
      const ModelDev &mm = ra.fk.m;
      double *tail = sm + ra.k.lds_pitch - tail_doubles(ra, pa);
      for (int i = li; i < 3 * mm.nf; i += W) tail[i] = sm[12 * (mm.nj + i / 3) + 9 + i % 3];
      if (ra.n_eqf > 0) {  // (kernel argument: wave-uniform)
        double *eqt = tail + ((3 * mm.nf + 1) & ~1);
        const double *UVs = sm + 12 * (mm.nj + mm.nf) + ((mm.nj + 1) & ~1), *ess = sm + fk_lds_doubles(mm.nj, mm.nf);
        for (int i = li; i < 24 * ra.n_eqf; i += W) {
          const int c = i / 24, k = i - 24 * c, f = ra.eq_frame[c];
          eqt[i] = k < 18 ? UVs[36 * f + k] : ess[6 * f + (k - 18)];
        }
      }
      wave_sync();
    }
  };
  // PAIRS: the sphere-pair stage, from the world poses of the joints (sm[12 j ..]) the kinematics left: centres (a sphere
  // per lane), distances (a pair per lane), the n_rows closest pairs -- ascending distance, ties to the lower pair index;
  // the rank of a pair is the number of pairs in front of it, counted over the distances in LDS (every lane reads the
  // same address: a broadcast) -- and per selected pair its slot: normal, right-hand side, sphere indices
  auto pair_rows = [&](const RolloutArgs &ra, const PairsArgs *pa) {
    if constexpr (PAIRS) {
      const int ns = pa->n_spheres, np = pa->n_pairs, nr = pa->n_rows;
      double *pc = sm + ra.k.lds_pitch - rollout_pairs_doubles(ns, np, nr), *pd = pc + 3 * ns, *ps = pd + np;
      for (int s = li; s < ns; s += W) {
        const double *X = sm + 12 * pa->sphere_joint[s], *c = pa->sphere_centre + 3 * s;
#pragma unroll
        for (int i = 0; i < 3; ++i) pc[3 * s + i] = X[3 * i] * c[0] + X[3 * i + 1] * c[1] + X[3 * i + 2] * c[2] + X[9 + i];
      }
      for (int i = li; i < 5 * nr; i += W) ps[i] = 0.0;
      wave_sync();
      for (int k = li; k < np; k += W) {
        const int sa = pa->pair_sphere[2 * k], sb = pa->pair_sphere[2 * k + 1];
        const double dx = pc[3 * sb] - pc[3 * sa], dy = pc[3 * sb + 1] - pc[3 * sa + 1], dz = pc[3 * sb + 2] - pc[3 * sa + 2];
        pd[k] = sqrt(dx * dx + dy * dy + dz * dz) - pa->sphere_radius[sa] - pa->sphere_radius[sb];
      }
      wave_sync();
      for (int k = li; k < np; k += W) {
        const double dk = pd[k];
        int rank = 0;
        for (int o = 0; o < np; ++o) {
          const double dv = pd[o];
          rank += (dv < dk || (dv == dk && o < k)) ? 1 : 0;
        }
        if (rank < nr) {
          const int sa = pa->pair_sphere[2 * k], sb = pa->pair_sphere[2 * k + 1];
          const double ra_ = pa->sphere_radius[sa], rb_ = pa->sphere_radius[sb];
          double u[3] = {pc[3 * sb] - pc[3 * sa], pc[3 * sb + 1] - pc[3 * sa + 1], pc[3 * sb + 2] - pc[3 * sa + 2]};
          const double rho = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), ir = rho > 0.0 ? 1.0 / rho : 0.0;
          // nearest points w1 = c_a + r_a u, w2 = c_b - r_b u; touching (np.allclose(w1, w2)): the row stays zero
          double n[3], n2 = 0.0;
          bool close = true;
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            u[i] *= ir;
            const double w1 = pc[3 * sa + i] + ra_ * u[i], w2 = pc[3 * sb + i] - rb_ * u[i];
            n[i] = w1 - w2;
            n2 += n[i] * n[i];
            close = close && fabs(n[i]) <= 1e-8 + 1e-5 * fabs(w2);
          }
          const double in_ = (close || !(n2 > 0.0)) ? 0.0 : 1.0 / sqrt(n2);
          double *slot = ps + 5 * rank;
          slot[0] = n[0] * in_, slot[1] = n[1] * in_, slot[2] = n[2] * in_;
          slot[3] = pa->gain * (dk - pa->d_min);  // (identity class-K function, barrier.py:246-254)
          slot[4] = (double)(sa + 32 * sb);
        }
      }
      wave_sync();
    }
  };
  // errors of the constant-row tasks, e_r = A_r (q (-) q_0) - b_r on the vector-space joints, behind the frame errors in LDS
  auto const_row_errors = [&](const RolloutArgs &ra, const Terms &tt) {
    if (ra.n_crow > 0) {  // wave-uniform (kernel argument)
      const ModelDev &mm = ra.fk.m;
      const int jt = mm.dof_joint[li < mm.nv ? li : 0];
      const bool vec = li < mm.nv && mm.jtype[jt] != JOINT_FREE_FLYER;
      const double dqv = vec ? tt.qv - ra.crow_q0[mm.idx_q[jt]] : 0.0;
      for (int r = 0; r < ra.n_crow; ++r) {
        const double er = group_sum<W>(vec ? ra.crow_A[(long long)r * mm.nv + li] * dqv : 0.0) - ra.crow_b[r];
        if (li == 0) tt.es[6 * mm.nf + r] = er;
      }
      wave_sync();
    }
  };
  // A task stack that is rank deficient by construction (host_tables.h: FrameTasks alone on more coordinates than they
  // have rows, examples/humanoid_jvrc.py:69-81) goes to the Goldfarb-Idnani code right away (kernel argument:
  // wave-uniform; its kinematics pass is the one below); everything else through the sweep tableau.
  const bool direct = a.k.rank_deficient != 0;
  Terms t = make_terms(a, pp);
  int st_sweep = STATUS_ROUTED;
  if (!direct) {
    ik_fk_instance<W, true, true, Terms>(a.fk, block, &t, sm);
    wave_sync();
    keep_frame_positions(a, pp);
    pair_rows(a, pp);
    const_row_errors(a, t);
    // (more tableau rows than lanes: the dense rows are virtual, ik_sweepx.h -- two robots per wavefront at nv = 30
    // with barrier rows instead of one)
    if constexpr (NV + MD > W) st_sweep = ik_sweepx_instance<NV, MD, W, Terms>(a.k, block, &t);
    else st_sweep = ik_sweep_instance<NV, MD, W, Terms, WARM>(a.k, block, &t);
  }
  // a result that fails its KKT certificate is not integrated: the Goldfarb-Idnani code solves that robot's QP again
  // (ik_sweep.h, ik_solve_sweep_body).  It forms the rows from the kinematics like the tableau did, and the tableau's
  // parking area has overwritten the kinematics scratch meanwhile: the kinematics run once more (wave-uniform, rare).
#ifdef PINKHIP_SWEEP_NO_HANDOVER  // (development: what the tableau code alone says)
  const bool over = false;
#else
  const bool over = st_sweep == STATUS_BREAKDOWN || st_sweep == STATUS_ROUTED;
#endif
  if (wave_any(over)) {
    wave_sync();
    // (arguments read again, terms built again: nothing of them is kept in registers through the tableau loop)
    const RolloutArgs *again = kernarg_reload<RolloutArgs>(a);
    const PairsArgs *pp2 = nullptr;
    if constexpr (PAIRS) pp2 = &reinterpret_cast<const RolloutPairsArgs *>(again)->p;
    Terms t2 = make_terms(*again, pp2);
    ik_fk_instance<W, true, true, Terms>(again->fk, block, &t2, sm);
    wave_sync();
    keep_frame_positions(*again, pp2);
    pair_rows(*again, pp2);
    const_row_errors(*again, t2);
    // (WARM: it leaves the working set it ends on in active_out)
    ik_packed_instance<NV, W, (MD > 0), Terms, WARM>(again->k, block, &t2, over,
                                                     again->k.rank_deficient ? PATH_GI : (st_sweep == STATUS_ROUTED ? PATH_ROUTED : PATH_HANDOVER));
    if (over) t.x = t2.x, t.status = t2.status;
  }
  // integration: lane = joint fetches its dq entries from the lanes that hold them (lane = tangent coordinate)
  const int st = t.status;  // group-uniform
  const bool isj = li < m.nj;
  const int jl = isj ? li : 0;
  const int iv = m.idx_v[jl], iq = m.idx_q[jl];
  const bool ff = m.jtype[jl] == JOINT_FREE_FLYER;
  double v[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) v[i] = lane_shfl(t.x, g * W + ((i == 0 || ff) ? (iv + i) & (W - 1) : iv & (W - 1)));
  if (a.integrate) {
    if (st == 0) {
      if (valid && isj) {
        double *qw = a.fk.q_rw + b * (long long)m.nq + iq;
        double qj[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) qj[i] = (i == 0 || ff) ? qw[i] : 0.0;
        integrate_joint(m, jl, qj, v);
#pragma unroll
        for (int i = 0; i < 7; ++i)
          if (i == 0 || ff) qw[i] = qj[i];
      }
    } else if (valid && li == 0 && a.first_failure && a.first_failure[b] == 0) {
      a.first_failure[b] = st | (a.step << 8);
    }
  }
}

template <int NV, int MD, int W>
__global__ void __launch_bounds__(kWave) PINKHIP_OCCUPANCY_ROLLOUT(NV + MD) ik_rollout_kernel(RolloutArgs a) {
  ik_rollout_instance<NV, MD, W>(a, block_id());
}

// ... whose tableau starts from the caller's active set (PINKHIP_WROLLOUT_TABLE): the budget of the cold twin
template <int NV, int W>
__global__ void __launch_bounds__(kWave) PINKHIP_OCCUPANCY_ROLLOUT(NV) ik_rollout_warm_kernel(RolloutArgs a) {
  ik_rollout_instance<NV, 0, W, true>(a, block_id());
}

// ... whose last dense rows are sphere-pair rows selected and formed on chip (PINKHIP_RPAIRS_TABLE): the
// budget of the twin without them
template <int NV, int MD, int W>
__global__ void __launch_bounds__(kWave) PINKHIP_OCCUPANCY_ROLLOUT(NV + MD) ik_rollout_pairs_kernel(RolloutPairsArgs a) {
  ik_rollout_instance<NV, MD, W, false, true>(a.r, block_id(), &a.p);
}

// The whole-step families (dispatch.h Family): the host plan (host_plan.h) has set lds_pitch = rollout_lds_doubles(...)
template <int NV, int MD, int W>
struct RolloutFamilyBase {
  // (NV + MD > W: dense rows without lanes of their own, ik_sweepx.h)
  static_assert(NV + MD > W ? sweepx_lds_doubles(NV, MD, W) == SweepXLds<NV, MD, W>::stride
                            : sweep_lds_doubles(NV, MD, W) == SweepLds<NV, MD, W>::stride, "dispatch.h restates the LDS layout");
  static_assert(packed_lds_doubles(NV, MD) == LdsP<NV>::stride(MD), "dispatch.h restates the LDS layout");
  static const KernelArgs &core(const RolloutArgs &a) { return a.k; }
  static const KernelArgs &core(const RolloutPairsArgs &a) { return a.r.k; }
  template <class Args>
  static Args prepared(const Args &a) { return a; }
  template <class Args>
  static size_t lds_bytes(const Args &a) { return 8 * static_cast<size_t>(core(a).lds_pitch) * (kWave / W) + 16; }
  template <class Args>
  static long long B(const Args &a) { return core(a).B; }
};
template <int NV, int W>
struct Family<PLAN_ROLLOUT, NV, 0, W, false> : RolloutFamilyBase<NV, 0, W> {
  using Args = RolloutArgs;
  static constexpr void (*kernel)(Args) = ik_rollout_kernel<NV, 0, W>;
};
template <int NV, int MD, int W>
struct Family<PLAN_ROLLOUT_DENSE, NV, MD, W, false> : RolloutFamilyBase<NV, MD, W> {
  static_assert(MD > 0, "barrier rows are dense rows");
  using Args = RolloutArgs;
  static constexpr void (*kernel)(Args) = ik_rollout_kernel<NV, MD, W>;
};
template <int NV, int W>
struct Family<PLAN_ROLLOUT_WARM, NV, 0, W, false> : RolloutFamilyBase<NV, 0, W> {
  using Args = RolloutArgs;
  static constexpr void (*kernel)(Args) = ik_rollout_warm_kernel<NV, W>;
};
template <int NV, int MD, int W>
struct Family<PLAN_ROLLOUT_PAIRS, NV, MD, W, false> : RolloutFamilyBase<NV, MD, W> {
  static_assert(MD > 0, "sphere-pair rows are dense rows");
  using Args = RolloutPairsArgs;
  static constexpr void (*kernel)(Args) = ik_rollout_pairs_kernel<NV, MD, W>;
};

}  // namespace pinkhip
