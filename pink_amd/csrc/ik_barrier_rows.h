// Barrier rows on the device (pink/barriers/position_barrier.py, body_spherical_barrier.py, self_collision_barrier.py): the
// dense inequality rows of PositionBarriers, BodySphericalBarriers and one SelfCollisionBarrier of sphere pairs, written
// into the Gd / hd streams of the solve kernel in the form it consumes (pink/barriers/barrier.py:246-254),
//   Gd[b sG + (row0 + r) nv + j] = -J_h[r][j] / dt,   hd[b sH + row0 + r] = gain alpha(h_r),
// beside the task rows of ik_fk_frame_tasks_kernel (ik_kinematics.h), ik_com_task_kernel (ik_com.h),
// ik_manipulability_task_kernel (ik_manip.h) and ik_rolling_tasks_kernel (ik_rolling.h).  Tables and conventions are those
// of the whole-step kernel's barrier rows (ik_rollout.h: RolloutArgs::bar_*, PairsArgs), so callers pass the same tables.
//
// Joint k has world pose (R_k, p_k) and world axis u = R_k axis_k; m_f in {0, 1} says that k is frame f's joint or one of its
// ancestors.  The world velocity of the origin p_f per unit velocity of a tangent column of joint k is
//     revolute    u x (p_f - p_k)        prismatic   u
//     free-flyer  R_k e_i (linear coordinate i),  (R_k e_i) x (p_f - p_k) (angular coordinate i)
// times m_f.  For the difference of two points p, p' carried by k with masks m, m' this is  s x (m p - m' p' - (m - m') p_k)
// for an angular column and (m - m') s for a linear one: a common ancestor contributes s x (p - p') without the two large
// terms that cancel, a joint off both paths exactly zero.
//   position row   h = sign (p_f[axis] - bound),      J_h = sign (velocity of p_f)[axis],           alpha = identity
//   spherical row  h = |d|^2 - bound, d = p_f - p_f2,  J_h = 2 d . (velocity of p_f - velocity of p_f2),  alpha = h / (1 + |h|)
//   pair rows      pair_rows of ik_rollout_instance: centres a sphere per lane, distances a pair per lane, the n_rows
//                  smallest distances (ascending, ties to the lower pair index) by counting; per kept pair
//                  J_h = n . (velocity of c_a - velocity of c_b), h = gain (dist - d_min), a zero row for touching spheres
//
// The joint poses and the pointer jumping to world poses are the expensive part and do not depend on the row: they are
// composed once, and the loop over the rows reads the poses from LDS.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/pinkhip.h"
#include "ik_kinematics.h"
#include "ik_rollout.h"

namespace pinkhip {

struct BarrierRowsArgs {
  ModelDev m;
  long long B;
  const double *q;  // [B, nq]
  double dt;
  int n_rows;  // position + spherical rows, described by the six tables [n_rows] (device memory)
  const int *frame, *axis, *frame2;
  const double *sign, *bound, *gain;
  PairsArgs p;  // p.n_rows sphere-pair rows behind them (0: none)
  double *Gd;   // Gd[b sG + (row0 + r) nv + j]
  double *hd;   // hd[b sH + row0 + r]
  long long sG, sH;
  int row0;
  double *dist_out;  // [B, p.n_rows] or NULL: the selected distances
};

// lanes per robot: the smallest of 8 / 32 / 64 that holds one lane per joint
inline int barrier_rows_group_width(int nj) { return nj <= 8 ? 8 : nj <= 32 ? 32 : 64; }

// doubles of LDS per robot: the world poses of the joints, and behind them the sphere-pair area (centres, distances, slots)
__device__ __host__ inline int barrier_rows_lds_doubles(int nj, const PairsArgs &p) {
  return pose_lds_doubles(nj) + (p.n_rows > 0 ? rollout_pairs_doubles(p.n_spheres, p.n_pairs, p.n_rows) : 0);
}

// World position of the origin of frame slot f: its placement's translation carried by its joint (world pose in oM), or the
// translation itself on the world
__device__ __forceinline__ void frame_origin_in_world(const ModelDev &m, int f, const double *oM, double *p) {
  const int fj = m.frame_joint[f];
  const double *pl = m.frame_placement + 12 * f;
  if (fj >= 0) {
    const double *X = oM + 12 * fj;
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = X[3 * i] * pl[9] + X[3 * i + 1] * pl[10] + X[3 * i + 2] * pl[11] + X[9 + i];
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = pl[9 + i];
  }
}

// The barrier rows of one instance by a group of W lanes (W >= nj), the mapping of ik_rolling_instance:
//   1.-2. lane = joint: pose in the parent frame, pointer jumping to world poses (as compose_world_poses);
//   3. per position / spherical row (a loop uniform over the wavefront): the frame origins from the LDS poses, the lane's own
//      column(s) stored by the joint lane; lane 0 stores the right-hand side;
//   4. the sphere-pair stage (pair_rows of ik_rollout_instance on the LDS behind the poses), then per kept pair the same.
// Every tangent column belongs to exactly one joint lane: the rows are written completely, zeros included.
template <int W>
__device__ __forceinline__ void ik_barrier_rows_instance(const BarrierRowsArgs &a, long long block) {
  const ModelDev &m = a.m;
  const GroupLane gl = group_lane<W>(block, a.B, m.nj);
  const int li = gl.li, jl = gl.jl;
  const long long b = gl.b;
  const bool valid = gl.valid, isj = gl.isj;
  double *oM = shared_base() + (long long)gl.g * barrier_rows_lds_doubles(m.nj, a.p);
  const double *q = a.q + b * (long long)m.nq;

  // the tables of this lane's joint, requested before the poses are composed
  const int my_col = m.idx_v[jl];
  const int my_type = m.jtype[jl];
  const double ax0 = m.axis[3 * jl], ax1 = m.axis[3 * jl + 1], ax2 = m.axis[3 * jl + 2];

  // 1. pose of joint li in its parent's frame
  double T[12];
  {
    double Tj[12];
    joint_transform(m, jl, q + m.idx_q[jl], Tj);
    se3_mul(m.placement + 12 * jl, Tj, T);
  }
  int *anc = reinterpret_cast<int *>(oM + 12 * m.nj);
  int up = isj ? m.parent[jl] : -1;
  if (isj) {
#pragma unroll
    for (int i = 0; i < 12; ++i) oM[12 * li + i] = T[i];
    anc[li] = up;
  }
  wave_sync();
  // 2. pointer jumping: T_j <- T_up(j) T_j, up(j) <- up(up(j)) until every joint is expressed in the world.
  // compose_world_poses (ik_kinematics.h) written out, as in ik_rolling_instance (see there and DESIGN.md): the two must stay
  // the same algorithm.
  while (wave_any(up >= 0)) {
    double P[12];
    int upup = -1;
    if (up >= 0) {
#pragma unroll
      for (int i = 0; i < 12; ++i) P[i] = oM[12 * up + i];
      upup = anc[up];
    }
    wave_sync();  // every lane has read the old poses and pointers
    if (up >= 0) {
      double N[12];
      se3_mul(P, T, N);
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        T[i] = N[i];
        oM[12 * li + i] = N[i];
      }
      anc[li] = upup;
      up = upup;
    }
    wave_sync();
  }
  // the lane's world axes: one for a revolute / prismatic joint; the free-flyer's are the columns of R_k
  const bool ff = my_type == JOINT_FREE_FLYER;
  const double u[3] = {T[0] * ax0 + T[1] * ax1 + T[2] * ax2, T[3] * ax0 + T[4] * ax1 + T[5] * ax2,
                       T[6] * ax0 + T[7] * ax1 + T[8] * ax2};
  const double inv_dt = 1.0 / a.dt;
  const bool store = valid && isj;
  double *Gb = a.Gd + b * a.sG + my_col;
  double *hb = a.hd + b * a.sH;

  // The lane's entries of the row whose J_h is n . (velocity of P - velocity of P2): column c of this lane's joint carries P
  // when M1[c] and P2 when M2[c] (1.0 or 0.0); w = m1 P - m2 P2 - (m1 - m2) p_k
  auto store_row = [&](int row, const double (&n)[3], const double (&P)[3], const double (&P2)[3], const double (&M1)[6], const double (&M2)[6]) {
    double *Go = Gb + (long long)row * m.nv;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      if (c == 0 || ff) {
        const double m1 = M1[c], m2 = M2[c], mm = m1 - m2;
        const bool on = m1 != 0.0 || m2 != 0.0;
        const double w[3] = {m1 * P[0] - m2 * P2[0] - mm * T[9], m1 * P[1] - m2 * P2[1] - mm * T[10], m1 * P[2] - m2 * P2[2] - mm * T[11]};
        const int k = c % 3;
        const double s[3] = {ff ? T[k] : u[0], ff ? T[3 + k] : u[1], ff ? T[6 + k] : u[2]};
        const bool angular = ff ? c >= 3 : my_type == JOINT_REVOLUTE;
        double l[3];
        cross3(s, w, l);
#pragma unroll
        for (int i = 0; i < 3; ++i) l[i] = angular ? l[i] : mm * s[i];
        const double v = n[0] * l[0] + n[1] * l[1] + n[2] * l[2];
        Go[c] = on ? -inv_dt * v : 0.0;
      }
    }
  };

  // 3. position and spherical rows
  for (int r = 0; r < a.n_rows; ++r) {
    const int f = a.frame[r], axis = a.axis[r];
    const bool sph = axis == 3;
    const int f2 = sph ? a.frame2[r] : f;
    double pf[3], pg[3];
    frame_origin_in_world(m, f, oM, pf);
    frame_origin_in_world(m, f2, oM, pg);
    const double d[3] = {pf[0] - pg[0], pf[1] - pg[1], pf[2] - pg[2]};
    const double sg = a.sign[r];
    // position: n = sign e_axis, the second point takes no part; spherical: n = 2 d
    const double n[3] = {sph ? 2.0 * d[0] : (axis == 0 ? sg : 0.0), sph ? 2.0 * d[1] : (axis == 1 ? sg : 0.0),
                         sph ? 2.0 * d[2] : (axis == 2 ? sg : 0.0)};
    const double m1 = (isj && m.anc[f * m.nj + jl] != 0) ? 1.0 : 0.0;
    const double m2 = (sph && isj && m.anc[f2 * m.nj + jl] != 0) ? 1.0 : 0.0;
    const double M1[6] = {m1, m1, m1, m1, m1, m1}, M2[6] = {m2, m2, m2, m2, m2, m2};
    if (store) store_row(a.row0 + r, n, pf, pg, M1, M2);
    if (valid && li == 0) {
      const double pa = axis == 0 ? pf[0] : (axis == 1 ? pf[1] : pf[2]);
      const double hs = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] - a.bound[r];
      hb[a.row0 + r] = sph ? a.gain[r] * hs / (1.0 + fabs(hs)) : a.gain[r] * sg * (pa - a.bound[r]);
    }
  }

  // 4. sphere-pair rows
  if (a.p.n_rows > 0) {  // (kernel argument: wave-uniform)
    const PairsArgs &pp = a.p;
    const int ns = pp.n_spheres, np = pp.n_pairs, nr = pp.n_rows;
    double *pc = oM + pose_lds_doubles(m.nj), *pd = pc + 3 * ns, *ps = pd + np;
    for (int s = li; s < ns; s += W) {
      const double *X = oM + 12 * pp.sphere_joint[s], *c = pp.sphere_centre + 3 * s;
#pragma unroll
      for (int i = 0; i < 3; ++i) pc[3 * s + i] = X[3 * i] * c[0] + X[3 * i + 1] * c[1] + X[3 * i + 2] * c[2] + X[9 + i];
    }
    for (int i = li; i < 5 * nr; i += W) ps[i] = 0.0;
    wave_sync();
    for (int k = li; k < np; k += W) {
      const int sa = pp.pair_sphere[2 * k], sb = pp.pair_sphere[2 * k + 1];
      const double dx = pc[3 * sb] - pc[3 * sa], dy = pc[3 * sb + 1] - pc[3 * sa + 1], dz = pc[3 * sb + 2] - pc[3 * sa + 2];
      pd[k] = sqrt(dx * dx + dy * dy + dz * dz) - pp.sphere_radius[sa] - pp.sphere_radius[sb];
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
        const int sa = pp.pair_sphere[2 * k], sb = pp.pair_sphere[2 * k + 1];
        const double ra_ = pp.sphere_radius[sa], rb_ = pp.sphere_radius[sb];
        double uu[3] = {pc[3 * sb] - pc[3 * sa], pc[3 * sb + 1] - pc[3 * sa + 1], pc[3 * sb + 2] - pc[3 * sa + 2]};
        const double rho = sqrt(uu[0] * uu[0] + uu[1] * uu[1] + uu[2] * uu[2]), ir = rho > 0.0 ? 1.0 / rho : 0.0;
        // nearest points w1 = c_a + r_a u, w2 = c_b - r_b u; touching (np.allclose(w1, w2)): the row stays zero
        double n[3], n2 = 0.0;
        bool close = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          uu[i] *= ir;
          const double w1 = pc[3 * sa + i] + ra_ * uu[i], w2 = pc[3 * sb + i] - rb_ * uu[i];
          n[i] = w1 - w2;
          n2 += n[i] * n[i];
          close = close && fabs(n[i]) <= 1e-8 + 1e-5 * fabs(w2);
        }
        const double in_ = (close || !(n2 > 0.0)) ? 0.0 : 1.0 / sqrt(n2);
        double *slot = ps + 5 * rank;
        slot[0] = n[0] * in_, slot[1] = n[1] * in_, slot[2] = n[2] * in_;
        slot[3] = pp.gain * (dk - pp.d_min);  // (identity class-K function, barrier.py:246-254)
        slot[4] = (double)(sa + 32 * sb);
        if (valid && a.dist_out) a.dist_out[b * nr + rank] = dk;
      }
    }
    wave_sync();
    // bit s of the mask of a column: the column moves sphere s
    unsigned pmask[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) pmask[c] = (isj && (c == 0 || ff)) ? pp.column_mask[my_col + c] : 0u;
    for (int k = 0; k < nr; ++k) {
      const double *slot = ps + 5 * k;
      const int ab = (int)slot[4], sa = ab & 31, sb = (ab >> 5) & 31;
      const double n[3] = {slot[0], slot[1], slot[2]};
      const double ca[3] = {pc[3 * sa], pc[3 * sa + 1], pc[3 * sa + 2]}, cb[3] = {pc[3 * sb], pc[3 * sb + 1], pc[3 * sb + 2]};
      double M1[6], M2[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) M1[c] = (double)((pmask[c] >> sa) & 1u), M2[c] = (double)((pmask[c] >> sb) & 1u);
      if (store) store_row(a.row0 + a.n_rows + k, n, ca, cb, M1, M2);
      if (valid && li == 0) hb[a.row0 + a.n_rows + k] = slot[3];
    }
  }
}

template <int W>
__global__ void __launch_bounds__(kWave) PINKHIP_OCCUPANCY_FK
ik_barrier_rows_kernel(BarrierRowsArgs a) {
  ik_barrier_rows_instance<W>(a, block_id());
}

}  // namespace pinkhip
