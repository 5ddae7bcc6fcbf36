// RollingTask / OmniwheelTask rows on the device (pink/tasks/rolling_task.py, omniwheel_task.py): wheel-contact rows of up
// to eight wheels of one robot, written into the packed e / J streams of the solve kernel beside the rows of
// ik_fk_frame_tasks_kernel (ik_kinematics.h), ik_com_task_kernel (ik_com.h) and ik_manipulability_task_kernel (ik_manip.h).
//
// A wheel is a relative frame slot of the model: frame = hub H (world pose R_H, p_H), root = floor F (R_F, p_F); rho its
// radius.  The contact point p_C = p_H - rho R_F e_z is the point of the hub's body rho below the hub along the floor's
// normal.
//   e = (0, 0, z - rho),  z = (R_F^T (p_H - p_F))_z
//   J = velocity of p_C, carried by the hub's body, in the floor's axes, per unit tangent velocity.  Joint k (world pose
//       R_k, p_k; world axis u = R_k axis_k) between the root and the hub:
//         revolute    R_F^T (u x (p_C - p_k))
//         prismatic   R_F^T u
//         free-flyer  R_F^T R_k e_i (linear coordinate i),  R_F^T ((R_k e_i) x (p_C - p_k)) (angular coordinate i)
//       every column of a joint off that path: exactly zero.
// The floor is inertial, as in the reference: R_F and p_F follow q when the floor hangs on a moving joint, but its ancestors
// own no column.  An Omniwheel keeps rows 0 and 2.
//
// The joint poses and the pointer jumping to world poses are the expensive part and do not depend on the wheel: they are
// composed once, and the loop over the wheels reads the poses from LDS.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/pinkhip.h"
#include "ik_kinematics.h"

namespace pinkhip {

constexpr int ROLLING_MAX_WHEELS = 8;  // pinkhip.h: PINKHIP_MAX_WHEELS
constexpr int WHEEL_ROLLING = 0;       // pinkhip.h: PINKHIP_WHEEL_ROLLING / _OMNI
constexpr int WHEEL_OMNI = 1;

struct RollingArgs {
  ModelDev m;
  long long B;
  const double *q;  // [B, nq]
  int n;            // wheels, 1..8
  int slot[ROLLING_MAX_WHEELS];       // relative frame slot of the device model: frame = hub, root = floor
  int kind[ROLLING_MAX_WHEELS];       // 0: three rows, 1: rows 0 and 2
  double radius[ROLLING_MAX_WHEELS];
  double *e_out;  // e_out[b sE + row0 + r_w + i]
  double *J_out;  // J_out[b sJ + (row0 + r_w + i) nv + j]
  long long sE, sJ;
  int row0;
  double *height_out;  // [B, n] or NULL: z per wheel
};

// rows of all wheels of a call
inline int rolling_rows_total(const RollingArgs &a) {
  int r = 0;
  for (int w = 0; w < a.n && w < ROLLING_MAX_WHEELS; ++w) r += a.kind[w] == WHEEL_OMNI ? 2 : 3;
  return r;
}

// Fills the by-value tables of the arguments from the caller's host arrays; NULL, or why the call is refused
// (PINKHIP_E_INVALID) -- the arrays are then not read further
inline const char *rolling_set_wheels(RollingArgs &a, int n, const int *slot, const int *kind, const double *radius) {
  a.n = n;
  if (n < 1 || n > ROLLING_MAX_WHEELS) return "the number of wheels must be in 1..8";
  if (!slot || !kind || !radius) return "null pointer";
  for (int w = 0; w < ROLLING_MAX_WHEELS; ++w) {
    a.slot[w] = w < n ? slot[w] : 0;
    a.kind[w] = w < n ? kind[w] : 0;
    a.radius[w] = w < n ? radius[w] : 0.0;
  }
  return nullptr;
}

// What pinkhip_rolling_tasks_device refuses before anything is enqueued (NULL: nothing); `code` receives PINKHIP_E_INVALID
// or PINKHIP_E_UNSUPPORTED.  root_joint: the HOST copy of the model's frame_root_joint table.
inline const char *rolling_task_fault(const RollingArgs &a, const int *root_joint, int &code) {
  code = PINKHIP_E_INVALID;
  if (a.B < 0 || a.B > 0x7fffffffLL) return "bad B";
  if (a.n < 1 || a.n > ROLLING_MAX_WHEELS) return "the number of wheels must be in 1..8";
  for (int w = 0; w < a.n; ++w) {
    if (a.slot[w] < 0 || a.slot[w] >= a.m.nf) return "wheel slot outside the model";
    if (root_joint[a.slot[w]] < -1) return "wheel slot without a root: a wheel is a relative slot (frame = hub, root = floor)";
    if (a.kind[w] != WHEEL_ROLLING && a.kind[w] != WHEEL_OMNI) return "wheel kind must be ROLLING (0) or OMNI (1)";
    if (!std::isfinite(a.radius[w])) return "wheel radius must be finite";
  }
  if (a.row0 < 0) return "row0 must not be negative";
  if (a.m.nj > 64) {
    code = PINKHIP_E_UNSUPPORTED;
    return "wheel-contact rows need nj <= 64 (one lane per joint)";
  }
  if (a.B == 0) return nullptr;
  if (!a.q || !a.e_out || !a.J_out) return "null pointer";
  const long long rows = (long long)a.row0 + rolling_rows_total(a);
  if (a.sE < rows || a.sJ < rows * a.m.nv) return "strides smaller than the rows";
  return nullptr;
}

// lanes per robot: the smallest of 8 / 32 / 64 that holds one lane per joint (the columns are formed by joint lanes, so the
// tangent dimension does not widen the group)
inline int rolling_group_width(int nj) { return nj <= 8 ? 8 : nj <= 32 ? 32 : 64; }

// The rows of every wheel of one instance by a group of W lanes (W >= nj), the mapping of ik_manip_instance:
//   1.-2. lane = joint: pose in the parent frame, pointer jumping to world poses (as compose_world_poses);
//   3. per wheel (a loop uniform over the wavefront): hub and floor pose from the LDS poses, the contact point, the lane's
//      own column(s) rotated into the floor's axes and stored by the joint lane; lane 0 stores e and the height.
// Every tangent column belongs to exactly one joint lane: the rows are written completely, zeros included.
template <int W>
__device__ __forceinline__ void ik_rolling_instance(const RollingArgs &a, long long block) {
  const ModelDev &m = a.m;
  const GroupLane gl = group_lane<W>(block, a.B, m.nj);
  const int li = gl.li, jl = gl.jl;
  const long long b = gl.b;
  const bool valid = gl.valid, isj = gl.isj;
  double *oM = shared_base() + (long long)gl.g * pose_lds_doubles(m.nj);
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
  // compose_world_poses (ik_kinematics.h) written out: with the pose returned by value the compiler fuses the other product
  // of some sums a b + c d of the wheel loop below, and the rows come out a rounding apart; with the pose behind a pointer
  // the kernel is 1 - 3 % slower.  The two must stay the same algorithm.
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

  // 3. the wheels
  int row = a.row0;
  for (int w = 0; w < a.n; ++w) {
    const int f = a.slot[w];
    const bool omni = a.kind[w] == WHEEL_OMNI;
    const double rho = a.radius[w];
    const int fj = m.frame_joint[f], rj = m.frame_root_joint[f];
    const bool onpath = isj && m.anc[f * m.nj + jl] != 0;
    double TH[12], TF[12];  // hub and floor in the world (joint -1: the world itself)
    frame_pose_in_world(fj, m.frame_placement + 12 * f, oM, TH);
    frame_pose_in_world(rj, m.frame_root_placement + 12 * f, oM, TF);
    // floor normal n = R_F e_z, height z = n . (p_H - p_F), contact point p_C = p_H - rho n; d = p_C - p_k
    const double n0 = TF[2], n1 = TF[5], n2 = TF[8];
    const double z = n0 * (TH[9] - TF[9]) + n1 * (TH[10] - TF[10]) + n2 * (TH[11] - TF[11]);
    const double d[3] = {TH[9] - rho * n0 - T[9], TH[10] - rho * n1 - T[10], TH[11] - rho * n2 - T[11]};
    if (valid && isj) {
      double *Jo = a.J_out + b * a.sJ + (long long)row * m.nv + my_col;
      const long long r1 = omni ? 0 : m.nv, r2 = omni ? m.nv : 2ll * m.nv;  // (an Omniwheel has no middle row)
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        if (c == 0 || ff) {
          // column c of the joint: axis s, angular (s x d) or linear (s)
          const int k = c % 3;
          const double s[3] = {ff ? T[k] : u[0], ff ? T[3 + k] : u[1], ff ? T[6 + k] : u[2]};
          const bool angular = ff ? c >= 3 : my_type == JOINT_REVOLUTE;
          double l[3];
          cross3(s, d, l);
#pragma unroll
          for (int i = 0; i < 3; ++i) l[i] = angular ? l[i] : s[i];
          double o[3];
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const double v = TF[i] * l[0] + TF[3 + i] * l[1] + TF[6 + i] * l[2];  // (R_F^T l)_i
            o[i] = onpath ? v : 0.0;
          }
          Jo[c] = o[0];
          if (!omni) Jo[r1 + c] = o[1];
          Jo[r2 + c] = o[2];
        }
      }
    }
    if (valid && li == 0) {
      double *eo = a.e_out + b * a.sE + row;
      eo[0] = 0.0;
      if (!omni) eo[1] = 0.0;
      eo[omni ? 1 : 2] = z - rho;
      if (a.height_out) a.height_out[b * a.n + w] = z;
    }
    row += omni ? 2 : 3;
  }
}

template <int W>
__global__ void __launch_bounds__(kWave) PINKHIP_OCCUPANCY_FK
ik_rolling_tasks_kernel(RollingArgs a) {
  ik_rolling_instance<W>(a, block_id());
}

}  // namespace pinkhip
