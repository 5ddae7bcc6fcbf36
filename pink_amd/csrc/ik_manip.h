// ManipulabilityTask row on the device (pink/tasks/manipulability_task.py): the gradient of Yoshikawa's index
//   m(q) = sqrt(det A),  A = J J^T,  J = the kept rows of the 6 x nv Jacobian of a frame (LOCAL: body, WORLD: spatial, twists
//   [v; w] taken at the world origin)
// written as ONE row into the packed e / J streams of the solve kernel, beside the rows of ik_fk_frame_tasks_kernel
// (ik_kinematics.h) and ik_com_task_kernel (ik_com.h).
//
// The reference builds the n x 6 x n kinematic Hessian H and contracts J H_i^T with pinv(A).  A is symmetric, so
//   Jm[i] = m sum_k P_k . H[i, :, k],   P = A^-1 J   (column k of P: two triangular solves on column k of J)
//   H[i, :3, k] = w_i x v_k  (i <= k),  w_k x v_i  (i > k)
//   H[i, 3:, k] = w_i x w_k  (i <= k),  0          (i > k)
// with (v_k, w_k) the linear and angular part of column k.  The task is admitted only where every joint between the root
// and the frame is revolute: one column per joint of the path, joint order = column order; every other column is zero.
//
// Singular A (this project's rule; the reference's result there is round-off): A = L D L^T without pivoting over the kept
// rows, and a pivot <= r eps max_i A_ii makes m = 0 and the row exactly zero (r = number of kept rows).
#pragma once

#include <cstdint>

#include "../../include/pinkhip.h"
#include "ik_kinematics.h"

namespace pinkhip {

constexpr int MANIP_LOCAL = 0;  // pinkhip.h: PINKHIP_FRAME_LOCAL / _WORLD
constexpr int MANIP_WORLD = 1;

struct ManipArgs {
  ModelDev m;
  long long B;
  const double *q;  // [B, nq]
  int frame;        // frame slot of the device model
  int world;        // reference frame: 0 LOCAL, 1 WORLD
  int row_mask;     // bit i: row i of the 6 x nv Jacobian is kept
  int rank;         // number of kept rows
  double rate;      // e = -rate
  double *e_out;    // e_out[b sE + row0]
  double *J_out;    // J_out[b sJ + row0 nv + j]
  long long sE, sJ;
  int row0;
  double *m_out;  // [B] or NULL
};

// what pinkhip_manipulability_task_device refuses before anything is enqueued, beside the path check (NULL: nothing)
inline const char *manip_task_fault(const ManipArgs &a) {
  if (a.B < 0 || a.B > 0x7fffffffLL) return "bad B";
  if (a.frame < 0 || a.frame >= a.m.nf) return "frame index outside the model";
  if (a.world != MANIP_LOCAL && a.world != MANIP_WORLD) return "reference frame must be LOCAL (0) or WORLD (1)";
  if ((a.row_mask & 63) == 0 || (a.row_mask & ~63) != 0) return "row mask must keep at least one of the six rows (bits 0..5)";
  if (a.B == 0) return nullptr;
  if (!a.q || !a.e_out || !a.J_out) return "null pointer";
  if (a.row0 < 0) return "row0 must not be negative";
  if (a.sE < a.row0 + 1 || a.sJ < (long long)(a.row0 + 1) * a.m.nv) return "strides smaller than the row";
  return nullptr;
}

// The path check on the host tables of a model (parent, jtype [nj]; the frame's joint): NULL, or why the task is not
// admitted (PINKHIP_E_UNSUPPORTED)
inline const char *manip_path_fault(int nj, const int *parent, const int *jtype, int frame_joint) {
  if (nj > 64) return "manipulability rows need nj <= 64 (one lane per joint)";
  for (int j = frame_joint; j >= 0; j = parent[j])
    if (jtype[j] != JOINT_REVOLUTE) return "ManipulabilityTask only supports revolute joints on the path to the frame";
  return nullptr;
}

// One instance by a group of W lanes (W >= nj), the mapping of ik_com_instance:
//   1.-2. lane = joint: pose in the parent frame, pointer jumping to world poses (compose_world_poses);
//   3. lane = joint k: its column (v, w) of the frame's Jacobian, zero off the path (cm: the kept rows of it);
//   4. A = sum over the lanes of column column^T (21 group sums), L D L^T in every lane's registers, m from the pivots,
//      P_k by two triangular solves on the lane's own column;
//   5. over the joints k of the path: (P_k, v_k, w_k) broadcast, the two cross-product terms accumulated with the
//      i <= k selects (no LDS traffic in that loop);
//   6. the row, stored by joint lane.
template <int W>
__device__ __forceinline__ void ik_manip_instance(const ManipArgs &a, long long block) {
  const ModelDev &m = a.m;
  const GroupLane gl = group_lane<W>(block, a.B, m.nj);
  const int li = gl.li, jl = gl.jl;
  const long long b = gl.b;
  const bool valid = gl.valid, isj = gl.isj;
  double *oM = shared_base() + (long long)gl.g * pose_lds_doubles(m.nj);
  const double *q = a.q + b * (long long)m.nq;

  // the tables of this lane's joint and of the frame, requested before the poses are composed
  const bool onpath = isj && m.anc[a.frame * m.nj + jl] != 0;
  const int my_col = m.idx_v[jl];
  const int my_ncol = m.jtype[jl] == JOINT_FREE_FLYER ? 6 : 1;  // (off the path: its columns are zero)
  const double ax0 = m.axis[3 * jl], ax1 = m.axis[3 * jl + 1], ax2 = m.axis[3 * jl + 2];
  const int fj = m.frame_joint[a.frame];
  double Fp[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) Fp[i] = m.frame_placement[12 * a.frame + i];

  // 1.-2. world pose of joint li, in this lane's registers and (all joints) in oM
  const Pose X = compose_world_poses(m, gl, joint_pose_in_parent(m, jl, q + m.idx_q[jl]), oM);
  const double(&T)[12] = X.T;
  // 3. the column of joint li: world axis u through p_k = T[9..11]
  double c[6];
  {
    const double u[3] = {T[0] * ax0 + T[1] * ax1 + T[2] * ax2, T[3] * ax0 + T[4] * ax1 + T[5] * ax2,
                         T[6] * ax0 + T[7] * ax1 + T[8] * ax2};
    const double pk[3] = {T[9], T[10], T[11]};
    if (a.world) {  // spatial Jacobian: the twist at the world origin, (p_k x u, u)
      cross3(pk, u, c);
      c[3] = u[0], c[4] = u[1], c[5] = u[2];
    } else {  // body Jacobian: R_f^T (u x (p_f - p_k)), R_f^T u
      double Tf[12];
      frame_pose_in_world(fj, Fp, oM, Tf);
      const double d[3] = {Tf[9] - pk[0], Tf[10] - pk[1], Tf[11] - pk[2]};
      double l[3];
      cross3(u, d, l);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        c[i] = Tf[i] * l[0] + Tf[3 + i] * l[1] + Tf[6 + i] * l[2];
        c[3 + i] = Tf[i] * u[0] + Tf[3 + i] * u[1] + Tf[6 + i] * u[2];
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) c[i] = onpath ? c[i] : 0.0;
  }
  // (the Hessian's cross products take the whole column -- the reference masks H's rows, not the columns it is built
  // from; A and P take the kept rows)
  double cm[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) cm[i] = ((a.row_mask >> i) & 1) ? c[i] : 0.0;
  // 4. A (a masked-out row: zero off the diagonal, one on it -- its pivot is one, it decouples), L D L^T, m, P
  double A[6][6];
  double amax = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) A[i][j] = group_sum<W>(cm[i] * cm[j]);
    const bool kept = ((a.row_mask >> i) & 1) != 0;
    amax = (kept && A[i][i] > amax) ? A[i][i] : amax;
    A[i][i] = kept ? A[i][i] : 1.0;
  }
  const double tol = (double)a.rank * 2.220446049250313e-16 * amax;
  bool singular = false;
  double L[6][6], D[6], rD[6];
  double det = 1.0;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * D[k];
    const bool kept = ((a.row_mask >> j) & 1) != 0;
    singular = singular || (kept && !(d > tol));
    D[j] = d;
    rD[j] = 1.0 / d;
    det *= d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k] * D[k];
      L[i][j] = s * rD[j];
    }
  }
  const double mval = singular ? 0.0 : sqrt(det);
  double Pc[6];  // the lane's own column of P = A^-1 J
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = cm[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * Pc[k];
    Pc[i] = s;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) Pc[i] *= rD[i];
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = Pc[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * Pc[k];
    Pc[i] = s;
  }
  // 5. sum_k P_k . H[i, :, k] for i = this lane's joint (the path is the model's: the same trips for every group)
  double acc = 0.0;
  const unsigned char *pa = m.anc + a.frame * m.nj;
  for (int k = 0; k < m.nj; ++k) {
    if (!pa[k]) continue;
    double Pk[6], ck[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      Pk[i] = uniform_bcast<W>(Pc[i], k);
      ck[i] = uniform_bcast<W>(c[i], k);
    }
    // (lane index = joint index, and build_model_image (model_tables.h) refuses a model whose parents do not come before
    // their children: along a path joint order, lane order and column order are one)
    const bool le = li <= k;
    // linear part: w_i x v_k (i <= k), w_k x v_i (i > k);  angular part: w_i x w_k (i <= k), 0 (i > k)
    const double wa[3] = {le ? c[3] : ck[3], le ? c[4] : ck[4], le ? c[5] : ck[5]};
    const double vb[3] = {le ? ck[0] : c[0], le ? ck[1] : c[1], le ? ck[2] : c[2]};
    double hl[3], ha[3];
    cross3(wa, vb, hl);
    cross3(c + 3, ck + 3, ha);
    const double lin = Pk[0] * hl[0] + Pk[1] * hl[1] + Pk[2] * hl[2];
    const double ang = Pk[3] * ha[0] + Pk[4] * ha[1] + Pk[5] * ha[2];
    acc += lin + (le ? ang : 0.0);
  }
  // 6. the row: m * sum in the column of a joint of the path, exact zeros elsewhere; e = -rate
  if (valid && isj) {
    double *Jo = a.J_out + b * a.sJ + (long long)a.row0 * m.nv + my_col;
    const double out = (onpath && !singular) ? mval * acc : 0.0;
    Jo[0] = out;
    if (my_ncol > 1) {
#pragma unroll
      for (int s = 1; s < 6; ++s) Jo[s] = 0.0;
    }
  }
  if (valid && li == 0) {
    a.e_out[b * a.sE + a.row0] = -a.rate;
    if (a.m_out) a.m_out[b] = mval;
  }
}

template <int W>
__global__ void __launch_bounds__(kWave) PINKHIP_OCCUPANCY_FK
ik_manipulability_task_kernel(ManipArgs a) {
  ik_manip_instance<W>(a, block_id());
}

}  // namespace pinkhip
