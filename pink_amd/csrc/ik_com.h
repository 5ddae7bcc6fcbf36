// ComTask rows on the device (pink/tasks/com_task.py:88-127): the centre of mass of a kinematic tree and its Jacobian,
// written straight into three rows of the packed e / J streams of the solve kernel, beside the FrameTask rows of
// ik_fk_frame_tasks_kernel (ik_kinematics.h).
//
//   c(q) = sum_k m_k x_k / M,   x_k = R_k c_k + p_k   (joint k's world pose, the centre c_k of the mass m_k attached to it)
//
// Column j of the Jacobian moves exactly the joints of the subtree of joint a = dof_joint[j] (a itself included).  With
// s_a = sum of m_k x_k over that subtree and M_a its mass -- a constant, precomputed on the host --
//   revolute   u x (s_a - M_a p_a) / M        u = R_a axis, the world axis through p_a
//   prismatic  u M_a / M
//   free-flyer (tangent = body twist): linear coordinate i as a prismatic joint along R_a e_i, angular coordinate i as a
//              revolute joint about R_a e_i through p_a (for a root free-flyer M_a = M and s_a = M c: R e_i and
//              (R e_i) x (c - p)).
// This is pin.jacobianCenterOfMass in this project's tangent convention.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pinkhip.h"
#include "ik_kinematics.h"

namespace pinkhip {

// Mass tables in device memory (built by pinkhip_com_create)
struct ComDev {
  const double *mass;              // [nj]
  const double *com;               // [nj, 3]  joint frame
  const double *submass;           // [nj]  mass of the subtree of joint k
  const unsigned long long *desc;  // [nj]  bit k: joint k is in the subtree of this joint (itself included)
  double inv_total;                // 1 / M
};

struct ComArgs {
  ModelDev m;
  ComDev c;
  long long B;
  const double *q;       // [B, nq]
  const double *target;  // [3], or [B, 3] (target_batched)
  int target_batched;
  double *e_out;  // e_out[b sE + row0 + i]
  double *J_out;  // J_out[b sJ + (row0 + i) nv + j]
  long long sE, sJ;
  int row0;
  double *com_out;  // [B, 3] or NULL
};

// ---- host side: the tables of a model's masses, laid out in one buffer (shared by libpinkhip.so and the emulator) ----
struct ComImage {
  std::vector<char> bytes;
  size_t off_mass, off_com, off_submass, off_desc;
  double inv_total;
  int nj;
};

// returns 0, or the PINKHIP_E_* code with the reason in `why`
inline int build_com_image(int model_nj, const int *parent, int nj, const double *mass, const double *com, ComImage &im,
                           std::string &why) {
  if (!mass || !com) {
    why = "mass / com must not be NULL";
    return PINKHIP_E_INVALID;
  }
  if (nj != model_nj) {
    why = "mass tables: nj is not the model's";
    return PINKHIP_E_INVALID;
  }
  if (nj > 64) {
    why = "centre-of-mass rows need nj <= 64 (one lane per joint)";
    return PINKHIP_E_UNSUPPORTED;
  }
  double total = 0.0;
  for (int k = 0; k < nj; ++k) {
    if (!(mass[k] >= 0.0) || !std::isfinite(mass[k])) {
      why = "masses must be finite and not negative";
      return PINKHIP_E_INVALID;
    }
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(com[3 * k + i])) {
        why = "centres must be finite";
        return PINKHIP_E_INVALID;
      }
    total += mass[k];
  }
  if (!(total > 0.0) || !std::isfinite(total)) {
    why = "the total mass must be positive and finite";
    return PINKHIP_E_INVALID;
  }
  std::vector<double> sub(mass, mass + nj);
  std::vector<unsigned long long> desc(nj);
  for (int k = 0; k < nj; ++k) desc[k] = 1ull << k;
  for (int k = nj - 1; k >= 0; --k) {  // (topological order: parent < child)
    const int p = parent[k];
    if (p >= 0) {
      sub[p] += sub[k];
      desc[p] |= desc[k];
    }
  }
  im.nj = nj;
  im.inv_total = 1.0 / total;
  im.bytes.clear();
  auto put = [&](const void *src, size_t n) {
    const size_t off = im.bytes.size();
    im.bytes.resize(off + n);
    std::memcpy(im.bytes.data() + off, src, n);
    return off;
  };
  im.off_mass = put(mass, 8 * (size_t)nj);
  im.off_com = put(com, 8 * 3 * (size_t)nj);
  im.off_submass = put(sub.data(), 8 * (size_t)nj);
  im.off_desc = put(desc.data(), 8 * (size_t)nj);
  return 0;
}

inline ComDev com_view(const ComImage &im, const char *base) {
  ComDev c{};
  c.mass = reinterpret_cast<const double *>(base + im.off_mass);
  c.com = reinterpret_cast<const double *>(base + im.off_com);
  c.submass = reinterpret_cast<const double *>(base + im.off_submass);
  c.desc = reinterpret_cast<const unsigned long long *>(base + im.off_desc);
  c.inv_total = im.inv_total;
  return c;
}

// what pinkhip_com_task_device refuses before anything is enqueued (NULL: nothing)
inline const char *com_task_fault(const ComArgs &a) {
  if (a.B < 0 || a.B > 0x7fffffffLL) return "bad B";
  if (a.B == 0) return nullptr;
  if (!a.q || !a.target || !a.e_out || !a.J_out) return "null pointer";
  if (a.row0 < 0) return "row0 must not be negative";
  if (a.sE < a.row0 + 3 || a.sJ < (long long)(a.row0 + 3) * a.m.nv) return "strides smaller than the rows";
  return nullptr;
}

// The centre of mass of one instance and its Jacobian by a group of W lanes (W >= nj), the mapping of ik_fk_instance:
//   1.-2. lane = joint: pose in the parent frame, pointer jumping to world poses (compose_world_poses);
//   3. lane = joint k: first moment m_k x_k, kept in registers;
//   4. lane = tangent column j: nj broadcast steps sum the moments of the joints in the subtree of the column's joint
//      (descendant bit mask) and of all joints; no LDS traffic in that loop;
//   5. the column, stored by column lane: consecutive lanes write consecutive addresses of a row of J.
template <int W>
__device__ __forceinline__ void ik_com_instance(const ComArgs &a, long long block) {
  const ModelDev &m = a.m;
  const GroupLane gl = group_lane<W>(block, a.B, m.nj);
  const int li = gl.li, jl = gl.jl;
  const long long b = gl.b;
  const bool valid = gl.valid, isj = gl.isj;
  double *oM = shared_base() + (long long)gl.g * pose_lds_doubles(m.nj);
  const double *q = a.q + b * (long long)m.nq;

  // The tables of this lane's joint and of its first tangent column are requested before the poses are composed (the
  // kernel is bound by dependent round trips, as ik_fk_instance is)
  const double mk = isj ? a.c.mass[jl] : 0.0;
  const double ck0 = a.c.com[3 * jl], ck1 = a.c.com[3 * jl + 1], ck2 = a.c.com[3 * jl + 2];
  const int j0 = li < m.nv ? li : 0;
  const int pf_jt = m.dof_joint[j0], pf_sub = m.dof_sub[j0], pf_ty = m.jtype[pf_jt];
  const double pf_ax[3] = {m.axis[3 * pf_jt], m.axis[3 * pf_jt + 1], m.axis[3 * pf_jt + 2]};
  const unsigned long long pf_desc = a.c.desc[pf_jt];
  const double pf_sub_mass = a.c.submass[pf_jt];
  const int ti = li < 3 ? li : 0;
  const double tgt = a.target[(a.target_batched ? 3 * b : 0) + ti];

  // 1.-2. world pose of joint li, in this lane's registers and (all joints) in oM
  const Pose X = compose_world_poses(m, gl, joint_pose_in_parent(m, jl, q + m.idx_q[jl]), oM);
  const double(&T)[12] = X.T;
  // 3. first moment of the mass attached to joint li (a lane without a joint, or a massless joint: exactly zero)
  double mx[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double x = T[3 * i] * ck0 + T[3 * i + 1] * ck1 + T[3 * i + 2] * ck2 + T[9 + i];
    mx[i] = (isj && mk != 0.0) ? mk * x : 0.0;
  }
  const double invM = a.c.inv_total;
  double ct[3] = {0.0, 0.0, 0.0};
  // 4. lane = tangent column (every lane runs the same number of passes: the broadcasts are group-wide)
  for (int jb = 0; jb < m.nv; jb += W) {
    const int j = jb + li;
    const bool on = j < m.nv, first = jb == 0;
    const int jc = on ? j : 0;
    const int jt = first ? pf_jt : m.dof_joint[jc], sub = first ? pf_sub : m.dof_sub[jc], ty = first ? pf_ty : m.jtype[jt];
    const unsigned long long D = first ? pf_desc : a.c.desc[jt];
    const double Ma = first ? pf_sub_mass : a.c.submass[jt];
    double s[3] = {0.0, 0.0, 0.0};
    ct[0] = ct[1] = ct[2] = 0.0;
    for (int k = 0; k < m.nj; ++k) {
      const bool in = ((D >> k) & 1ull) != 0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double v = uniform_bcast<W>(mx[i], k);
        ct[i] += v;
        s[i] += in ? v : 0.0;
      }
    }
    const double *Xj = oM + 12 * jt;  // world pose of the column's joint
    double ax[3], u[3];
    if (ty == JOINT_FREE_FLYER) {
      const int k = sub % 3;
      ax[0] = k == 0 ? 1.0 : 0.0;
      ax[1] = k == 1 ? 1.0 : 0.0;
      ax[2] = k == 2 ? 1.0 : 0.0;
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) ax[i] = first ? pf_ax[i] : m.axis[3 * jt + i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = Xj[3 * i] * ax[0] + Xj[3 * i + 1] * ax[1] + Xj[3 * i + 2] * ax[2];
    const bool angular = (ty == JOINT_REVOLUTE) || (ty == JOINT_FREE_FLYER && sub >= 3);
    double col[3];
    if (angular) {  // u x (s - M_a p_a) / M
      const double r0 = (s[0] - Ma * Xj[9]) * invM, r1 = (s[1] - Ma * Xj[10]) * invM, r2 = (s[2] - Ma * Xj[11]) * invM;
      col[0] = u[1] * r2 - u[2] * r1;
      col[1] = u[2] * r0 - u[0] * r2;
      col[2] = u[0] * r1 - u[1] * r0;
    } else {  // u M_a / M
      const double w = Ma * invM;
      col[0] = u[0] * w, col[1] = u[1] * w, col[2] = u[2] * w;
    }
    if (valid && on) {
      double *Jo = a.J_out + b * a.sJ + (long long)a.row0 * m.nv + j;
#pragma unroll
      for (int i = 0; i < 3; ++i) Jo[(long long)i * m.nv] = col[i];
    }
  }
  // 5. the error (task.compute_error: actual minus target) and the centre itself, by the first three lanes of the group
  if (valid && li < 3) {
    const double ci = (li == 0 ? ct[0] : li == 1 ? ct[1] : ct[2]) * invM;
    a.e_out[b * a.sE + a.row0 + li] = ci - tgt;
    if (a.com_out) a.com_out[3 * b + li] = ci;
  }
}

template <int W>
__global__ void __launch_bounds__(kWave) PINKHIP_OCCUPANCY_FK
ik_com_task_kernel(ComArgs a) {
  ik_com_instance<W>(a, block_id());
}

}  // namespace pinkhip
