// rbd_tree_step.hpp — the per-state tree recursion of inverse_dynamics! (src/mechanism_algorithms.jl:542-553) over BigModel's tables, one body at a
// time: what the any-size kernels (rbd_big_kernels.hip), the tangent and adjoint RNEA (rbd_tangent.hpp, rbd_adjoint.hpp) and the point pullback
// (rbd_point.hpp) share.  Every routine is templated on the scalar S (T, or Dual<T, N> of rbd_tangent.hpp) and host+device — the CPU tests compile
// them as plain C++.  The caller owns the scratch: it hands over how the parent's entry is loaded, stores the body's, and adds its own external wrench.
//   K = (R 9, p 3, twist 6, acceleration 6) of a body in the root frame, 24 values.
#pragma once
#include "rbd_lane.hpp"

namespace rbd {

// body i's table entry (the reference's order, parents first) for state `st`
template <typename S> RBD_HD Body<S> tree_body(const BigModel& M, int i, long st) {
  Body<S> b{};
  b.parent = M.tbl[4 * i]; b.jtype = M.tbl[4 * i + 1]; b.qoff = M.tbl[4 * i + 2]; b.voff = M.tbl[4 * i + 3];
  b.state = st; b.valid = true; b.orig = i;
  return b;
}

// the world's entry: identity, at rest, a = −g
template <typename S> RBD_HD void tree_world_k(const BigModel& M, S* pk) {
#pragma unroll
  for (int k = 0; k < 24; ++k) pk[k] = S((k < 9 && k % 4 == 0) ? 1 : 0);
  pk[21] = S(-M.gravity[0]); pk[22] = S(-M.gravity[1]); pk[23] = S(-M.gravity[2]);
}

// K of body b from its parent's; qj, vj, aj: the joint's coordinates (zero past its own).  parent_k(pk) fills the parent's entry from the caller's scratch,
// or with tree_world_k — a callable, so that the loads stay behind the joint's local transform, where every kernel had them (the registers they take).
// ACC adds the acceleration with the joint's X S_local v̇ (spatial_accelerations! :387-417): a = a_parent + (−T) × T_parent + X a_local; without it only
// (R, p, twist): K[0 … 18) from pk[0 … 18), aj unused
template <bool ACC = true, typename S, typename PK> RBD_HD void tree_kin_step(const Body<S>& b, const S* rb, const S* qj, const S* vj, const S* aj, PK parent_k, S* K) {
  S XR[9], Xp[3], tl[6], al[6], pk[24];
  local_transform(b, rb, qj, XR, Xp);
  local_joint_motion(b, rb, vj, tl);
  if (ACC) local_joint_motion(b, rb, aj, al);
  parent_k(pk);
  matmul3(pk, XR, K);
  matvec3(pk, Xp, K + 9);
#pragma unroll
  for (int k = 0; k < 3; ++k) K[9 + k] += pk[9 + k];
  S vJ[6], nT[6], cr[6], ajw[6];
  xmotion(K, K + 9, tl, vJ);
#pragma unroll
  for (int k = 0; k < 6; ++k) { K[12 + k] = pk[12 + k] + vJ[k]; nT[k] = -K[12 + k]; }
  if (!ACC) return;
  se3_comm(nT, pk + 12, cr);
  xmotion(K, K + 9, al, ajw);
#pragma unroll
  for (int k = 0; k < 6; ++k) K[18 + k] = pk[18 + k] + cr[k] + ajw[k];
}

// newton_euler! (:428-439) without the external wrench: w = I a + T ×* I T in the root frame
template <typename S> RBD_HD void newton_euler_wrench(const S* rb, const S* K, S* w) {
  RInertia<S> I;
  S Ia[6], x[6];
  inertia_to_root(rb + RB_J, rb + RB_MC, rb[RB_M], K, K + 9, I);
  mul_inertia(I, K + 18, Ia);
  momentum_cross(I, K + 12, x);
#pragma unroll
  for (int k = 0; k < 6; ++k) w[k] = Ia[k] + x[k];
}

// joint_wrenches_and_torques! (:442-459) for one joint: out[0 … nv_joint) = Sᵀ w, zero past them.  rb: the body's constants, of the scalar or its base type
template <typename S, typename C> RBD_HD void joint_torque(int jt, const C* rb, const S* K, const S* w, S* out) {
#pragma unroll
  for (int k = 0; k < 6; ++k) out[k] = S(0);
  if (jt == RBD_JOINT_QUAT_FLOATING) {
    xforce_inv(K, K + 9, w, out);
  } else {
    const S ax[3] = {S(rb[RB_AXIS]), S(rb[RB_AXIS + 1]), S(rb[RB_AXIS + 2])}, ay[3] = {S(rb[RB_AXIS2]), S(rb[RB_AXIS2 + 1]), S(rb[RB_AXIS2 + 2])};
    for (int k = 0; k < joint_nv(jt); ++k) {
      S sl[6], Sc[6];
      subspace_col(jt, ax, ay, k, sl);
      xmotion(K, K + 9, sl, Sc);
      const S d = dot6(Sc, w);
      if (k == 0) out[0] = d; else if (k == 1) out[1] = d; else out[2] = d;
    }
  }
}

}  // namespace rbd
