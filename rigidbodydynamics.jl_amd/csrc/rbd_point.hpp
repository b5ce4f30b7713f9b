// rbd_point.hpp — batched point kinematics (rbd_point_kinematics, rbd_point_kinematics_vjp): for P points fixed to bodies (rbd_workspace_set_points), expressed
// in the root frame with paths from the world,
//   pos = R_b r + p_b                       transform(state, point, world)
//   vel = ω_b × pos + v_b                   point_velocity (src/spatial/spatialmotion.jl:346), (ω_b; v_b) = twist_wrt_world
//   acc = α_b × pos + a_b + ω_b × vel       point_acceleration (:358-362), (α_b; a_b) the body's spatial acceleration relative to the world (no gravity)
//   jac = ang(S) × pos + lin(S) per velocity coordinate of a joint on path(world → body), zero elsewhere: point_jacobian! (src/mechanism_algorithms.jl:168-189)
// and the pullback of (pos, vel) to the RAW coordinates q (as rbd_adjoint.hpp defines them) and v.
//
// Forward (point_kin_state; kernel: rbd_point_kernels.hip point_kin_kernel): one thread per (point, state) walks the point's path root-first with
// (R, p, twist, acceleration) in registers — point_body_step, the in-place form of tree_kin_step (rbd_tree_step.hpp) —, and, when the Jacobian is asked for, walks it a second time
// recomputing (R, p) per body and writing the joint's columns.  No scratch, no LDS.  The routine is templated on the scalar, so that it also instantiates on
// Dual<double, 1>: tests/test_point_kinematics_cpu.py takes J·d from that instantiation and checks the pullback against it.
//
// Reverse (point_adjoint_state; kernel: point_adjoint_kernel): one thread per state over the parents-first union of the paths.  Sweep A is tree_kin_step<false>
// (K = (R, p, twist) into the adjoint scratch) and seeds K̄ from the cotangents of the points on each body; sweep B is sweep 4 of adjoint_rnea_state
// (adjoint_kinematic_step), children first.
#pragma once
#include "rbd_adjoint.hpp"

namespace rbd {

// the points of a workspace on the device.  path: for point k the bodies of path(world → body[k]), root first, at path[poff[k]] … path[poff[k + 1] − 1];
// uni: the union of those paths, parents first (ascending body index); the points fixed to uni[u] are upts[ubeg[u]] … upts[ubeg[u + 1] − 1]
struct PointPlan {
  int32_t np, nu;
  const int32_t* poff;
  const int32_t* path;
  const int32_t* uni;
  const int32_t* ubeg;
  const int32_t* upts;
  const void* r;  // [3 np] of the kernel's scalar type, each in its body's frame
};

template <typename T> struct PointArgs {
  long B;
  const T *q, *v, *vdot;  // v: needed by vel and acc; vdot nullable (zero)
  Layout Lq, Lv, L3, Lj;  // L3: 3 np values per state; Lj: 3 nv np
  T *pos, *vel, *acc, *jac;  // each nullable
};

template <typename T> struct PointAdjArgs {
  const T *pos_bar, *vel_bar;  // 3 np per state, layout L3; each nullable (zero)
  Layout L3;
};

// the scalar under a Dual
template <typename S> struct ScalarOf { using type = S; };
template <typename T, int N> struct ScalarOf<Dual<T, N>> { using type = T; };

// One body's kinematic step from its parent's (R, p, twist Tw, acceleration a), in place; `motion`: twist and acceleration too (else only R, p).
// qj, vj, aj: the joint's coordinates (zero past its own).
template <typename S> RBD_HD void point_body_step(int jt, const S* rb, const S* qj, const S* vj, const S* aj, bool motion, S* R, S* p, S* Tw, S* a) {
  Body<S> b{};
  b.jtype = jt;
  S XR[9], Xp[3], t3[3];
  local_transform(b, rb, qj, XR, Xp);
  matvec3(R, Xp, t3);
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] += t3[k];
  matmul3(R, XR, R);
  if (motion) {
    S tl[6], al[6], vJ[6], nT[6], cr[6], ajw[6];
    local_joint_motion(b, rb, vj, tl);
    local_joint_motion(b, rb, aj, al);
    xmotion(R, p, tl, vJ);
#pragma unroll
    for (int k = 0; k < 6; ++k) nT[k] = -(Tw[k] + vJ[k]);
    se3_comm(nT, Tw, cr);  // (−T_body) × T_parent
    xmotion(R, p, al, ajw);
#pragma unroll
    for (int k = 0; k < 6; ++k) { Tw[k] = Tw[k] + vJ[k]; a[k] = a[k] + cr[k] + ajw[k]; }
  }
}

// Point kinematics of one (point, state).  path: the n bodies of the point's path, root first; r: the point in its body's frame; coordinates come through
// lq(row) / lv(row) / la(row) (a Dual scalar loads its tangent there).  pos, vel, acc: 3 values each, always formed (vel, acc from zero motion without v).
// jac(col, c, x): stores component c of the column of velocity coordinate col — called for the path's columns only, and not at all when !want_jac.
template <typename S, typename LQ, typename LV, typename LA, typename JO>
RBD_HD void point_kin_state(const BigModel& M, const int32_t* path, int n, const S* r, bool motion, bool want_jac, LQ lq, LV lv, LA la, JO jac, S* pos, S* vel, S* acc) {
  using T = typename ScalarOf<S>::type;
  const T* rbase = reinterpret_cast<const T*>(M.rb);
  auto body = [&](int i, int* jt, int* voff, S* rb, S* qj, S* vj, S* aj, bool mot) {
    *jt = M.tbl[4 * i + 1];
    const int qoff = M.tbl[4 * i + 2];
    *voff = M.tbl[4 * i + 3];
    const int nqi = joint_nq<T>(*jt), nvi = joint_nv(*jt);
    // (the constants the kinematic step reads: axes and joint_to_predecessor, not the inertia)
#pragma unroll
    for (int k = 0; k < RB_J; ++k) rb[k] = S(rbase[(long)i * RB_STRIDE + k]);
#pragma unroll
    for (int k = 0; k < 7; ++k) qj[k] = k < nqi ? lq(qoff + k) : S(T(0));
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      vj[k] = (mot && k < nvi) ? lv(*voff + k) : S(T(0));
      aj[k] = (mot && k < nvi) ? la(*voff + k) : S(T(0));
    }
  };
  S R[9], p[3], Tw[6], a[6];
  auto world = [&]() {  // (as tree_world_k, without its −g: the accelerations here are relative to the world)
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = S(k % 4 == 0 ? T(1) : T(0));
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = S(T(0));
#pragma unroll
    for (int k = 0; k < 6; ++k) { Tw[k] = S(T(0)); a[k] = S(T(0)); }
  };
  // pass 1: root first, (R, p, twist, acceleration) in registers
  world();
  for (int j = 0; j < n; ++j) {
    int jt, voff;
    S rb[RB_J], qj[7], vj[6], aj[6];
    body(path[j], &jt, &voff, rb, qj, vj, aj, motion);
    point_body_step(jt, rb, qj, vj, aj, motion, R, p, Tw, a);
  }
  S t3[3], u3[3], w3[3];
  matvec3(R, r, t3);
#pragma unroll
  for (int k = 0; k < 3; ++k) pos[k] = t3[k] + p[k];
  cross3(Tw, pos, t3);
#pragma unroll
  for (int k = 0; k < 3; ++k) vel[k] = t3[k] + Tw[3 + k];
  cross3(a, pos, u3);
  cross3(Tw, vel, w3);
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[k] = u3[k] + a[3 + k] + w3[k];
  if (!want_jac) return;
  // pass 2: the path again, (R, p) recomputed per body; a joint's columns are ang(S) × pos + lin(S) with S its motion subspace in the root frame
  world();
  for (int j = 0; j < n; ++j) {
    int jt, voff;
    S rb[RB_J], qj[7], vj[6], aj[6];
    body(path[j], &jt, &voff, rb, qj, vj, aj, false);
    point_body_step(jt, rb, qj, vj, aj, false, R, p, Tw, a);
    const S ax[3] = {rb[RB_AXIS], rb[RB_AXIS + 1], rb[RB_AXIS + 2]}, ay[3] = {rb[RB_AXIS2], rb[RB_AXIS2 + 1], rb[RB_AXIS2 + 2]};
    const int nvi = joint_nv(jt);
    for (int k = 0; k < nvi; ++k) {
      S sl[6], Sw[6], c3[3];
      subspace_col(jt, ax, ay, k, sl);
      xmotion(R, p, sl, Sw);
      cross3(Sw, pos, c3);
#pragma unroll
      for (int c = 0; c < 3; ++c) jac(voff + k, c, c3[c] + Sw[3 + c]);
    }
  }
}

// (q̄, v̄) = Jᵀ(pos_bar, vel_bar) for state `st` over the union of the paths.  A: q, v and their layouts, qbar / vbar (overwritten: zero off the union; added to with accum), sign 1,
// no vdot.  sc: the adjoint scratch of adjoint_rnea_state, element (field, body) at (field nb + body) ld + slot; only K and K̄ are used.
template <typename T> RBD_HD void point_adjoint_state(const BigModel& M, const PointPlan& P, const AdjArgs<T>& A, const PointAdjArgs<T>& C, long st, T* sc, long ld, long slot) {
  auto at = [&](int f, int i) -> T& { return sc[((long)f * M.nb + i) * ld + slot]; };
  const T* rbase = reinterpret_cast<const T*>(M.rb);
  const T* rpt = reinterpret_cast<const T*>(P.r);
  // the coordinates of joints off every path take no part (A.accum: the pullback is ADDED to what qbar / vbar hold — rbd_dynamics_contact_vjp)
  if (A.qbar && !A.accum)
    for (int k = 0; k < M.nq; ++k) A.qbar[(long)k * A.Lq.sk + layout_base(A.Lq, st)] = T(0);
  if (A.vbar && !A.accum)
    for (int k = 0; k < M.nv; ++k) A.vbar[(long)k * A.Lv.sk + layout_base(A.Lv, st)] = T(0);
  // A. parents first: K = (R, p, twist) (tree_kin_step<false>, rbd_tree_step.hpp), and K̄ seeded by the points on the body
  for (int u = 0; u < P.nu; ++u) {
    const int i = P.uni[u];
    const Body<T> b = tree_body<T>(M, i, st);
    const T* rb = rbase + (long)i * RB_STRIDE;
    T qj[7], vj[6], K[18];
    adj_load_q(A, st, b.qoff, joint_nq<T>(b.jtype), qj);
    adj_load_v(A.v, A.Lv, st, b.voff, joint_nv(b.jtype), vj);
    tree_kin_step<false>(b, rb, qj, vj, (const T*)nullptr, [&](T* pk) {
      if (b.parent >= 0) {
#pragma unroll
        for (int k = 0; k < 18; ++k) pk[k] = at(ADJ_K + k, b.parent);
      } else {
        tree_world_k(M, pk);
      }
    }, K);
#pragma unroll
    for (int k = 0; k < 18; ++k) at(ADJ_K + k, i) = K[k];
    T Kb[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) Kb[k] = T(0);
    for (int e = P.ubeg[u]; e < P.ubeg[u + 1]; ++e) {
      const int pt = P.upts[e];
      const T r[3] = {rpt[3 * pt], rpt[3 * pt + 1], rpt[3 * pt + 2]};
      T pb[3], vb[3], pos[3], x[3], y[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const long o = (long)(3 * pt + k) * C.L3.sk + layout_base(C.L3, st);
        pb[k] = C.pos_bar ? C.pos_bar[o] : T(0);
        vb[k] = C.vel_bar ? C.vel_bar[o] : T(0);
      }
      matvec3(K, r, pos);
#pragma unroll
      for (int k = 0; k < 3; ++k) pos[k] += K[9 + k];
      // vel = ω × pos + v_lin, pos = R r + p
      cross3(vb, K + 12, x);  // p̄ = pos_bar + vel_bar × ω
      cross3(pos, vb, y);     // ω̄ += pos × vel_bar
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const T pbar = pb[k] + x[k];
        Kb[3 * k] += pbar * r[0]; Kb[3 * k + 1] += pbar * r[1]; Kb[3 * k + 2] += pbar * r[2];  // R̄ += p̄ rᵀ
        Kb[9 + k] += pbar;
        Kb[12 + k] += y[k];
        Kb[15 + k] += vb[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 24; ++k) at(ADJ_KB + k, i) = Kb[k];
  }
  // B. children first: sweep 4 of adjoint_rnea_state
  for (int u = P.nu - 1; u >= 0; --u) adjoint_kinematic_step<T>(M, A, st, P.uni[u], at);
}

}  // namespace rbd
