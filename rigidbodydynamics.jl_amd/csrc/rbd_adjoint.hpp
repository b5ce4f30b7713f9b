// rbd_adjoint.hpp — reverse-mode derivatives of inverse_dynamics! (src/mechanism_algorithms.jl:542-553): for one state, the value τ = ID(q, v, v̇, f_ext)
// and, given a cotangent λ ∈ R^nv, the pullbacks q̄ = (∂τ/∂q)ᵀλ, v̄ = (∂τ/∂v)ᵀλ, v̇̄ = (∂τ/∂v̇)ᵀλ = Mλ and f̄ext = (∂τ/∂f_ext)ᵀλ.  They are exactly the transpose of
// what tangent_rnea_state (rbd_tangent.hpp) differentiates: the RAW coordinates q (a quaternion joint's unnormalised rotation, a SinCosRevolute's (s, c)
// as two coordinates), every tree joint type, any tree size.
//
// Four sweeps over BigModel's tables (the reference's order, parents first):
//   1. parents first: forward kinematics and newton_euler! values, K = (R, p, twist, acceleration) and the body wrench w per body (the arithmetic of
//      tree_kin_step, newton_euler_wrench and joint_torque of rbd_tree_step.hpp, written out here: calling them moved the fp32 kernel off the parent's time);
//   2. children first: the subtree wrenches W_i = w_i + Σ W_child and τ_i = S_iᵀ W_i;
//   3. parents first: W̄_i = S_i λ_i + W̄_parent (f̄ext_i = −W̄_i), and K̄_i from τ_i = ⟨S_i(K_i) λ_i, W_i⟩ and from newton_euler!;
//   4. children first (K̄_i complete: the children have added theirs): the kinematic step pulled back to q̄_i, v̄_i, v̇̄_i and K̄_parent.
// The spatial primitives (xmotion, se3_comm, mul_inertia, momentum_cross, inertia_to_root) have hand-written adjoints below; the joint-local transform
// X(q) is differentiated with Dual<T, N> through the same local_transform every kernel uses, and contracted with its adjoint.
//
// Mapping (rbd_tangent_kernels.hip adjoint_rnea_kernel): one thread per state; the per-body K, W, K̄, W̄ live in an HBM scratch laid out [field][body][thread]
// (coalesced across the wavefront).  The routine is host+device: tests/test_vjp_cpu.py compiles it as plain C++ and runs it against tangent_rnea_state.
#pragma once
#include "rbd_tangent.hpp"

namespace rbd {

enum { ADJ_K = 0, ADJ_W = 24, ADJ_KB = 30, ADJ_WB = 54, ADJ_FIELDS = 60 };  // scratch fields per body: K 24, W 6, K̄ 24, W̄ 6

template <typename T> struct AdjArgs {
  long B;
  const T *q, *v, *vdot, *fext;  // values (vdot, fext nullable)
  const T* lam;                  // the cotangent of τ, nv per state, layout Llam
  Layout Lq, Lv, Lf, Llam;
  T* tau;                            // value of τ (nullable)
  T *qbar, *vbar, *vdbar, *fbar;     // pullbacks times `sign` (each nullable), layouts Lq, Lv, Lv, Lf; overwritten
  T sign;                            // dynamics!: −1 (the implicit-function identity)
  int accum;                         // 1: ADD to qbar, vbar, vdbar, fbar instead of overwriting them (rbd_simulate_vjp sums over stages)
  T* lbar;                           // nullable: λ is added here (Lv; rbd_simulate_vjp's τ̄)
  int fset;                          // 1: fbar is OVERWRITTEN even with accum (rbd_simulate_contact_vjp: the contact pullback needs one stage's f̄ alone)
};

// ---- adjoints of the spatial primitives (rbd_device.hpp): given the output's adjoint ō, ADD the inputs' adjoints ----------------------------------------
// o = a × b
template <typename T> RBD_HD void cross3_adj(const T* a, const T* b, const T* ob, T* ab, T* bb) {
  T x[3], y[3];
  cross3(b, ob, x);
  cross3(ob, a, y);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (ab) ab[k] += x[k];
    if (bb) bb[k] += y[k];
  }
}
// o = R x (R 3×3 row-major)
template <typename T> RBD_HD void matvec3_adj(const T* R, const T* x, const T* ob, T* Rb, T* xb) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (Rb) Rb[3 * i + j] += ob[i] * x[j];
      if (xb) xb[j] += R[3 * i + j] * ob[i];
    }
}
// o = xmotion(R, p, m) = (R m_ang, R m_lin + p × R m_ang)
template <typename T> RBD_HD void xmotion_adj(const T* R, const T* p, const T* m, const T* ob, T* Rb, T* pb, T* mb) {
  T a[3], ab[3] = {ob[0], ob[1], ob[2]};
  matvec3(R, m, a);
  cross3_adj(p, a, ob + 3, pb, ab);
  matvec3_adj(R, m + 3, ob + 3, Rb, mb ? mb + 3 : (T*)nullptr);
  matvec3_adj(R, m, ab, Rb, mb);
}
// o = se3_comm(x, y) = (x_ang × y_ang, x_ang × y_lin + x_lin × y_ang)
template <typename T> RBD_HD void se3_comm_adj(const T* x, const T* y, const T* ob, T* xb, T* yb) {
  cross3_adj(x, y, ob, xb, yb);
  cross3_adj(x, y + 3, ob + 3, xb, yb ? yb + 3 : (T*)nullptr);
  cross3_adj(x + 3, y, ob + 3, xb ? xb + 3 : (T*)nullptr, yb);
}
// the gradient of ⟨a, I b⟩ (mul_inertia) with respect to the inertia's J (6 unique) and c
template <typename T> RBD_HD void inertia_form_adj(const T* a, const T* b, T* Jb, T* cb) {
  Jb[0] += a[0] * b[0];
  Jb[1] += a[0] * b[1] + a[1] * b[0];
  Jb[2] += a[0] * b[2] + a[2] * b[0];
  Jb[3] += a[1] * b[1];
  Jb[4] += a[1] * b[2] + a[2] * b[1];
  Jb[5] += a[2] * b[2];
  T x[3], y[3];
  cross3(b + 3, a, x);
  cross3(b, a + 3, y);
#pragma unroll
  for (int k = 0; k < 3; ++k) cb[k] += x[k] - y[k];
}
// O = inertia_to_root(Jb, mcb, m, R, p) with the body's constants: (Ō.J, Ō.c) → R̄, p̄
template <typename T> RBD_HD void inertia_to_root_adj(const T* Jb, const T* mcb, T m, const T* R, const T* p, const T* OJb, const T* Ocb, T* Rb, T* pb) {
  T Rmc[3], mp[3];
  matvec3(R, mcb, Rmc);
#pragma unroll
  for (int k = 0; k < 3; ++k) mp[k] = m * p[k];
  // O.J = A − Y + tr(Y) 1, O.c = Rmc + mp
  const T tr = OJb[0] + OJb[3] + OJb[5];
  const T Yb[6] = {tr - OJb[0], -OJb[1], -OJb[2], tr - OJb[3], -OJb[4], tr - OJb[5]};
  T Rmcb[3] = {Ocb[0], Ocb[1], Ocb[2]}, mpb[3] = {Ocb[0], Ocb[1], Ocb[2]};
  // Y_ij = Rmc_i p_j + Rmc_j p_i + mp_i p_j (i <= j, the packed order xx xy xz yy yz zz)
  constexpr int PI[6] = {0, 0, 0, 1, 1, 2}, PJ[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    const int i = PI[e], j = PJ[e];
    Rmcb[i] += Yb[e] * p[j];
    Rmcb[j] += Yb[e] * p[i];
    pb[j] += Yb[e] * (Rmc[i] + mp[i]);
    pb[i] += Yb[e] * Rmc[j];
    mpb[i] += Yb[e] * p[j];
  }
  // A = R Jf Rᵀ (A_ij = Σ_k RJ_ik R_jk), RJ = R Jf
  const T Jf[9] = {Jb[0], Jb[1], Jb[2], Jb[1], Jb[3], Jb[4], Jb[2], Jb[4], Jb[5]};
  T RJ[9], RJb[9];
  matmul3(R, Jf, RJ);
#pragma unroll
  for (int k = 0; k < 9; ++k) RJb[k] = T(0);
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    const int i = PI[e], j = PJ[e];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      RJb[3 * i + k] += OJb[e] * R[3 * j + k];
      Rb[3 * j + k] += OJb[e] * RJ[3 * i + k];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int l = 0; l < 3; ++l) Rb[3 * i + l] += RJb[3 * i] * Jf[3 * l] + RJb[3 * i + 1] * Jf[3 * l + 1] + RJb[3 * i + 2] * Jf[3 * l + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) pb[k] += m * mpb[k];
  matvec3_adj(R, mcb, Rmcb, Rb, (T*)nullptr);
}
// w = I a + T ×* (I T) − f_ext with I = inertia_to_root(R, p) (newton_euler!): w̄ → K̄ = (R̄, p̄, T̄, ā)
template <typename T> RBD_HD void newton_euler_adj(const T* rb, const T* K, const T* wb, T* Kb) {
  RInertia<T> I;
  inertia_to_root(rb + RB_J, rb + RB_MC, rb[RB_M], K, K + 9, I);
  const T* Tw = K + 12;
  const T* a = K + 18;
  T Jb[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, cb[3] = {T(0), T(0), T(0)};
  // I a
  T Iw[6];
  mul_inertia(I, wb, Iw);
#pragma unroll
  for (int k = 0; k < 6; ++k) Kb[18 + k] += Iw[k];
  inertia_form_adj(wb, a, Jb, cb);
  // momentum_cross: h = I T, o = (T_ang × h_ang + T_lin × h_lin, T_ang × h_lin)
  T h[6], hb[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  mul_inertia(I, Tw, h);
  cross3_adj(Tw, h, wb, Kb + 12, hb);
  cross3_adj(Tw + 3, h + 3, wb, Kb + 15, hb + 3);
  cross3_adj(Tw, h + 3, wb + 3, Kb + 12, hb + 3);
  T Ih[6];
  mul_inertia(I, hb, Ih);
#pragma unroll
  for (int k = 0; k < 6; ++k) Kb[12 + k] += Ih[k];
  inertia_form_adj(hb, Tw, Jb, cb);
  inertia_to_root_adj(rb + RB_J, rb + RB_MC, rb[RB_M], K, K + 9, Jb, cb, Kb, Kb + 9);
}

// (X̄R, X̄p) of the joint's local transform → q̄ of its first min(nqi, N) coordinates, with Dual<T, N> through local_transform (unit tangents on them)
template <typename T, int N> RBD_HD void local_transform_pullback(int jt, const T* rbt, const T* qv, int nqi, const T* XRb, const T* Xpb, T* qb) {
  using D = Dual<T, N>;
  Body<D> b{};
  b.jtype = jt;
  D rb[RB_STRIDE];
#pragma unroll
  for (int k = 0; k < RB_STRIDE; ++k) rb[k] = D(rbt[k]);
  D qj[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    qj[k] = D(k < nqi ? qv[k] : T(0));
#pragma unroll
    for (int j = 0; j < N; ++j) qj[k].d[j] = (j == k && k < nqi) ? T(1) : T(0);
  }
  D XR[9], Xp[3];
  local_transform(b, rb, qj, XR, Xp);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    T s = T(0);
#pragma unroll
    for (int k = 0; k < 9; ++k) s += XRb[k] * XR[k].d[j];
#pragma unroll
    for (int k = 0; k < 3; ++k) s += Xpb[k] * Xp[k].d[j];
    qb[j] = s;
  }
}

// a joint's coordinates of state `st` (zero past the joint's own, or without the buffer)
template <typename T> RBD_HD void adj_load_q(const AdjArgs<T>& A, long st, int qoff, int nqi, T* qj) {
#pragma unroll
  for (int k = 0; k < 7; ++k) qj[k] = k < nqi ? A.q[(long)(qoff + k) * A.Lq.sk + layout_base(A.Lq, st)] : T(0);
}
template <typename T> RBD_HD void adj_load_v(const T* x, Layout L, long st, int voff, int nvi, T* xj) {
#pragma unroll
  for (int k = 0; k < 6; ++k) xj[k] = (x && k < nvi) ? x[(long)(voff + k) * L.sk + layout_base(L, st)] : T(0);
}

// Sweep 4's step for body i (K̄_i complete): the kinematic step pulled back to q̄_i, v̄_i, v̇̄_i, and its share added to K̄_parent.  `at(field, body)`: the scratch.
// Reads K_i, K_parent and K̄_i; of K only (R, p, twist) — the accelerations enter through K̄ alone.  Shared with point_adjoint_state (rbd_point.hpp).
template <typename T, typename At> RBD_HD void adjoint_kinematic_step(const BigModel& M, const AdjArgs<T>& A, long st, int i, At& at) {
  const T* rbase = reinterpret_cast<const T*>(M.rb);
  Body<T> b{};
  b.parent = M.tbl[4 * i]; b.jtype = M.tbl[4 * i + 1]; b.qoff = M.tbl[4 * i + 2]; b.voff = M.tbl[4 * i + 3];
  b.state = st; b.valid = true; b.orig = i;
  const T* rb = rbase + (long)i * RB_STRIDE;
  const int nqi = joint_nq<T>(b.jtype), nvi = joint_nv(b.jtype);
  T qj[7], vj[6], aj[6];
  adj_load_q(A, st, b.qoff, nqi, qj);
  adj_load_v(A.v, A.Lv, st, b.voff, nvi, vj);
  adj_load_v(A.vdot, A.Lv, st, b.voff, nvi, aj);
  T XR[9], Xp[3], tl[6], al[6], pk[24], K[24], Kb[24], pkb[24];
  local_transform(b, rb, qj, XR, Xp);
  local_joint_motion(b, rb, vj, tl);
  local_joint_motion(b, rb, aj, al);
  if (b.parent >= 0) {
#pragma unroll
    for (int k = 0; k < 24; ++k) pk[k] = at(ADJ_K + k, b.parent);
  } else {
    tree_world_k(M, pk);
  }
#pragma unroll
  for (int k = 0; k < 24; ++k) { K[k] = at(ADJ_K + k, i); Kb[k] = at(ADJ_KB + k, i); pkb[k] = T(0); }
  T tlb[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, alb[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, nT[6], nTb[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  // a = a_parent + se3_comm(−T, T_parent) + xmotion(R, p, a_local)
#pragma unroll
  for (int k = 0; k < 6; ++k) { pkb[18 + k] = Kb[18 + k]; nT[k] = -K[12 + k]; }
  xmotion_adj(K, K + 9, al, Kb + 18, Kb, Kb + 9, alb);
  se3_comm_adj(nT, pk + 12, Kb + 18, nTb, pkb + 12);
  // T = T_parent + xmotion(R, p, t_local)
#pragma unroll
  for (int k = 0; k < 6; ++k) { Kb[12 + k] -= nTb[k]; pkb[12 + k] += Kb[12 + k]; }
  xmotion_adj(K, K + 9, tl, Kb + 12, Kb, Kb + 9, tlb);
  // p = R_parent Xp + p_parent, R = R_parent XR
  T XRb[9] = {T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0), T(0)}, Xpb[3] = {T(0), T(0), T(0)};
#pragma unroll
  for (int k = 0; k < 3; ++k) pkb[9 + k] = Kb[9 + k];
  matvec3_adj(pk, Xp, Kb + 9, pkb, Xpb);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pkb[3 * r + c] += Kb[3 * r] * XR[3 * c] + Kb[3 * r + 1] * XR[3 * c + 1] + Kb[3 * r + 2] * XR[3 * c + 2];  // R̄ XRᵀ
      XRb[3 * r + c] += pk[r] * Kb[c] + pk[3 + r] * Kb[3 + c] + pk[6 + r] * Kb[6 + c];    // R_parentᵀ R̄
    }
  if (b.parent >= 0) {
#pragma unroll
    for (int k = 0; k < 24; ++k) at(ADJ_KB + k, b.parent) += pkb[k];
  }
  // the joint's coordinates: q̄ through the local transform, v̄ and v̇̄ through the (constant) local motion subspace
  if (A.qbar && nqi > 0) {
    T qb[7];
    if (nqi == 1) {
      local_transform_pullback<T, 1>(b.jtype, rb, qj, nqi, XRb, Xpb, qb);
    } else {
      local_transform_pullback<T, 4>(b.jtype, rb, qj, nqi, XRb, Xpb, qb);
      // (a floating joint's translation enters linearly, Xp = X_pred,R q[4:7] + X_pred,p: its three coordinates by hand, the Duals stay 4 wide)
      if (b.jtype == RBD_JOINT_QUAT_FLOATING) matTvec3(rb + RB_XPR, Xpb, qb + 4);
    }
#pragma unroll
    for (int k = 0; k < 7; ++k)
      if (k < nqi) {
        T& o = A.qbar[(long)(b.qoff + k) * A.Lq.sk + layout_base(A.Lq, st)];
        o = A.accum ? o + A.sign * qb[k] : A.sign * qb[k];
      }
  }
  if (A.vbar || A.vdbar) {
    const T ax[3] = {rb[RB_AXIS], rb[RB_AXIS + 1], rb[RB_AXIS + 2]}, ay[3] = {rb[RB_AXIS2], rb[RB_AXIS2 + 1], rb[RB_AXIS2 + 2]};
    for (int k = 0; k < nvi; ++k) {
      T sl[6];
      subspace_col(b.jtype, ax, ay, k, sl);
      const long o = (long)(b.voff + k) * A.Lv.sk + layout_base(A.Lv, st);
      if (A.vbar) A.vbar[o] = A.accum ? A.vbar[o] + A.sign * dot6(sl, tlb) : A.sign * dot6(sl, tlb);
      if (A.vdbar) A.vdbar[o] = A.accum ? A.vdbar[o] + A.sign * dot6(sl, alb) : A.sign * dot6(sl, alb);
    }
  }
}

// inverse_dynamics! and its pullback for state `st`.  sc: scratch, element (field, body) at (field nb + body) ld + slot
template <typename T> RBD_HD void adjoint_rnea_state(const BigModel& M, const AdjArgs<T>& A, long st, T* sc, long ld, long slot) {
  auto at = [&](int f, int i) -> T& { return sc[((long)f * M.nb + i) * ld + slot]; };
  const T* rbase = reinterpret_cast<const T*>(M.rb);
  auto load_q = [&](int qoff, int nqi, T* qj) { adj_load_q(A, st, qoff, nqi, qj); };
  auto load_v = [&](const T* x, Layout L, int voff, int nvi, T* xj) { adj_load_v(x, L, st, voff, nvi, xj); };
  // 1. forward kinematics and newton_euler! (as tree_kin_step and newton_euler_wrench)
  for (int i = 0; i < M.nb; ++i) {
    Body<T> b{};
    b.parent = M.tbl[4 * i]; b.jtype = M.tbl[4 * i + 1]; b.qoff = M.tbl[4 * i + 2]; b.voff = M.tbl[4 * i + 3];
    b.state = st; b.valid = true; b.orig = i;
    const T* rb = rbase + (long)i * RB_STRIDE;
    const int nqi = joint_nq<T>(b.jtype), nvi = joint_nv(b.jtype);
    T qj[7], vj[6], aj[6];
    load_q(b.qoff, nqi, qj);
    load_v(A.v, A.Lv, b.voff, nvi, vj);
    load_v(A.vdot, A.Lv, b.voff, nvi, aj);
    T XR[9], Xp[3], tl[6], al[6], pk[24], K[24];
    local_transform(b, rb, qj, XR, Xp);
    local_joint_motion(b, rb, vj, tl);
    local_joint_motion(b, rb, aj, al);
    if (b.parent >= 0) {
#pragma unroll
      for (int k = 0; k < 24; ++k) pk[k] = at(ADJ_K + k, b.parent);
    } else {
      tree_world_k(M, pk);
    }
    matmul3(pk, XR, K);
    matvec3(pk, Xp, K + 9);
#pragma unroll
    for (int k = 0; k < 3; ++k) K[9 + k] += pk[9 + k];
    T vJ[6], nT[6], cr[6], ajw[6];
    xmotion(K, K + 9, tl, vJ);
#pragma unroll
    for (int k = 0; k < 6; ++k) { K[12 + k] = pk[12 + k] + vJ[k]; nT[k] = -K[12 + k]; }
    se3_comm(nT, pk + 12, cr);
    xmotion(K, K + 9, al, ajw);
#pragma unroll
    for (int k = 0; k < 6; ++k) K[18 + k] = pk[18 + k] + cr[k] + ajw[k];
#pragma unroll
    for (int k = 0; k < 24; ++k) at(ADJ_K + k, i) = K[k];
    RInertia<T> I;
    T Ia[6], x[6];
    inertia_to_root(rb + RB_J, rb + RB_MC, rb[RB_M], K, K + 9, I);
    mul_inertia(I, K + 18, Ia);
    momentum_cross(I, K + 12, x);
#pragma unroll
    for (int k = 0; k < 6; ++k) at(ADJ_W + k, i) = Ia[k] + x[k] - (A.fext ? A.fext[(long)(6 * i + k) * A.Lf.sk + layout_base(A.Lf, st)] : T(0));
  }
  // 2. joint_wrenches_and_torques!: W_i = w_i + Σ W_child, τ_i = S_iᵀ W_i
  for (int i = M.nb - 1; i >= 0; --i) {
    const int jt = M.tbl[4 * i + 1], voff = M.tbl[4 * i + 3], p = M.tbl[4 * i];
    T w[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = at(ADJ_W + k, i);
    if (A.tau) {
      const T* rbt = rbase + (long)i * RB_STRIDE;
      T K[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) K[k] = at(ADJ_K + k, i);
      T out[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
      if (jt == RBD_JOINT_QUAT_FLOATING) {
        xforce_inv(K, K + 9, w, out);
      } else {
        const T ax[3] = {rbt[RB_AXIS], rbt[RB_AXIS + 1], rbt[RB_AXIS + 2]}, ay[3] = {rbt[RB_AXIS2], rbt[RB_AXIS2 + 1], rbt[RB_AXIS2 + 2]};
        for (int k = 0; k < joint_nv(jt); ++k) {
          T sl[6], S[6];
          subspace_col(jt, ax, ay, k, sl);
          xmotion(K, K + 9, sl, S);
          const T dd = dot6(S, w);
          if (k == 0) out[0] = dd; else if (k == 1) out[1] = dd; else out[2] = dd;
        }
      }
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (k < joint_nv(jt)) A.tau[(long)(voff + k) * A.Lv.sk + layout_base(A.Lv, st)] = out[k];
    }
    if (p >= 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) at(ADJ_W + k, p) += w[k];
    }
  }
  // 3. W̄_i = S_i λ_i + W̄_parent, f̄ext_i = −W̄_i; K̄_i from τ_i = ⟨xmotion(K_i, S_local λ_i), W_i⟩ and from newton_euler!
  for (int i = 0; i < M.nb; ++i) {
    Body<T> b{};
    b.parent = M.tbl[4 * i]; b.jtype = M.tbl[4 * i + 1]; b.voff = M.tbl[4 * i + 3];
    const T* rb = rbase + (long)i * RB_STRIDE;
    const int nvi = joint_nv(b.jtype);
    T lj[6], m[6], K[24], W[6], Wb[6], Kb[24];
    load_v(A.lam, A.Llam, b.voff, nvi, lj);
    if (A.lbar)
      for (int k = 0; k < nvi; ++k) A.lbar[(long)(b.voff + k) * A.Lv.sk + layout_base(A.Lv, st)] += lj[k];
    local_joint_motion(b, rb, lj, m);
#pragma unroll
    for (int k = 0; k < 24; ++k) { K[k] = at(ADJ_K + k, i); Kb[k] = T(0); }
#pragma unroll
    for (int k = 0; k < 6; ++k) W[k] = at(ADJ_W + k, i);
    xmotion(K, K + 9, m, Wb);
    if (b.parent >= 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) Wb[k] += at(ADJ_WB + k, b.parent);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      at(ADJ_WB + k, i) = Wb[k];
      if (A.fbar) {
        T& o = A.fbar[(long)(6 * i + k) * A.Lf.sk + layout_base(A.Lf, st)];
        o = A.accum && !A.fset ? o - A.sign * Wb[k] : -A.sign * Wb[k];
      }
    }
    xmotion_adj(K, K + 9, m, W, Kb, Kb + 9, (T*)nullptr);
    newton_euler_adj(rb, K, Wb, Kb);
#pragma unroll
    for (int k = 0; k < 24; ++k) at(ADJ_KB + k, i) = Kb[k];
  }
  // 4. the kinematic step, children first: K̄_i → q̄_i, v̄_i, v̇̄_i and K̄_parent
  for (int i = M.nb - 1; i >= 0; --i) {
    adjoint_kinematic_step<T>(M, A, st, i, at);
  }
}

}  // namespace rbd
