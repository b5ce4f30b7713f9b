// rbd_tangent.hpp — forward-mode derivatives of inverse_dynamics! (src/mechanism_algorithms.jl:542-553): the value and N tangents of every
// per-body quantity carried together through spatial_accelerations! (:387-417), newton_euler! (:428-439) and joint_wrenches_and_torques! (:442-459).
// This is what ForwardDiff.Dual with a chunk of N partials computes through the reference: the derivative of the function the library evaluates,
// in the RAW coordinates q (a quaternion joint's rotation is the unnormalised formula, rot_quat; a SinCosRevolute's (s, c) are two coordinates).
//
// The scalar type Dual<T, N> runs through the same templated primitives as every other kernel (rbd_lane.hpp / rbd_device.hpp); the constants of the
// mechanism enter as Duals with zero tangents, and rbd_tangent_kernels.hip is compiled with finite-math and no signed zeros so that the products with
// those zeros fold away.  The per-state routine is host+device: tests/test_derivatives_cpu.py compiles it as plain C++ and runs it against the oracle.
//
// Mapping: one thread per (state, chunk of N directions), thread t = chunk · B + state; the per-body values and tangents live in an HBM scratch laid
// out [field][component][body][thread] (coalesced across the wavefront, as in rbd_big_kernels.hip).  Bodies in the reference's order (parents first):
// the tables are BigModel's, built for every tree mechanism.
#pragma once
#include "rbd_tree_step.hpp"

namespace rbd {

template <typename T, int N> struct Dual {
  T v;
  T d[N];
  RBD_HD Dual() {}
  RBD_HD Dual(T x) : v(x) {
#pragma unroll
    for (int j = 0; j < N; ++j) d[j] = T(0);
  }
  RBD_HD Dual& operator+=(const Dual& b) {
    v += b.v;
#pragma unroll
    for (int j = 0; j < N; ++j) d[j] += b.d[j];
    return *this;
  }
  RBD_HD Dual& operator-=(const Dual& b) {
    v -= b.v;
#pragma unroll
    for (int j = 0; j < N; ++j) d[j] -= b.d[j];
    return *this;
  }
  friend RBD_HD Dual operator-(const Dual& a) {
    Dual r;
    r.v = -a.v;
#pragma unroll
    for (int j = 0; j < N; ++j) r.d[j] = -a.d[j];
    return r;
  }
  friend RBD_HD Dual operator+(const Dual& a, const Dual& b) { Dual r = a; r += b; return r; }
  friend RBD_HD Dual operator-(const Dual& a, const Dual& b) { Dual r = a; r -= b; return r; }
  friend RBD_HD Dual operator+(const Dual& a, T b) { Dual r = a; r.v += b; return r; }
  friend RBD_HD Dual operator+(T a, const Dual& b) { Dual r = b; r.v += a; return r; }
  friend RBD_HD Dual operator-(const Dual& a, T b) { Dual r = a; r.v -= b; return r; }
  friend RBD_HD Dual operator-(T a, const Dual& b) { Dual r = -b; r.v += a; return r; }
  friend RBD_HD Dual operator*(const Dual& a, const Dual& b) {
    Dual r;
    r.v = a.v * b.v;
#pragma unroll
    for (int j = 0; j < N; ++j) r.d[j] = a.d[j] * b.v + a.v * b.d[j];
    return r;
  }
  friend RBD_HD Dual operator*(T a, const Dual& b) {
    Dual r;
    r.v = a * b.v;
#pragma unroll
    for (int j = 0; j < N; ++j) r.d[j] = a * b.d[j];
    return r;
  }
  friend RBD_HD Dual operator*(const Dual& a, T b) { return b * a; }
  friend RBD_HD Dual operator/(const Dual& a, T b) { return (T(1) / b) * a; }
};

// the transcendental pieces of the joint transforms (revolute: sincos_fast, planar: sincos_t), with their derivatives
template <typename T, int N> RBD_HD void sincos_fast(const Dual<T, N>& x, Dual<T, N>* s, Dual<T, N>* c) {
  T sv, cv;
  sincos_fast(x.v, &sv, &cv);
  s->v = sv; c->v = cv;
#pragma unroll
  for (int j = 0; j < N; ++j) { s->d[j] = cv * x.d[j]; c->d[j] = -sv * x.d[j]; }
}
template <typename T, int N> RBD_HD void sincos_t(const Dual<T, N>& x, Dual<T, N>* s, Dual<T, N>* c) {
  T sv, cv;
  sincos_t(x.v, &sv, &cv);
  s->v = sv; c->v = cv;
#pragma unroll
  for (int j = 0; j < N; ++j) { s->d[j] = cv * x.d[j]; c->d[j] = -sv * x.d[j]; }
}

// where the tangent of direction `col` (0-based within the call) of a state goes: columns < split to a, the others to b at col - split; rows of n
template <typename T> struct ColOut {
  T* a; Layout La;
  T* b; Layout Lb;
  int split, n;
  // every column to one buffer
  static RBD_HD ColOut single(T* p, Layout L, int n) { return ColOut{p, L, nullptr, Layout{0, 0}, INT32_MAX, n}; }
  RBD_HD T* at(int col, int row, long st) const {
    if (col < split) return a ? a + ((long)col * n + row) * La.sk + layout_base(La, st) : nullptr;
    return b ? b + ((long)(col - split) * n + row) * Lb.sk + layout_base(Lb, st) : nullptr;
  }
};

enum { TAN_K = 0, TAN_W = 24, TAN_FIELDS = 30 };  // scratch fields per body: K = R 9, p 3, twist 6, acceleration 6; wrench 6

template <typename T> struct TanArgs {
  long B;
  int ntan;  // directions of the call
  int unit;  // 1: direction g0 + e is the coordinate unit vector of (q; v) — column g0 + e < nq of ∂/∂q, else of ∂/∂v (the Jacobians); tangent inputs unused
  int g0;
  const T *q, *v, *vdot, *fext;      // values (vdot, fext nullable)
  const T *dq, *dv, *dvdot, *dfext;  // tangents (nullable = zero direction), direction e of state b at rows e·n … of the state's n·ntan
  Layout Lq, Lv, Lf, Ldq, Ldv, Ldf;
  T* tau;  // value of τ (nullable; the threads of chunk 0 write it)
  ColOut<T> out;  // tangent of τ, times `sign`, plus `dadd` (nullable, layout Ldv: rows e·nv …): dynamics! forms dτ − ∂ID·(dq, dv, 0, dfext) in one pass
  T sign;
  const T* dadd;
};

// inverse_dynamics! with N tangents for state `st`, directions chunk·N … chunk·N + N − 1 of the call.  sc: scratch, element (field, component, body)
// at ((field (N + 1) + component) nb + body) ld + slot.  `mid(get, put)` runs between the two sweeps, when every body's K and wrench (with their tangents) are
// in the scratch: get(field, body) / put(field, body, x) are the scratch's accessors; it returns whether the wrench sweep runs.  The plain pass hands in a
// functor that does nothing (tangent_rnea_state below); the contact variant forms the tangents of the contact wrenches there (tangent_contact_state).
template <typename T, int N, typename Mid>
RBD_HD void tangent_rnea_sweeps(const BigModel& M, const TanArgs<T>& A, long st, int chunk, T* sc, long ld, long slot, Mid mid) {
  using D = Dual<T, N>;
  auto at = [&](int f, int c, int i) -> T& { return sc[(((long)f * (N + 1) + c) * M.nb + i) * ld + slot]; };
  auto get = [&](int f, int i) {
    D x;
    x.v = at(f, 0, i);
#pragma unroll
    for (int j = 0; j < N; ++j) x.d[j] = at(f, 1 + j, i);
    return x;
  };
  auto put = [&](int f, int i, const D& x) {
    at(f, 0, i) = x.v;
#pragma unroll
    for (int j = 0; j < N; ++j) at(f, 1 + j, i) = x.d[j];
  };
  const int e0 = chunk * N;
  const T* rbase = reinterpret_cast<const T*>(M.rb);
  // a tangent input of n coordinates per direction: row r of direction e0 + j (zero past the call's directions or without the buffer)
  auto tan_in = [&](const T* x, Layout L, int n, int r, int j) -> T {
    return (x && e0 + j < A.ntan) ? x[((long)(e0 + j) * n + r) * L.sk + layout_base(L, st)] : T(0);
  };
  auto unit_hit = [&](int g, int j) -> T { return (A.unit && e0 + j < A.ntan && A.g0 + e0 + j == g) ? T(1) : T(0); };
  for (int i = 0; i < M.nb; ++i) {
    const Body<D> b = tree_body<D>(M, i, st);
    const T* rbt = rbase + (long)i * RB_STRIDE;
    D rb[RB_STRIDE];
#pragma unroll
    for (int k = 0; k < RB_STRIDE; ++k) rb[k] = D(rbt[k]);
    const int nqi = joint_nq<T>(b.jtype), nvi = joint_nv(b.jtype);
    D qj[7], vj[6], aj[6];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      qj[k] = D(k < nqi ? A.q[(long)(b.qoff + k) * A.Lq.sk + layout_base(A.Lq, st)] : T(0));
#pragma unroll
      for (int j = 0; j < N; ++j) qj[k].d[j] = k < nqi ? (A.unit ? unit_hit(b.qoff + k, j) : tan_in(A.dq, A.Ldq, M.nq, b.qoff + k, j)) : T(0);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const bool in = k < nvi;
      vj[k] = D(in ? A.v[(long)(b.voff + k) * A.Lv.sk + layout_base(A.Lv, st)] : T(0));
      aj[k] = D(in && A.vdot ? A.vdot[(long)(b.voff + k) * A.Lv.sk + layout_base(A.Lv, st)] : T(0));
#pragma unroll
      for (int j = 0; j < N; ++j) {
        vj[k].d[j] = in ? (A.unit ? unit_hit(M.nq + b.voff + k, j) : tan_in(A.dv, A.Ldv, M.nv, b.voff + k, j)) : T(0);
        aj[k].d[j] = (in && !A.unit) ? tan_in(A.dvdot, A.Ldv, M.nv, b.voff + k, j) : T(0);
      }
    }
    // forward kinematics from the parent's entry (tree_kin_step, rbd_tree_step.hpp)
    D K[24], w[6];
    tree_kin_step(b, rb, qj, vj, aj, [&](D* pk) {
      if (b.parent >= 0) {
#pragma unroll
        for (int k = 0; k < 24; ++k) pk[k] = get(TAN_K + k, b.parent);
      } else {
        tree_world_k(M, pk);
      }
    }, K);
#pragma unroll
    for (int k = 0; k < 24; ++k) put(TAN_K + k, i, K[k]);
    newton_euler_wrench(rb, K, w);  // − f_ext below
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      D fe = D(A.fext ? A.fext[(long)(6 * i + k) * A.Lf.sk + layout_base(A.Lf, st)] : T(0));
#pragma unroll
      for (int j = 0; j < N; ++j) fe.d[j] = A.unit ? T(0) : tan_in(A.dfext, A.Ldf, 6 * M.nb, 6 * i + k, j);
      put(TAN_W + k, i, w[k] - fe);
    }
  }
  if (!mid(get, put)) return;
  for (int i = M.nb - 1; i >= 0; --i) {  // joint_wrenches_and_torques!: τ = Sᵀ w, w added to the parent's
    const int jt = M.tbl[4 * i + 1], voff = M.tbl[4 * i + 3], p = M.tbl[4 * i];
    const T* rbt = rbase + (long)i * RB_STRIDE;
    D w[6], K[12];
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = get(TAN_W + k, i);
#pragma unroll
    for (int k = 0; k < 12; ++k) K[k] = get(TAN_K + k, i);
    D out[6];
    joint_torque(jt, rbt, K, w, out);
    const int nvi = joint_nv(jt);
    for (int k = 0; k < nvi; ++k) {
      if (A.tau && chunk == 0) A.tau[(long)(voff + k) * A.Lv.sk + layout_base(A.Lv, st)] = out[k].v;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int e = e0 + j;
        if (e >= A.ntan) continue;
        T* o = A.out.at(A.g0 + e, voff + k, st);
        if (o) *o = A.sign * out[k].d[j] + (A.dadd ? A.dadd[((long)e * M.nv + voff + k) * A.Ldv.sk + layout_base(A.Ldv, st)] : T(0));
      }
    }
    if (p >= 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) put(TAN_W + k, p, get(TAN_W + k, p) + w[k]);
    }
  }
}

struct TanNoMid {
  template <typename G, typename P> RBD_HD bool operator()(G&, P&) const { return true; }
};
template <typename T, int N>
RBD_HD void tangent_rnea_state(const BigModel& M, const TanArgs<T>& A, long st, int chunk, T* sc, long ld, long slot) {
  tangent_rnea_sweeps<T, N>(M, A, st, chunk, sc, ld, slot, TanNoMid());
}

// x = M⁻¹ rhs for one right-hand side of one state against its Cholesky factor (lower triangle of L, column-major per state, layout Ll): the rhs of
// column c is rhs[(c nv + r) B + st] (identity: e_c, rhs unused); x goes to out.at(c, r, st).  NVP > 0: loops bounded by NVP >= nv at compile time,
// so that x can live in registers; NVP == 0: x is memory of nv values
template <int NVP, typename T, typename X>
RBD_HD void tri_solve_col(int nv, const T* L, Layout Ll, long st, int c, const T* rhs, long B, int identity, const ColOut<T>& out, X& x) {
  auto Lr = [&](int r, int k) -> T { return L[((long)k * nv + r) * Ll.sk + layout_base(Ll, st)]; };
  const int n = NVP > 0 ? NVP : nv;
#pragma unroll
  for (int i = 0; i < n; ++i) {  // L y = rhs
    if (i < nv) {
      T s = identity ? (i == c ? T(1) : T(0)) : rhs[((long)c * nv + i) * B + st];
#pragma unroll
      for (int k = 0; k < i; ++k) s -= Lr(i, k) * x[k];
      x[i] = s / Lr(i, i);
    }
  }
#pragma unroll
  for (int i = n - 1; i >= 0; --i) {  // Lᵀ x = y
    if (i < nv) {
      T s = x[i];
#pragma unroll
      for (int k = i + 1; k < n; ++k)
        if (k < nv) s -= Lr(k, i) * x[k];
      x[i] = s / Lr(i, i);
    }
  }
#pragma unroll
  for (int i = 0; i < n; ++i)
    if (i < nv)
      if (T* o = out.at(c, i, st)) *o = x[i];
}

}  // namespace rbd
