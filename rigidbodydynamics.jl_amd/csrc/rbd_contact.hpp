// rbd_contact.hpp — the soft contact model of one (contact point, half-space) pair and its hand-written pullback (rbd_contact_dynamics_vjp,
// rbd_dynamics_contact_vjp), and the friction state's Runge–Kutta tableau with its pullback (rbd_simulate_contact_vjp).  The model is the reference's default (src/contact.jl: HuntCrossleyModel :98-119, ViscoelasticCoulombModel :122-178,
// HalfSpace3D :202-228) with the arithmetic of contact_kernel (rbd_contact_kernels.hip), which stays the forward path:
//   sep = (pos − h)·n;  outside (sep > 0): f = 0, ẋ = 0, the friction state x is reset to 0
//   z = −sep, ż = −vel·n, fn = max(0, λ zⁿ ż + k zⁿ)                       Hunt–Crossley
//   v_t = vel + ż n, f_s⁰ = −k_s x − b v_t, f_s = f_s⁰ · min(1, μ fn / ‖f_s⁰‖)    viscoelastic Coulomb: stick, or slip on the cone
//   ẋ = (−k_s x − f_s) / b,  f = fn n + f_s,  the body's wrench += (pos × f; f)
// contact_pair_force<S> is templated on the scalar, like point_kin_state<S>: tests/test_contact_vjp_cpu.py takes J·d from its Dual<double, 1> instantiation
// and checks contact_pair_adjoint<double> against it.  contact_pair_adjoint is the derivative of the branch the forward pass takes:
//   outside            every cotangent is zero (x_out = 0 and ẋ = 0 whatever the inputs);
//   clamped (fn ≤ 0)   the normal force and the slip scale contribute nothing;
//   sticking           f_s = f_s⁰;
//   slipping           f_s = f_s⁰ · (μ fn / ‖f_s⁰‖) differentiated in THAT form — sqrt(m2 / n2) has an infinite derivative in m2 at fn = 0;
//   zⁿ                 n zⁿ⁻¹, which pow gives the one-sided limit of at z = 0 for n ≥ 1 (0, or 1 when n = 1); n < 1 at z = 0 is not finite.
// On a branch boundary (sep = 0, fn = 0, ‖f_s⁰‖ = μ fn) the model is not differentiable; the pullback is then that of the branch taken.
#pragma once
#include "rbd_point.hpp"

namespace rbd {

RBD_HD double ct_val(double x) { return x; }
RBD_HD float ct_val(float x) { return x; }
template <typename T, int N> RBD_HD T ct_val(const Dual<T, N>& x) { return x.v; }
RBD_HD double ct_pow(double x, double n) { return pow(x, n); }
RBD_HD float ct_pow(float x, float n) { return powf(x, n); }
RBD_HD double ct_sqrt(double x) { return sqrt(x); }
RBD_HD float ct_sqrt(float x) { return sqrtf(x); }
RBD_HD double ct_div(double a, double b) { return a / b; }
RBD_HD float ct_div(float a, float b) { return a / b; }
template <typename T, int N> RBD_HD Dual<T, N> ct_pow(const Dual<T, N>& x, T n) {
  Dual<T, N> r;
  r.v = ct_pow(x.v, n);
  const T g = n * ct_pow(x.v, n - T(1));
#pragma unroll
  for (int j = 0; j < N; ++j) r.d[j] = g * x.d[j];
  return r;
}
// (at x = 0 the tangent is taken as zero: the one place the model forms sqrt(0) is the slip scale of a clamped pair, whose force is identically zero nearby)
template <typename T, int N> RBD_HD Dual<T, N> ct_sqrt(const Dual<T, N>& x) {
  Dual<T, N> r;
  r.v = ct_sqrt(x.v);
  const T g = x.v > T(0) ? T(0.5) / r.v : T(0);
#pragma unroll
  for (int j = 0; j < N; ++j) r.d[j] = g * x.d[j];
  return r;
}
template <typename T, int N> RBD_HD Dual<T, N> ct_div(const Dual<T, N>& a, const Dual<T, N>& b) {
  Dual<T, N> r;
  const T ib = T(1) / b.v;
  r.v = a.v * ib;
#pragma unroll
  for (int j = 0; j < N; ++j) r.d[j] = (a.d[j] - r.v * b.d[j]) * ib;
  return r;
}

// One pair.  pos, vel: the contact point in the root frame; x: its friction state for this half-space; c: the point's CP_STRIDE parameters; H: the half-space
// (point, unit outward normal).  Returns whether the point is inside; f (3) and xd = ẋ (3) are always written (zero outside, where the caller resets x).
template <typename S> RBD_HD bool contact_pair_force(const S* pos, const S* vel, const S* x, const typename ScalarOf<S>::type* c,
                                                     const typename ScalarOf<S>::type* H, S* f, S* xd) {
  using T = typename ScalarOf<S>::type;
  const T* n = H + 3;
  const S sep = (pos[0] - H[0]) * n[0] + (pos[1] - H[1]) * n[1] + (pos[2] - H[2]) * n[2];  // separation (contact.jl:224)
  if (!(ct_val(sep) <= T(0))) {  // reset! the state, zero! the derivative (mechanism_algorithms.jl:714-715)
#pragma unroll
    for (int j = 0; j < 3; ++j) { f[j] = S(T(0)); xd[j] = S(T(0)); }
    return false;
  }
  const S z = -sep;
  const S zd = -(vel[0] * n[0] + vel[1] * n[1] + vel[2] * n[2]);
  const S zn = ct_pow(z, c[CP_HCN]);
  S fn = c[CP_HCL] * zn * zd + c[CP_HCK] * zn;  // HuntCrossley normal_force (:115-118)
  if (!(ct_val(fn) > T(0))) fn = S(T(0));
  S fs[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) fs[j] = (-c[CP_K]) * x[j] - c[CP_B] * (vel[j] + zd * n[j]);  // friction_force (:150-169): the stick force
  const S n2 = fs[0] * fs[0] + fs[1] * fs[1] + fs[2] * fs[2], m2 = (c[CP_MU] * fn) * (c[CP_MU] * fn);
  if (ct_val(n2) > ct_val(m2)) {  // clipped to the friction cone
    const S sc = ct_sqrt(ct_div(m2, n2));
#pragma unroll
    for (int j = 0; j < 3; ++j) fs[j] = fs[j] * sc;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    xd[j] = ((-c[CP_K]) * x[j] - fs[j]) / c[CP_B];  // dynamics! of the friction state (:171-178)
    f[j] = fn * n[j] + fs[j];
  }
  return true;
}

// The forward path's pair, statement for statement what contact_kernel has always computed (contact_pair_force above is the same model with the slip scale and
// the wrench formed in the order the derivative passes want): shared by contact_kernel and contact_sim_kernel (rbd_contact_sim_kernels.hip).  pt, vel: the
// contact point in the root frame; x: the pair's friction state; c, H as above.  Returns whether the point is inside; xd = ẋ (3) is always written (zero
// outside, where the caller resets x), and the pair's wrench (pt × f; f) is ADDED to w (6) when inside.
template <typename T> RBD_HD bool contact_pair_wrench(const T* pt, const T* vel, const T* x, const T* c, const T* H, T* xd, T* w) {
  const T* n = H + 3;
  const T sep = (pt[0] - H[0]) * n[0] + (pt[1] - H[1]) * n[1] + (pt[2] - H[2]) * n[2];  // separation (contact.jl:224)
  if (!(sep <= T(0))) {  // not point_inside (:225): reset! the state, zero! the derivative (mechanism_algorithms.jl:714-715)
#pragma unroll
    for (int j = 0; j < 3; ++j) xd[j] = T(0);
    return false;
  }
  // contact_dynamics! (contact.jl:79-93)
  const T z = -sep;
  const T zd = -(vel[0] * n[0] + vel[1] * n[1] + vel[2] * n[2]);
  const T zn = ct_pow(z, c[CP_HCN]);
  T fn = c[CP_HCL] * zn * zd + c[CP_HCK] * zn;  // HuntCrossley normal_force (:115-118)
  fn = fn > T(0) ? fn : T(0);
  T vt[3], fs[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) vt[j] = vel[j] + zd * n[j];
  // friction_force (:150-169): stick force −k x − b v, clipped to the friction cone
#pragma unroll
  for (int j = 0; j < 3; ++j) fs[j] = -c[CP_K] * x[j] - c[CP_B] * vt[j];
  const T n2 = fs[0] * fs[0] + fs[1] * fs[1] + fs[2] * fs[2], m2 = (c[CP_MU] * fn) * (c[CP_MU] * fn);
  if (n2 > m2) {
    const T sc = ct_sqrt(m2 / n2);
#pragma unroll
    for (int j = 0; j < 3; ++j) fs[j] *= sc;
  }
  // dynamics! of the friction state (:171-178): ẋ = (−k x − f_tangential) / b
#pragma unroll
  for (int j = 0; j < 3; ++j) xd[j] = (-c[CP_K] * x[j] - fs[j]) / c[CP_B];
  T f[3], tq[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) f[j] = fn * n[j] + fs[j];
  cross3(pt, f, tq);  // Wrench(point, force) (:712)
#pragma unroll
  for (int j = 0; j < 3; ++j) { w[j] += tq[j]; w[3 + j] += f[j]; }
  return true;
}

// The point of contact_kernel's walk: point = body_to_root * location; velocity = point_velocity(twist, point) = ω × point + v (mechanism_algorithms.jl:697-699),
// from the body's exported kinematics k (R 9, p 3, twist 6) and the point's constants c.
template <typename T> RBD_HD void contact_point_in_root(const T* k, const T* c, T* pt, T* vel) {
  T t3[3];
  matvec3(k, c + CP_LOC, pt);
#pragma unroll
  for (int j = 0; j < 3; ++j) pt[j] += k[9 + j];
  cross3(k + 12, pt, t3);
#pragma unroll
  for (int j = 0; j < 3; ++j) vel[j] = t3[j] + k[15 + j];
}

// One contact point against every half-space, from its body's kinematics: the contact step of forward mode (rbd_contact_dynamics_jvp, rbd_dynamics_contact_jvp:
// S = Dual<T, N> between the two sweeps of the tangent RNEA pass, rbd_tangent.hpp) and, with S = T, contact_kernel's arithmetic for one point.
//   K    the body's (R 9 row-major, p 3, twist 6 = (ω; v)) in the root frame, as tangent_rnea_state and the per-body kinematics export keep them
//   c    the point's CP_STRIDE constants;  hs: the nh half-spaces, 6 values each
//   xin(h, x)                    loads the pair's friction state (3 values of S: value and tangents) — wherever the caller keeps it
//   xout(h, inside, xd, xo)      receives ẋ and the state after the reset (xo = x inside, 0 outside, tangents included) of the pair
//   w    the point's wrench (pos × f; f) summed over the half-spaces, OVERWRITTEN (zero when every pair is outside)
// Nothing here knows a buffer layout: the stage-wise passes of simulate can call it per stage state, and tests/test_contact_jvp_cpu.py builds it as plain C++.
template <typename S, typename XIn, typename XOut>
RBD_HD void contact_point_step(const S* K, const typename ScalarOf<S>::type* c, const typename ScalarOf<S>::type* hs, int nh, XIn xin, XOut xout, S* w) {
  using T = typename ScalarOf<S>::type;
  S loc[3], pos[3], vel[3], t3[3], fsum[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) { loc[j] = S(c[CP_LOC + j]); fsum[j] = S(T(0)); }
  matvec3(K, loc, pos);  // point = body_to_root * location; velocity = ω × point + v (mechanism_algorithms.jl:697-699)
#pragma unroll
  for (int j = 0; j < 3; ++j) pos[j] += K[9 + j];
  cross3(K + 12, pos, t3);
#pragma unroll
  for (int j = 0; j < 3; ++j) vel[j] = t3[j] + K[15 + j];
  for (int h = 0; h < nh; ++h) {
    S x[3], f[3], xd[3], xo[3];
    xin(h, x);
    const bool inside = contact_pair_force<S>(pos, vel, x, c, hs + (long)h * 6, f, xd);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      xo[j] = inside ? x[j] : S(T(0));
      fsum[j] += f[j];
    }
    xout(h, inside, xd, xo);
  }
  cross3(pos, fsum, w);  // Wrench(point, force) (:712), the sum over the half-spaces: pos × is linear in f
#pragma unroll
  for (int j = 0; j < 3; ++j) w[3 + j] = fsum[j];
}

// ---- forward mode: the contact variant of the tangent RNEA pass (rbd_tangent.hpp tangent_rnea_sweeps) -----------------------------------------------------------
// What the variant needs beside TanArgs.  The friction state's tangents follow the rules of TanArgs' (direction e of a state at rows e·ns …, nullable = zero);
// with A.unit the directions g ≥ gs0 are the unit vectors of s (gs0 = nq + nv: the third block of the columns of (q; v; s)).  The tangent outputs go by column
// A.g0 + e like A.out (every buffer nullable): dcw rows of 6 nb (every body's, zero where no point sits), dsdot and dsout rows of ns.
template <typename T> struct TanContactArgs {
  ContactModel C;
  const T *s, *ds;
  Layout Ls, Lds;
  int gs0;
  ColOut<T> dcw, dsdot, dsout;
  int forward_only;  // 1: return after the contact step (rbd_contact_dynamics_jvp: no wrench sweep for nothing)
};

// tangent_rnea_state with contact: after the forward sweep stored every body's Dual K, the thread walks the contact points in the order of the additional state,
// calls contact_point_step<Dual<T, N>> on the point's body and SUBTRACTS THE TANGENT PART of the point's wrench from the body's TAN_W (the sign of fext there).
// The value part is not touched: the caller hands the pass the TOTAL wrenches (fext + contact, contact_kernel's) as A.fext, the wrenches v̇ was solved at, so
// the contact value is in TAN_W once already.  The wrench sweep and the right-hand sides then see d(total wrench) = dfext + d(contact wrench).
template <typename T, int N>
RBD_HD void tangent_contact_state(const BigModel& M, const TanArgs<T>& A, const TanContactArgs<T>& C, long st, int chunk, T* sc, long ld, long slot) {
  using D = Dual<T, N>;
  const int e0 = chunk * N;
  const int np = C.C.np, nh = C.C.nh, ns = 3 * np * nh;
  const T* cp = reinterpret_cast<const T*>(C.C.cp);
  const T* hs = reinterpret_cast<const T*>(C.C.hs);
  tangent_rnea_sweeps<T, N>(M, A, st, chunk, sc, ld, slot, [&](auto& get, auto& put) -> bool {
    const bool want_cw = C.dcw.a || C.dcw.b;
    if (want_cw)
      for (int r = 0; r < 6 * M.nb; ++r)
#pragma unroll
        for (int j = 0; j < N; ++j)
          if (e0 + j < A.ntan)
            if (T* o = C.dcw.at(A.g0 + e0 + j, r, st)) *o = T(0);
    for (int ip = 0; ip < np; ++ip) {
      const int body = C.C.cbody[ip];
      D K[18], w[6];
#pragma unroll
      for (int k = 0; k < 18; ++k) K[k] = get(TAN_K + k, body);
      contact_point_step<D>(
          K, cp + (long)ip * CP_STRIDE, hs, nh,
          [&](int h, D* x) {
            const int so = (ip * nh + h) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              x[k].v = C.s[(long)(so + k) * C.Ls.sk + layout_base(C.Ls, st)];
#pragma unroll
              for (int j = 0; j < N; ++j) {
                const int e = e0 + j;
                T d = T(0);
                if (e < A.ntan) {
                  if (A.unit) d = A.g0 + e == C.gs0 + so + k ? T(1) : T(0);
                  else if (C.ds) d = C.ds[((long)e * ns + so + k) * C.Lds.sk + layout_base(C.Lds, st)];
                }
                x[k].d[j] = d;
              }
            }
          },
          [&](int h, bool, const D* xd, const D* xo) {
            const int so = (ip * nh + h) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
              for (int j = 0; j < N; ++j) {
                const int e = e0 + j;
                if (e >= A.ntan) continue;
                if (T* o = C.dsdot.at(A.g0 + e, so + k, st)) *o = xd[k].d[j];
                if (T* o = C.dsout.at(A.g0 + e, so + k, st)) *o = xo[k].d[j];
              }
          },
          w);
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        D x = get(TAN_W + k, body);
#pragma unroll
        for (int j = 0; j < N; ++j) {
          x.d[j] -= w[k].d[j];
          if (want_cw && e0 + j < A.ntan)
            if (T* o = C.dcw.at(A.g0 + e0 + j, 6 * body + k, st)) *o += w[k].d[j];
        }
        put(TAN_W + k, body, x);
      }
    }
    return !C.forward_only;
  });
}

// The pullback of one pair.  fb, tqb: the cotangent (τ̄q; f̄) of the body's wrench (pos × f; f) (each nullable: zero); xdb: that of ẋ; xob: that of the friction
// state after the reset (each nullable).  pos_bar, vel_bar, x_bar (3 each) are OVERWRITTEN.  Returns whether the point is inside.
template <typename T> RBD_HD bool contact_pair_adjoint(const T* pos, const T* vel, const T* x, const T* c, const T* H, const T* fb, const T* tqb, const T* xdb,
                                                       const T* xob, T* pos_bar, T* vel_bar, T* x_bar) {
  const T* n = H + 3;
#pragma unroll
  for (int j = 0; j < 3; ++j) { pos_bar[j] = T(0); vel_bar[j] = T(0); x_bar[j] = T(0); }
  const T sep = (pos[0] - H[0]) * n[0] + (pos[1] - H[1]) * n[1] + (pos[2] - H[2]) * n[2];
  if (!(sep <= T(0))) return false;
  // the forward values of the branch
  const T z = -sep, zd = -(vel[0] * n[0] + vel[1] * n[1] + vel[2] * n[2]);
  const T zn = ct_pow(z, c[CP_HCN]);
  const T fr = c[CP_HCL] * zn * zd + c[CP_HCK] * zn;
  const bool pushing = fr > T(0);
  const T fn = pushing ? fr : T(0);
  T f0[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) f0[j] = -c[CP_K] * x[j] - c[CP_B] * (vel[j] + zd * n[j]);
  const T n2 = f0[0] * f0[0] + f0[1] * f0[1] + f0[2] * f0[2], mf = c[CP_MU] * fn;
  const bool slip = n2 > mf * mf;
  const T in0 = slip ? T(1) / ct_sqrt(n2) : T(0);  // (n2 > m2 ≥ 0)
  const T sc = slip ? mf * in0 : T(1);
  // f = fn n + f_s, the wrench (pos × f; f): f̄ += τ̄q × pos, pos_bar = f × τ̄q
  T fbar[3] = {fb ? fb[0] : T(0), fb ? fb[1] : T(0), fb ? fb[2] : T(0)};
  if (tqb) {
    T f[3], t3[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) f[j] = fn * n[j] + sc * f0[j];
    cross3(tqb, pos, t3);
#pragma unroll
    for (int j = 0; j < 3; ++j) fbar[j] += t3[j];
    cross3(f, tqb, pos_bar);
  }
  T fnb = fbar[0] * n[0] + fbar[1] * n[1] + fbar[2] * n[2];
  // ẋ = (−k_s x − f_s) / b
  T fsb[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const T g = xdb ? xdb[j] / c[CP_B] : T(0);
    fsb[j] = fbar[j] - g;
    x_bar[j] = -c[CP_K] * g + (xob ? xob[j] : T(0));
  }
  // f_s = sc f_s⁰ with sc = μ fn / ‖f_s⁰‖ when slipping: f̄_s⁰ = sc (f̄_s − u (u·f̄_s)), f̄n += μ (u·f̄_s), u = f_s⁰ / ‖f_s⁰‖
  if (slip) {
    const T ub = (f0[0] * fsb[0] + f0[1] * fsb[1] + f0[2] * fsb[2]) * in0;
    fnb += c[CP_MU] * ub;
#pragma unroll
    for (int j = 0; j < 3; ++j) fsb[j] = sc * (fsb[j] - f0[j] * in0 * ub);
  }
  // f_s⁰ = −k_s x − b v_t, v_t = vel + ż n
  T zdb = T(0);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    x_bar[j] -= c[CP_K] * fsb[j];
    vel_bar[j] = -c[CP_B] * fsb[j];
    zdb += vel_bar[j] * n[j];
  }
  // fn = max(0, zⁿ (λ ż + k)), zⁿ pulled back with n zⁿ⁻¹
  T zb = T(0);
  if (pushing) {
    zdb += fnb * c[CP_HCL] * zn;
    zb = fnb * (c[CP_HCL] * zd + c[CP_HCK]) * c[CP_HCN] * ct_pow(z, c[CP_HCN] - T(1));
  }
  // ż = −vel·n, z = −(pos − h)·n
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    vel_bar[j] -= zdb * n[j];
    pos_bar[j] -= zb * n[j];
  }
  return true;
}

// ---- the friction state through the Runge–Kutta tableau (rbd_simulate_contact_vjp) ---------------------------------------------------------------------------
// contact_sim_kernel's map of s (runge_kutta_4, ode_integrators.jl:48-55) in its value form, stage k = 0 … 3 like mk_stage_value_joint: from the step's start s0
// and ṡ_k at stage state k, the next stage state s_{k+1} = s0 + dt a_k ṡ_k and the running sum acc = Σ_{j ≤ k} dt b_j ṡ_j (stages 0-2; acc is not read at stage
// 0), or at stage 3 the state after the step s⁺ = s0 + acc + dt b_3 ṡ_3.  The stage states stay apart from s0: the reset of an outside pair's state happens in
// the stage state only.  Templated on the scalar: tests/test_simulate_contact_vjp_cpu.py takes J·d from the Dual<double, 1> instantiation.
template <typename T> RBD_HD T contact_tableau_a(int stage) { return stage == 2 ? T(1) : T(0.5); }
template <typename T> RBD_HD T contact_tableau_b(int stage) { return stage == 0 || stage == 3 ? T(1) / T(6) : T(1) / T(3); }

template <typename S> RBD_HD void contact_stage_value(int stage, typename ScalarOf<S>::type dt, const S& s0, const S& sd, S& acc, S& sn) {
  using T = typename ScalarOf<S>::type;
  const T wb = dt * contact_tableau_b<T>(stage), wa = dt * contact_tableau_a<T>(stage);
  const S sum = stage == 0 ? wb * sd : acc + wb * sd;
  if (stage < 3) {
    acc = sum;
    sn = s0 + wa * sd;
  } else {
    sn = s0 + sum;
  }
}

// Its pullback, stages 3 … 0.  snb: the cotangent of the stage's output (stage 3: of s⁺).  s0b: the cotangent of s0 collected over the stages done so far
// (written at 3, added to at 2 … 0); accb: in, the cotangent of the sum out (stages 0-2; ignored at 3), out, that of the sum in (zero at stage 0, which does
// not read it).  sdb = ṡ̄_k is written.
template <typename T> RBD_HD void contact_stage_adjoint(int stage, T dt, T snb, T& s0b, T& accb, T& sdb) {
  const T wb = dt * contact_tableau_b<T>(stage), wa = dt * contact_tableau_a<T>(stage);
  if (stage == 3) {
    s0b = snb; accb = snb;
    sdb = wb * snb;
  } else {
    sdb = wa * snb + wb * accb;
    s0b += snb;
    if (stage == 0) accb = T(0);
  }
}

// one launch of tangent_contact_stage_kernel (rbd_tangent_kernels.hip; rbd_simulate_contact_jvp, rbd_simulate_contact_step_derivatives): contact_stage_value on
// Dual<T, N>, the friction state's share of what MkTanArgs is for (q, v).  Values (the call's layout Ls; sn may be s0 itself at stage 3) are written by chunk 0;
// tangents are ColOut views (direction e of the pass at column e, rows of the ns values of s), each thread reads and writes only its own.
template <typename T> struct CtTanStageArgs {
  long B;
  int ntan, ns, stage;  // directions of the pass, values of s per state, stage 0..3
  T dt;
  const T *s0, *sd;  // the step's start, ṡ at the stage state just evaluated
  T* acc;            // Σ dt b_j ṡ_j (read at stages 1-3, written at 0-2)
  T* sn;             // the next stage state (stage 3: the state after the step)
  Layout Ls;
  ColOut<T> ds0, dsd, dacc;
  ColOut<T> os;      // tangent of sn at rows orow + …, direction e at column ocol + e
  int ocol, orow;
};

}  // namespace rbd
