// rbd_tangent_mk.hpp — forward-mode derivative of one stage of the Munthe-Kaas RK4 step (MuntheKaasIntegrator.step, src/ode_integrators.jl:233-299;
// runge_kutta_4, :48-55): the Dual<T, N> counterpart of mk_stage_lane (rbd_integrator.hpp) for one joint.  Three pieces per joint:
//  - tan_joint_local_rate: ϕ̇ of local_coordinates! at the stage state just evaluated, from (q0, q_i, v_i) and their tangents;
//  - the tableau: the next stage state needs only this stage's rates (a_{i+1,i}), the closing combination needs the running sums Σ dt b_j (ϕ̇_j, v̇_j);
//  - tan_joint_global: global_coordinates!, the next stage state and its tangent.
// The values are those of rbd_integrator.hpp up to rounding.  The derivatives are those of the SMOOTH map: the small-angle branches of the reference
// (θ < eps in rotvec / exp / log_with_time_derivative, the Bortz series) are removable singularities, and a literal Dual pass through them would give
// 0/0 at |ϕ_rot| = 0 and drop the first-order terms ½ ϕ_rot × ϕ_trans (exp) and ½ ad_X v (log) exactly where rollouts start (a floating base at rest,
// or with ω = 0).  Every coefficient that is singular at θ = 0 is therefore written as a power series in θ² below a threshold (the Bortz equation's own:
// 1e-2 in fp64, 0.5 in fp32) and in closed form above it, so that its derivative is carried through θ² = ϕ·ϕ, which is smooth.
// Host+device: tests/test_simulate_derivatives_cpu.py compiles this header as plain C++ and checks it against a central difference of the oracle.
#pragma once
#include "rbd_tangent.hpp"

namespace rbd {

template <typename T, int N> RBD_HD Dual<T, N> operator/(const Dual<T, N>& a, const Dual<T, N>& b) {
  Dual<T, N> r;
  const T ib = T(1) / b.v;
  r.v = a.v * ib;
#pragma unroll
  for (int j = 0; j < N; ++j) r.d[j] = (a.d[j] - r.v * b.d[j]) * ib;
  return r;
}
template <typename T, int N> RBD_HD Dual<T, N> operator/(T a, const Dual<T, N>& b) { return Dual<T, N>(a) / b; }
template <typename T, int N> RBD_HD Dual<T, N> dsqrt(const Dual<T, N>& x) {  // (x.v > 0)
  Dual<T, N> r;
  r.v = sqrt(x.v);
  const T h = T(0.5) / r.v;
#pragma unroll
  for (int j = 0; j < N; ++j) r.d[j] = h * x.d[j];
  return r;
}
template <typename T, int N> RBD_HD Dual<T, N> datan2(const Dual<T, N>& y, const Dual<T, N>& x) {  // (x, y) != (0, 0)
  Dual<T, N> r;
  r.v = atan2(y.v, x.v);
  const T id = T(1) / (x.v * x.v + y.v * y.v);
#pragma unroll
  for (int j = 0; j < N; ++j) r.d[j] = (x.v * y.d[j] - y.v * x.d[j]) * id;
  return r;
}
// c0 + c1 t + … + c5 t⁵ (Horner)
template <typename T, int N>
RBD_HD Dual<T, N> series6(const Dual<T, N>& t, double c0, double c1, double c2, double c3, double c4, double c5) {
  Dual<T, N> r = t * T(c5) + T(c4);
  r = r * t + T(c3);
  r = r * t + T(c2);
  r = r * t + T(c1);
  return r * t + T(c0);
}
template <typename T, int N> RBD_HD Dual<T, N> dot3d(const Dual<T, N>* a, const Dual<T, N>* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// θ below which the θ²-series replace the closed forms (rbd_integrator.hpp's Bortz threshold)
template <typename T> RBD_HD T mk_series_theta() { return sizeof(T) == 4 ? T(0.5) : T(1e-2); }

// Taylor coefficients in t = θ² (x = θ/2): α = x cot x, β = x²/sin²x
// (1 − α)/θ²: the Bortz coefficient of rotation_vector_rate and the (1 − α)/θ² of log_with_time_derivative's q_v
#define RBD_MK_CA 1.0 / 12, 1.0 / 720, 1.0 / 30240, 1.0 / 1209600, 1.0 / 47900160, 691.0 / 1307674368000
// (2(1 − α) + (α − β)/2)/θ² and ((1 − α) + (α − β)/2)/θ⁴ of log_with_time_derivative
#define RBD_MK_A 1.0 / 12, 0.0, -1.0 / 30240, -1.0 / 604800, -1.0 / 15966720, -691.0 / 326918592000
#define RBD_MK_BC -1.0 / 720, -1.0 / 15120, -1.0 / 403200, -1.0 / 11975040, -691.0 / 261534873600, -1.0 / 12454041600
// exp on SE(3): (1 − cos θ)/θ², (θ − sin θ)/θ³; quaternion of a rotation vector: cos(θ/2), sin(θ/2)/θ
#define RBD_MK_EA 1.0 / 2, -1.0 / 24, 1.0 / 720, -1.0 / 40320, 1.0 / 3628800, -1.0 / 479001600
#define RBD_MK_EB 1.0 / 6, -1.0 / 120, 1.0 / 5040, -1.0 / 362880, 1.0 / 39916800, -1.0 / 6227020800
#define RBD_MK_QC 1.0, -1.0 / 8, 1.0 / 384, -1.0 / 46080, 1.0 / 10321920, -1.0 / 3715891200
#define RBD_MK_QS 1.0 / 2, -1.0 / 48, 1.0 / 3840, -1.0 / 645120, 1.0 / 185794560, -1.0 / 81749606400
// atan(√z)/√z: the rotation vector of a quaternion (w, u) is (2/w) atan(√z)/√z · u with z = |u|²/w²
#define RBD_MK_AT 1.0, -1.0 / 3, 1.0 / 5, -1.0 / 7, 1.0 / 9, -1.0 / 11

template <typename T, int N> RBD_HD void dquat_mul(const Dual<T, N>* a, const Dual<T, N>* b, Dual<T, N>* o) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
template <typename T, int N> RBD_HD void dquat_rotate(const Dual<T, N>* q, const Dual<T, N>* x, Dual<T, N>* o) {  // R(q) x, the unnormalised formula
  Dual<T, N> R[9];
  rot_quat(q[0], q[1], q[2], q[3], R);
  matvec3(R, x, o);
}

// RotationVec(quat): θ/|u| · u for the quaternion (w, u), θ = 2 atan2(|u|, w)
template <typename T, int N> RBD_HD void tan_rotvec_from_quat(const Dual<T, N>* q, Dual<T, N>* r) {
  using D = Dual<T, N>;
  const D u2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const T lim = mk_series_theta<T>() / 2;
  D k;
  if (q[0].v > T(0) && u2.v < lim * lim * q[0].v * q[0].v) {
    const D iw = T(1) / q[0];
    k = T(2) * iw * series6<T, N>(u2 * iw * iw, RBD_MK_AT);
  } else if (u2.v > T(0)) {
    const D s = dsqrt(u2);
    k = T(2) * datan2(s, q[0]) / s;
  } else {
    k = D(T(2));  // (w <= 0 and u = 0: a rotation by 2π, outside any step)
  }
  r[0] = k * q[1]; r[1] = k * q[2]; r[2] = k * q[3];
}

// QuatRotation(RotationVec(r))
template <typename T, int N> RBD_HD void tan_quat_from_rotvec(const Dual<T, N>* r, Dual<T, N>* q) {
  using D = Dual<T, N>;
  const D t2 = dot3d(r, r);
  const T lim = mk_series_theta<T>();
  D c, k;
  if (t2.v < lim * lim) {
    c = series6<T, N>(t2, RBD_MK_QC);
    k = series6<T, N>(t2, RBD_MK_QS);
  } else {
    const D th = dsqrt(t2);
    D s;
    sincos_t(T(0.5) * th, &s, &c);
    k = s / th;
  }
  q[0] = c; q[1] = k * r[0]; q[2] = k * r[1]; q[3] = k * r[2];
}

// ϕ̇ of local_coordinates! for one joint (rbd_integrator.hpp joint_local_rate), with tangents
template <typename T, int N> RBD_HD void tan_joint_local_rate(int t, const Dual<T, N>* q0, const Dual<T, N>* q, const Dual<T, N>* v, Dual<T, N>* o) {
  using D = Dual<T, N>;
  const T lim = mk_series_theta<T>();
#pragma unroll
  for (int k = 0; k < 6; ++k) o[k] = D(T(0));
  if (t == RBD_JOINT_REVOLUTE || t == RBD_JOINT_PRISMATIC || t == RBD_JOINT_SINCOS_REVOLUTE) {
    o[0] = v[0];
  } else if (t == RBD_JOINT_PLANAR) {
    D s, c;
    sincos_t(q[2], &s, &c);
    o[0] = c * v[0] - s * v[1]; o[1] = s * v[0] + c * v[1]; o[2] = v[2];
  } else if (t == RBD_JOINT_QUAT_SPHERICAL) {  // rotation_vector_rate (Bortz equation, spatial/util.jl:88-102)
    const D q0c[4] = {q0[0], -q0[1], -q0[2], -q0[3]};
    D dq[4], phi[3], c1[3], c2[3];
    dquat_mul(q0c, q, dq);
    tan_rotvec_from_quat(dq, phi);
    cross3(phi, v, c1);
    const D t2 = dot3d(phi, phi);
    D f;
    if (t2.v < lim * lim) {
      f = series6<T, N>(t2, RBD_MK_CA);
    } else {
      const D th = dsqrt(t2);
      D s, c;
      sincos_t(th, &s, &c);
      f = (T(1) - (th * s) / (T(2) * (T(1) - c))) / t2;
    }
    cross3(phi, c1, c2);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = v[k] + T(0.5) * c1[k] + f * c2[k];
  } else if (t == RBD_JOINT_QUAT_FLOATING) {  // log_with_time_derivative of inv(T0) T with the body twist (spatialmotion.jl:226-304)
    const D q0c[4] = {q0[0], -q0[1], -q0[2], -q0[3]};
    D dq[4], d[3], dp[3], psi[3];
    dquat_mul(q0c, q, dq);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = q[4 + k] - q0[4 + k];
    dquat_rotate(q0c, d, dp);
    tan_rotvec_from_quat(dq, psi);
    const D t2 = dot3d(psi, psi);
    D ca, A, Bc;
    if (t2.v < lim * lim) {
      ca = series6<T, N>(t2, RBD_MK_CA);
      A = series6<T, N>(t2, RBD_MK_A);
      Bc = series6<T, N>(t2, RBD_MK_BC);
    } else {
      const D th = dsqrt(t2), h = T(0.5) * th;
      D s2, c2;
      sincos_t(h, &s2, &c2);
      const D alpha = h * c2 / s2, beta = h * h / (s2 * s2), ith2 = T(1) / t2;
      ca = (T(1) - alpha) * ith2;
      A = (T(2) * (T(1) - alpha) + T(0.5) * (alpha - beta)) * ith2;
      Bc = ((T(1) - alpha) + T(0.5) * (alpha - beta)) * ith2 * ith2;
    }
    D x1[3], x2[3], X[6], a1[6], a2[6], a3[6], a4[6];
    cross3(psi, dp, x1);
    cross3(psi, x1, x2);
#pragma unroll
    for (int k = 0; k < 3; ++k) { X[k] = psi[k]; X[3 + k] = dp[k] - T(0.5) * x1[k] + ca * x2[k]; }
    se3_comm(X, v, a1);
    se3_comm(X, a1, a2);
    se3_comm(X, a2, a3);
    se3_comm(X, a3, a4);
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = v[k] + T(0.5) * a1[k] + A * a2[k] + Bc * a4[k];
    // the value of the reference's branch (θ <= eps: the body twist itself, without ½ ad_X v — O(|q_v| |ω|), which is not small when only the rotation is),
    // the derivative of the smooth map: rbd_simulate's state, and the limit the reference's own derivative takes for every θ > 0
    const T eps = sizeof(T) == 4 ? T(1.1920929e-7) : T(2.220446049250313e-16);
    if (!(t2.v > eps * eps)) {
#pragma unroll
      for (int k = 0; k < 6; ++k) o[k].v = v[k].v;
    }
  }
}

// global_coordinates! for one joint (rbd_integrator.hpp joint_global), with tangents
template <typename T, int N> RBD_HD void tan_joint_global(int t, const Dual<T, N>* q0, const Dual<T, N>* phi, Dual<T, N>* q) {
  using D = Dual<T, N>;
#pragma unroll
  for (int k = 0; k < 7; ++k) q[k] = D(T(0));
  if (t == RBD_JOINT_REVOLUTE || t == RBD_JOINT_PRISMATIC) {
    q[0] = q0[0] + phi[0];
  } else if (t == RBD_JOINT_PLANAR) {
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = q0[k] + phi[k];
  } else if (t == RBD_JOINT_SINCOS_REVOLUTE) {
    D sd, cd;
    sincos_t(phi[0], &sd, &cd);
    q[0] = q0[0] * cd + q0[1] * sd;
    q[1] = q0[1] * cd - q0[0] * sd;
  } else if (t == RBD_JOINT_QUAT_SPHERICAL) {
    D dq[4];
    tan_quat_from_rotvec(phi, dq);
    dquat_mul(q0, dq, q);
  } else if (t == RBD_JOINT_QUAT_FLOATING) {  // exp(::Twist) (spatialmotion.jl:311-332): translation V ν = ν + a ω × ν + b ω × (ω × ν)
    D dq[4], c1[3], c2[3], tr[3], w[3];
    tan_quat_from_rotvec(phi, dq);
    const D t2 = dot3d(phi, phi);
    const T lim = mk_series_theta<T>();
    D a, b;
    if (t2.v < lim * lim) {
      a = series6<T, N>(t2, RBD_MK_EA);
      b = series6<T, N>(t2, RBD_MK_EB);
    } else {
      const D th = dsqrt(t2);
      D s, c;
      sincos_t(th, &s, &c);
      a = (T(1) - c) / t2;
      b = (th - s) / (t2 * th);
    }
    cross3(phi, phi + 3, c1);
    cross3(phi, c1, c2);
#pragma unroll
    for (int k = 0; k < 3; ++k) tr[k] = phi[3 + k] + a * c1[k] + b * c2[k];
    dquat_mul(q0, dq, q);
    dquat_rotate(q0, tr, w);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[4 + k] = q0[4 + k] + w[k];
  }
}

// Stage `stage` (0..3) of a step for one joint, after the dynamics at that stage's state: rate = ϕ̇ of the stage, then the tableau of runge_kutta_4 and
// global_coordinates!.  acc_p / acc_v: Σ_{j<stage} dt b_j ϕ̇_j and v0 + Σ_{j<stage} dt b_j v̇_j in (unused at stage 0), the sums through this stage out
// (stages 0-2).  qn, vn: the next stage's state (stage 3: the state after the step), summed in the order of mk_stage_lane.
template <typename T, int N>
RBD_HD void tan_mk_stage_joint(int jt, int stage, T dt, const Dual<T, N>* q0, const Dual<T, N>* v0, const Dual<T, N>* qs, const Dual<T, N>* vs,
                               const Dual<T, N>* vd, Dual<T, N>* acc_p, Dual<T, N>* acc_v, Dual<T, N>* qn, Dual<T, N>* vn) {
  using D = Dual<T, N>;
  const int nv = joint_nv(jt);
  D rate[6], phi[6];
  tan_joint_local_rate(jt, q0, qs, vs, rate);
  const T b = stage == 0 || stage == 3 ? T(1) / 6 : T(1) / 3;  // (ode_integrators.jl:48-55)
  const T wb = dt * b;
  const T wa = dt * (stage == 2 ? T(1) : T(0.5));
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    phi[k] = D(T(0)); vn[k] = D(T(0));
    if (k < nv) {
      const D sp = stage == 0 ? wb * rate[k] : acc_p[k] + wb * rate[k];
      const D sv = (stage == 0 ? v0[k] : acc_v[k]) + wb * vd[k];
      if (stage < 3) {
        acc_p[k] = sp; acc_v[k] = sv;
        phi[k] = wa * rate[k];
        vn[k] = v0[k] + wa * vd[k];
      } else {
        phi[k] = sp; vn[k] = sv;
      }
    }
  }
  tan_joint_global(jt, q0, phi, qn);
}

// one launch of tangent_mk_stage_kernel (rbd_tangent_kernels.hip).  Values (layouts Lq, Lv) are read by every chunk of directions and written by chunk 0;
// tangents are ColOut views (direction e of the pass at column e, rows of the joint's coordinates), each thread reads and writes only its own.
template <typename T> struct MkTanArgs {
  long B;
  int ntan, nb, stage;  // directions of the pass, bodies (BigModel tables), stage 0..3
  T dt;
  const int32_t* tbl;
  const T *q0, *v0, *qs, *vs, *vd;  // the step's base point, the stage state just evaluated, its v̇
  T *accp, *accv;                   // Σ dt b_j ϕ̇_j and v0 + Σ dt b_j v̇_j (read at stages 1-3, written at 0-2)
  T *qn, *vn;                       // the next stage state (stage 3: the state after the step)
  Layout Lq, Lv;
  ColOut<T> dq0, dv0, dqs, dvs, dvd, daccp, daccv;
  ColOut<T> oq, ov;                 // tangents of qn (rows of q) and vn (rows ovrow + … ), direction e at column ocol + e
  int ocol, ovrow;
};

}  // namespace rbd
