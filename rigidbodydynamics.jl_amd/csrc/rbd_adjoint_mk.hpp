// rbd_adjoint_mk.hpp — reverse-mode derivative of one stage of the Munthe-Kaas RK4 step (MuntheKaasIntegrator.step, src/ode_integrators.jl:233-299) for
// one joint: adj_mk_stage_joint is the exact transpose of tan_mk_stage_joint (rbd_tangent_mk.hpp), i.e. of the function rbd_simulate_jvp differentiates —
// the θ²-series below mk_series_theta and the value-of-the-branch convention of log's θ <= eps included, so ⟨ȳ, J d⟩ = ⟨Jᵀȳ, d⟩ holds at θ = 0 as well.
//  - the tableau (v0, v̇, the running sums: multiples of dt b_i and dt a_i) by hand;
//  - the two nonlinear maps, joint_local_rate in (q0, qs, vs) (at most 20 inputs) and joint_global in (q0, ϕ) (at most 13), by contracting forward passes
//    of tan_joint_local_rate / tan_joint_global over N input coordinates at a time with the output's cotangent: the series code is reused, not re-derived;
//  - the 1-coordinate joints (revolute, prismatic, SinCosRevolute) by hand, without Dual code (adjoint_mk_stage_kernel's narrow class, WIDE = false).
// The value stage map of the reverse-mode driver (mk_stage_value_joint) computes the values tan_mk_stage_joint does, so the stage states of
// rbd_simulate_vjp equal rbd_simulate_jvp's to rounding.
// Host+device: tests/test_simulate_vjp_cpu.py compiles this header as plain C++ and checks the dot-product identity against tan_mk_stage_joint.
#pragma once
#include "rbd_tangent_mk.hpp"

namespace rbd {

RBD_HD bool mk_narrow_joint(int jt) { return jt == RBD_JOINT_REVOLUTE || jt == RBD_JOINT_PRISMATIC || jt == RBD_JOINT_SINCOS_REVOLUTE; }

// input coordinates per forward pass of the contractions
template <typename T> struct AdjMkChunk { enum { N = 2 }; };  // (4: 520 bytes of scratch per lane in fp64 on gfx950; 2: none)

// x[0 … K) as Duals seeded with the unit directions of the pass: d[j] = 1 where input base + k is input e0 + j (compares, no indexing by a variable)
template <typename T, int N, int K> RBD_HD void adj_seed(const T* x, int n, int base, int e0, Dual<T, N>* o) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    o[k] = Dual<T, N>(k < n ? x[k] : T(0));
#pragma unroll
    for (int j = 0; j < N; ++j) o[k].d[j] = k < n && base + k == e0 + j ? T(1) : T(0);
  }
}
// xb[k] += g[j] where input base + k is input e0 + j
template <typename T, int N, int K> RBD_HD void adj_gather(const T* g, int n, int base, int e0, T* xb) {
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (k < n && base + k == e0 + j) xb[k] += g[j];
}

// ϕ̇ of tan_joint_local_rate, values only
template <typename T> RBD_HD void mk_rate_value(int jt, const T* q0, const T* qs, const T* vs, T* rate) {
  using D = Dual<T, 1>;
  D a[7], b[7], c[6], o[6];
#pragma unroll
  for (int k = 0; k < 7; ++k) { a[k] = D(q0[k]); b[k] = D(qs[k]); }
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] = D(vs[k]);
  tan_joint_local_rate<T, 1>(jt, a, b, c, o);
#pragma unroll
  for (int k = 0; k < 6; ++k) rate[k] = o[k].v;
}

// (q̄0, q̄s, v̄s) += (∂ϕ̇/∂(q0, qs, vs))ᵀ ϕ̇̄ (ϕ̇̄ zero past the joint's nv)
template <typename T, int N> RBD_HD void adj_joint_local_rate(int jt, const T* q0, const T* qs, const T* vs, const T* rb, T* q0b, T* qsb, T* vsb) {
  using D = Dual<T, N>;
  const int nq = joint_nq<T>(jt), nv = joint_nv(jt), nin = 2 * nq + nv;
  for (int e0 = 0; e0 < nin; e0 += N) {
    D a[7], b[7], c[6], o[6];
    adj_seed<T, N, 7>(q0, nq, 0, e0, a);
    adj_seed<T, N, 7>(qs, nq, nq, e0, b);
    adj_seed<T, N, 6>(vs, nv, 2 * nq, e0, c);
    tan_joint_local_rate<T, N>(jt, a, b, c, o);
    T g[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      g[j] = T(0);
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (k < nv) g[j] += rb[k] * o[k].d[j];
    }
    adj_gather<T, N, 7>(g, nq, 0, e0, q0b);
    adj_gather<T, N, 7>(g, nq, nq, e0, qsb);
    adj_gather<T, N, 6>(g, nv, 2 * nq, e0, vsb);
  }
}

// (q̄0, ϕ̄) += (∂q/∂(q0, ϕ))ᵀ q̄ of tan_joint_global
template <typename T, int N> RBD_HD void adj_joint_global(int jt, const T* q0, const T* phi, const T* qb, T* q0b, T* phib) {
  using D = Dual<T, N>;
  const int nq = joint_nq<T>(jt), nv = joint_nv(jt), nin = nq + nv;
  for (int e0 = 0; e0 < nin; e0 += N) {
    D a[7], b[6], o[7];
    adj_seed<T, N, 7>(q0, nq, 0, e0, a);
    adj_seed<T, N, 6>(phi, nv, nq, e0, b);
    tan_joint_global<T, N>(jt, a, b, o);
    T g[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      g[j] = T(0);
#pragma unroll
      for (int k = 0; k < 7; ++k)
        if (k < nq) g[j] += qb[k] * o[k].d[j];
    }
    adj_gather<T, N, 7>(g, nq, 0, e0, q0b);
    adj_gather<T, N, 6>(g, nv, nq, e0, phib);
  }
}

// global_coordinates! of a 1-coordinate joint: q0 + ϕ, or (s, c) rotated by ϕ (tan_joint_global's formulas)
template <typename T> RBD_HD void mk_narrow_global(int jt, const T* q0, T phi, T* q) {
  if (jt == RBD_JOINT_SINCOS_REVOLUTE) {
    T sd, cd;
    sincos_t(phi, &sd, &cd);
    q[0] = q0[0] * cd + q0[1] * sd;
    q[1] = q0[1] * cd - q0[0] * sd;
  } else {
    q[0] = q0[0] + phi;
  }
}
template <typename T> RBD_HD void adj_narrow_global(int jt, const T* q0, T phi, const T* qb, T* q0b, T* phib) {
  if (jt == RBD_JOINT_SINCOS_REVOLUTE) {
    T sd, cd;
    sincos_t(phi, &sd, &cd);
    q0b[0] += qb[0] * cd - qb[1] * sd;
    q0b[1] += qb[0] * sd + qb[1] * cd;
    *phib += qb[0] * (q0[1] * cd - q0[0] * sd) - qb[1] * (q0[1] * sd + q0[0] * cd);
  } else {
    q0b[0] += qb[0];
    *phib += qb[0];
  }
}

// The transpose of tan_mk_stage_joint(jt, stage, dt, …) at the values (q0, qs, vs) and, at stage 3, accp (the sums Σ_{j<3} dt b_j ϕ̇_j in; v0 and v̇ enter
// linearly, their values are not needed).  In: qnb, vnb, the cotangents of the next stage state (stage 3: of the state after the step), and accpb, accvb,
// those of the sums out (stages 0-2; ignored at stage 3).  Out: accpb, accvb become the cotangents of the sums in (stages 1-3; zero at stage 0), and the
// cotangents of q0, v0, qs, vs and v̇ are ADDED to q0b, v0b, qsb, vsb, vdb.  Arrays hold 7 (q) and 6 (v) entries, zero past the joint's coordinates.
// WIDE = false: 1-coordinate joints only, without the Dual code.
template <typename T, bool WIDE = true, int N = AdjMkChunk<T>::N>
RBD_HD void adj_mk_stage_joint(int jt, int stage, T dt, const T* q0, const T* qs, const T* vs, const T* accp, const T* qnb, const T* vnb, T* accpb, T* accvb,
                               T* q0b, T* v0b, T* qsb, T* vsb, T* vdb) {
  constexpr int KV = WIDE ? 6 : 1;
  const bool narrow = !WIDE || mk_narrow_joint(jt);
  const int nv = joint_nv(jt);
  const T b = stage == 0 || stage == 3 ? T(1) / 6 : T(1) / 3;  // (ode_integrators.jl:48-55)
  const T wb = dt * b;
  const T wa = dt * (stage == 2 ? T(1) : T(0.5));
  T rate[6], phi[6], phib[6], rateb[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) { rate[k] = T(0); phi[k] = T(0); phib[k] = T(0); rateb[k] = T(0); }
  if (narrow) {
    rate[0] = vs[0];
  } else if constexpr (WIDE) {
    mk_rate_value(jt, q0, qs, vs, rate);
  }
#pragma unroll
  for (int k = 0; k < KV; ++k)
    if (k < nv) phi[k] = stage < 3 ? wa * rate[k] : accp[k] + wb * rate[k];
  if (narrow) {
    adj_narrow_global(jt, q0, phi[0], qnb, q0b, phib);
  } else if constexpr (WIDE) {
    adj_joint_global<T, N>(jt, q0, phi, qnb, q0b, phib);
  }
  // the tableau: stages 0-2 ϕ = dt a ϕ̇, v_n = v0 + dt a v̇, sums += dt b (ϕ̇, v̇); stage 3 (ϕ, v_n) = the sums + dt b (ϕ̇, v̇)
#pragma unroll
  for (int k = 0; k < KV; ++k)
    if (k < nv) {
      if (stage < 3) {
        rateb[k] = wa * phib[k] + wb * accpb[k];
        v0b[k] += vnb[k];
        vdb[k] += wa * vnb[k] + wb * accvb[k];
        if (stage == 0) {  // (the sums start as dt b ϕ̇ and v0 + dt b v̇)
          v0b[k] += accvb[k];
          accpb[k] = T(0); accvb[k] = T(0);
        }
      } else {
        rateb[k] = wb * phib[k];
        vdb[k] += wb * vnb[k];
        accpb[k] = phib[k]; accvb[k] = vnb[k];
      }
    }
  if (narrow) {
    vsb[0] += rateb[0];  // (ϕ̇ = v)
  } else if constexpr (WIDE) {
    adj_joint_local_rate<T, N>(jt, q0, qs, vs, rateb, q0b, qsb, vsb);
  }
}

// The values of tan_mk_stage_joint (the same arguments, plain numbers): the value stage map of rbd_simulate_vjp's forward and recompute passes.
template <typename T, bool WIDE = true>
RBD_HD void mk_stage_value_joint(int jt, int stage, T dt, const T* q0, const T* v0, const T* qs, const T* vs, const T* vd, T* accp, T* accv, T* qn, T* vn) {
  if (!WIDE || mk_narrow_joint(jt)) {
    const T b = stage == 0 || stage == 3 ? T(1) / 6 : T(1) / 3;
    const T wb = dt * b;
    const T wa = dt * (stage == 2 ? T(1) : T(0.5));
    const T rate = vs[0];
    const T sp = stage == 0 ? wb * rate : accp[0] + wb * rate;
    const T sv = (stage == 0 ? v0[0] : accv[0]) + wb * vd[0];
    T phi;
    if (stage < 3) {
      accp[0] = sp; accv[0] = sv;
      phi = wa * rate;
      vn[0] = v0[0] + wa * vd[0];
    } else {
      phi = sp; vn[0] = sv;
    }
    mk_narrow_global(jt, q0, phi, qn);
  } else if constexpr (WIDE) {
    using D = Dual<T, 1>;
    D a[7], b[7], c[6], d[6], e[6], f[6], g[6], o[7], p[6];
#pragma unroll
    for (int k = 0; k < 7; ++k) { a[k] = D(q0[k]); b[k] = D(qs[k]); }
#pragma unroll
    for (int k = 0; k < 6; ++k) { c[k] = D(v0[k]); d[k] = D(vs[k]); e[k] = D(vd[k]); f[k] = D(accp[k]); g[k] = D(accv[k]); }
    tan_mk_stage_joint<T, 1>(jt, stage, dt, a, c, b, d, e, f, g, o, p);
#pragma unroll
    for (int k = 0; k < 7; ++k) qn[k] = o[k].v;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      vn[k] = p[k].v;
      if (stage < 3) { accp[k] = f[k].v; accv[k] = g[k].v; }
    }
  }
}

// one launch of value_mk_stage_kernel / adjoint_mk_stage_kernel (rbd_tangent_kernels.hip): one class of joints (1-coordinate or not), one thread per
// (joint of the class, state), thread = j · B + state; each thread reads and writes only its own joint's rows.
template <typename T> struct MkAdjArgs {
  long B;
  int nj, stage;      // joints of the launch's class, stage 0..3
  T dt;
  const int32_t* jl;  // the class's joints: (jtype, qoff, voff) each
  const T *q0, *v0, *qs, *vs, *vd;  // values, layouts Lq and Lv (v0, vd: the value map only)
  T *accp, *accv;                   // the running sums (Lv): written by the value map at stages 0-2; the pullback reads accp at stage 3
  T *qn, *vn;                       // the value map's next stage state (stage 3: the state after the step; may be q0 / v0 itself)
  Layout Lq, Lv;
  // the pullback.  qsb, vsb (layouts Lqb, Lvb): in, the cotangent of the stage's output; out, that of its stage state (stage 0: of the step's start,
  // q̄0 + q̄s).  Batch-innermost (row r of state b at r B + b): q0b, v0b, the base point's cotangent over stages 3 … 1 (written at 3, read at 0);
  // vdb, v̇̄ of the stage (out); apb, avb, the running sums' cotangents (written at 3, read at 2 … 0).
  T *qsb, *vsb, *q0b, *v0b, *vdb, *apb, *avb;
  Layout Lqb, Lvb;
};

}  // namespace rbd
