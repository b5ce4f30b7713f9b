/*
 * rbd_oracle_q.c — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * The oracle of rbd_oracle_impl.h instantiated a third time, in IEEE binary128 (_Float128 arithmetic and the libm *f128 functions; no
 * libquadmath), with drivers that differentiate it by central differences evaluated wholly in quad: the reference of the derivative kernels.
 * It is the same program text as the fp64 oracle, hence the same function of RAW coordinates (a quaternion off its unit sphere included).
 * Built by oracle/Makefile into oracle/librbd_oracle_q.so, an object of its own: the fp64 oracle, its flags and its tests do not depend on it.
 *
 * numpy has no binary128, so nothing quad crosses this file's boundary: the drivers take doubles (widened exactly), evaluate and difference
 * in quad and round the result to double once, at the end.
 *
 * Why a difference quotient is exact here: with u = 2^-113 ≈ 1e-34 the quotient (f(h) − f(−h)) / 2h carries a truncation error h² f'''/6 and a
 * rounding error ≈ cond · u / h; at h = 1e-11 these are ≈ 1e-23 · f''' and ≈ 1e-23 · cond, both far below the 1.1e-16 of the final rounding to
 * double.  The 4-point form (8 (f(h) − f(−h)) − (f(2h) − f(−2h))) / 12h has the truncation error h⁴ f⁽⁵⁾/30 and serves larger steps.
 * tests/test_oracle_quad.py proves both on every model: the result at h and at 3h agree to 1e-14 of the scale, and on the double pendulum they
 * equal the closed-form derivative.  No evaluation at the centre point enters a derivative.
 *
 * The contact path of the impl header calls pow through double; it compiles here but is not quad-accurate and no driver reaches it.
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "rbd_hip.h"

#define REAL _Float128
#define SFX _f128
#define SIN sinf128
#define COS cosf128
#define SQRT sqrtf128
#include "rbd_oracle_impl.h"
#undef REAL
#undef SFX
#undef SIN
#undef COS
#undef SQRT

typedef _Float128 quad;

/* what: the codes of rbdo_batch (0 dynamics by the reference's route, 1 inverse dynamics, 2 dynamics bias, 4 ABA) */
static int q_eval(const rbd_flat_model_t* m, int what, const quad* q, const quad* v, const quad* x, const quad* f, quad* out) {
  switch (what) {
    case 0: return rbdo_dynamics_f128(m, q, v, x, f, out, NULL, NULL, NULL);
    case 1: return rbdo_inverse_dynamics_f128(m, q, v, x, f, out);
    case 2: return rbdo_dynamics_bias_f128(m, q, v, f, out);
    case 4: return rbdo_aba_f128(m, q, v, x, f, out);
    default: return RBD_ERR_INVALID_ARGUMENT;
  }
}

/* o = a + s d in quad (a NULL: zero; d NULL: no displacement), plus s on coordinate `unit` (< 0: none) */
static void q_point(quad* o, const double* a, const double* d, quad s, int n, int unit) {
  for (int i = 0; i < n; ++i) o[i] = (a ? (quad)a[i] : (quad)0) + (d ? s * (quad)d[i] : (quad)0);
  if (unit >= 0 && unit < n) o[unit] += s;
}

/* One state, one direction: f(0) rounded to double into val (nullable) and the directional derivative into out (stride ostride).  The direction is
 * (dq, dv, dx, df), any of them NULL, plus the unit vector `unit` of the concatenated (q, v, x) coordinates (< 0: none).
 * points: 2 or 4 (see the head of the file). */
static int q_directional(const rbd_flat_model_t* m, int what, const double* q, const double* v, const double* x, const double* f, const double* dq,
                         const double* dv, const double* dx, const double* df, int unit, double h, int points, double* val, double* out, int ostride) {
  const int nq = m->nq, nv = m->nv, nf = 6 * m->n_bodies;
  if (points != 2 && points != 4) return RBD_ERR_INVALID_ARGUMENT;
  quad* buf = (quad*)malloc(sizeof(quad) * (size_t)(nq + 4 * nv + nf + 1));
  if (!buf) return RBD_ERR_OUT_OF_MEMORY;
  quad *Q = buf, *V = Q + nq, *X = V + nv, *F = X + nv, *o = F + nf, *acc = o + nv;
  const int has_x = x || dx || (unit >= nq + nv), has_f = f || df;
  const quad H = (quad)h;
  const int k[5] = {1, -1, 2, -2, 0};
  const quad w2[2] = {1, -1}, w4[4] = {8, -8, -1, 1};
  int st = RBD_OK;
  for (int i = 0; i < nv; ++i) acc[i] = 0;
  for (int e = 0; e < 5 && st == RBD_OK; ++e) {
    if (e < 4 ? (!out || e >= points) : !val) continue;
    const quad s = (quad)k[e] * H;
    q_point(Q, q, dq, s, nq, unit);
    q_point(V, v, dv, s, nv, unit - nq);
    q_point(X, x, dx, s, nv, unit - nq - nv);
    q_point(F, f, df, s, nf, -1);
    st = q_eval(m, what, Q, V, has_x ? X : NULL, has_f ? F : NULL, o);
    if (st != RBD_OK) break;
    if (e == 4) for (int i = 0; i < nv; ++i) val[i] = (double)o[i];
    else for (int i = 0; i < nv; ++i) acc[i] += (points == 2 ? w2[e] : w4[e]) * o[i];
  }
  if (st == RBD_OK && out) for (int i = 0; i < nv; ++i) out[(size_t)i * ostride] = (double)(acc[i] / ((points == 2 ? (quad)2 : (quad)12) * H));
  free(buf);
  return st;
}

/* Values in quad, rounded to double: out[B, nv]; what == 3: the mass matrix, out[B, nv*nv] as rbdo_batch leaves it. */
int rbdo_q_values(const rbd_flat_model_t* m, int what, int B, int nthreads, const double* q, const double* v, const double* x, const double* fext,
                  double* out) {
  const int nq = m->nq, nv = m->nv, nf = 6 * m->n_bodies;
  int status = RBD_OK;
  if (nthreads < 1) nthreads = 1;
#pragma omp parallel for num_threads(nthreads) schedule(dynamic)
  for (int b = 0; b < B; ++b) {
    int st;
    if (what == 3) {
      quad* Q = (quad*)malloc(sizeof(quad) * (size_t)(nq + nv * nv + 1));
      quad* M = Q + nq;
      q_point(Q, q + (size_t)b * nq, NULL, 0, nq, -1);
      st = rbdo_mass_matrix_f128(m, Q, M);
      for (int i = 0; i < nv * nv; ++i) out[(size_t)b * nv * nv + i] = (double)M[i];
      free(Q);
    } else {
      st = q_directional(m, what, q + (size_t)b * nq, v ? v + (size_t)b * nv : NULL, x ? x + (size_t)b * nv : NULL, fext ? fext + (size_t)b * nf : NULL,
                         NULL, NULL, NULL, NULL, -1, 1.0, 2, out + (size_t)b * nv, NULL, 1);
    }
    if (st != RBD_OK) {
#pragma omp critical
      status = st;
    }
  }
  return status;
}

/* Directional derivatives along ntan directions per state: dq[B, ntan, nq], dv[B, ntan, nv], dx[B, ntan, nv] (dτ or dv̇), dfext[B, ntan, 6 n_bodies],
 * any of them NULL; out[B, ntan, nv], val[B, nv] (nullable).  OpenMP over (state, direction). */
int rbdo_q_jvp(const rbd_flat_model_t* m, int what, int B, int ntan, int nthreads, const double* q, const double* v, const double* x, const double* fext,
               const double* dq, const double* dv, const double* dx, const double* dfext, double h, int points, double* val, double* out) {
  const size_t nq = (size_t)m->nq, nv = (size_t)m->nv, nf = 6 * (size_t)m->n_bodies;
  int status = RBD_OK;
  if (nthreads < 1) nthreads = 1;
  if (ntan < 1 || !(h > 0)) return RBD_ERR_INVALID_ARGUMENT;
#pragma omp parallel for num_threads(nthreads) schedule(dynamic)
  for (long job = 0; job < (long)B * ntan; ++job) {
    const size_t b = (size_t)(job / ntan), d = (size_t)(job % ntan), bd = b * (size_t)ntan + d;
    int st = q_directional(m, what, q + b * nq, v ? v + b * nv : NULL, x ? x + b * nv : NULL, fext ? fext + b * nf : NULL, dq ? dq + bd * nq : NULL,
                           dv ? dv + bd * nv : NULL, dx ? dx + bd * nv : NULL, dfext ? dfext + bd * nf : NULL, -1, h, points,
                           (val && d == 0) ? val + b * nv : NULL, out + bd * nv, 1);
    if (st != RBD_OK) {
#pragma omp critical
      status = st;
    }
  }
  return status;
}

/* Full Jacobians by unit directions: Jq[B, nv, nq], Jv[B, nv, nv], Jx[B, nv, nv] (∂/∂τ or ∂/∂v̇), row-major per state (J[b][i][j] = ∂out_i/∂coordinate_j),
 * each nullable, and the value f(0) in val[B, nv] (nullable).  OpenMP over (state, column). */
int rbdo_q_jacobians(const rbd_flat_model_t* m, int what, int B, int nthreads, const double* q, const double* v, const double* x, const double* fext,
                     double h, int points, double* val, double* Jq, double* Jv, double* Jx) {
  const size_t nq = (size_t)m->nq, nv = (size_t)m->nv, nf = 6 * (size_t)m->n_bodies;
  const long ncol = (long)(nq + 2 * nv);
  int status = RBD_OK;
  if (nthreads < 1) nthreads = 1;
  if (!(h > 0)) return RBD_ERR_INVALID_ARGUMENT;
#pragma omp parallel for num_threads(nthreads) schedule(dynamic)
  for (long job = 0; job < (long)B * ncol; ++job) {
    const size_t b = (size_t)(job / ncol), j = (size_t)(job % ncol);
    double* col; int stride;
    if (j < nq) { col = Jq ? Jq + b * nv * nq + j : NULL; stride = (int)nq; }
    else if (j < nq + nv) { col = Jv ? Jv + b * nv * nv + (j - nq) : NULL; stride = (int)nv; }
    else { col = Jx ? Jx + b * nv * nv + (j - nq - nv) : NULL; stride = (int)nv; }
    double* vb = (val && j == 0) ? val + b * nv : NULL;
    if (!col && !vb) continue;
    int st = q_directional(m, what, q + b * nq, v ? v + b * nv : NULL, x ? x + b * nv : NULL, fext ? fext + b * nf : NULL, NULL, NULL, NULL, NULL, (int)j, h,
                           points, vb, col, stride);
    if (st != RBD_OK) {
#pragma omp critical
      status = st;
    }
  }
  return status;
}
