"""Reverse-mode derivatives of inverse_dynamics! without a GPU (header 700 additions): rbd_inverse_dynamics_vjp and rbd_dynamics_vjp are declared and
exported, and the per-state adjoint routine of their kernel (csrc/rbd_adjoint.hpp adjoint_rnea_state), compiled as plain C++ for the host beside the
tangent routine (csrc/rbd_tangent.hpp tangent_rnea_state), is exactly its transpose: ⟨λ, J d⟩ = ⟨Jᵀλ, d⟩ for random cotangents and directions over
(q, v, v̇, f_ext), quaternion directions off the unit sphere included.  q̄, v̄, v̇̄ are also checked against Jᵀλ from the quad-precision oracle's Jacobians
(oracle.jacobians), f̄ext against its derivative along every wrench coordinate, and v̇̄ against Mλ."""
import ctypes
import os

import numpy as np
import pytest

from host_harness import CLANG, ROOT, build
from test_derivatives_cpu import tables

NEW = ("rbd_inverse_dynamics_vjp", "rbd_dynamics_vjp")
MODELS = ["randmech1", "randmech2", "randmech3", "inner_floating", "mixed20", "double_pendulum"]

HARNESS = r"""
#include <hip/hip_runtime.h>
#include "rbd_adjoint.hpp"
thread_local EmuDim3 threadIdx, blockIdx, blockDim, gridDim;
int emu_unreachable(const char*) { __builtin_trap(); return 0; }
// state-major (AOS) buffers, one state after the other, a scratch of one thread
extern "C" void emu_tangent_rnea(int nb, int nq, int nv, const int* tbl, const double* rb, const double* g, long B, const double* q, const double* v,
                                 const double* vdot, const double* fext, const double* dq, const double* dv, const double* dvdot, const double* dfext,
                                 double* dtau) {
  constexpr int N = 2;
  rbd::BigModel M{nb, nq, nv, 0, tbl, rb, {g[0], g[1], g[2]}};
  rbd::TanArgs<double> A{};
  A.B = B; A.ntan = 1; A.q = q; A.v = v; A.vdot = vdot; A.fext = fext; A.dq = dq; A.dv = dv; A.dvdot = dvdot; A.dfext = dfext;
  A.Lq = A.Ldq = rbd::Layout{1, nq}; A.Lv = A.Ldv = rbd::Layout{1, nv}; A.Lf = A.Ldf = rbd::Layout{1, 6L * nb};
  A.tau = nullptr; A.sign = 1.0; A.dadd = nullptr;
  A.out = rbd::ColOut<double>::single(dtau, A.Ldv, nv);
  double* sc = new double[(size_t)rbd::TAN_FIELDS * (N + 1) * nb];
  for (long st = 0; st < B; ++st) rbd::tangent_rnea_state<double, N>(M, A, st, 0, sc, 1, 0);
  delete[] sc;
}
extern "C" void emu_adjoint_rnea(int nb, int nq, int nv, const int* tbl, const double* rb, const double* g, long B, const double* q, const double* v,
                                 const double* vdot, const double* fext, const double* lam, double* tau, double* qbar, double* vbar, double* vdbar,
                                 double* fbar) {
  rbd::BigModel M{nb, nq, nv, 0, tbl, rb, {g[0], g[1], g[2]}};
  rbd::AdjArgs<double> A{};
  A.B = B; A.q = q; A.v = v; A.vdot = vdot; A.fext = fext; A.lam = lam;
  A.Lq = rbd::Layout{1, nq}; A.Lv = A.Llam = rbd::Layout{1, nv}; A.Lf = rbd::Layout{1, 6L * nb};
  A.tau = tau; A.qbar = qbar; A.vbar = vbar; A.vdbar = vdbar; A.fbar = fbar; A.sign = 1.0;
  double* sc = new double[(size_t)rbd::ADJ_FIELDS * nb];
  for (long st = 0; st < B; ++st) rbd::adjoint_rnea_state<double>(M, A, st, sc, 1, 0);
  delete[] sc;
}
"""


def build_harness():
    return build(HARNESS, "rbd_adjoint_emu")


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dims(flat):
    tbl, rb = tables(flat)
    return [ctypes.c_int(flat.n_bodies), ctypes.c_int(flat.nq), ctypes.c_int(flat.nv), _p(tbl), _p(rb), _p(np.asarray(flat.gravity, dtype=np.float64))], (tbl, rb)


def emu_jvp(lib, flat, q, v, vd, fext, dq, dv, dvd, dfext):
    """J·d for one direction per state (the tangent routine)."""
    B = q.shape[0]
    head, keep = _dims(flat)
    args = [_c(x) for x in (q, v, vd, fext, dq, dv, dvd, dfext)]
    dtau = np.full((B, flat.nv), np.nan)
    lib.emu_tangent_rnea(*head, ctypes.c_long(B), *[_p(a) for a in args], _p(dtau))
    return dtau


def emu_vjp(lib, flat, q, v, vd, fext, lam):
    """τ and Jᵀλ = (q̄, v̄, v̇̄, f̄ext) per state (the adjoint routine)."""
    B = q.shape[0]
    head, keep = _dims(flat)
    args = [_c(x) for x in (q, v, vd, fext, lam)]
    out = [np.full((B, n), np.nan) for n in (flat.nv, flat.nq, flat.nv, flat.nv, 6 * flat.n_bodies)]
    lib.emu_adjoint_rnea(*head, ctypes.c_long(B), *[_p(a) for a in args], *[_p(o) for o in out])
    return out


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang")
    return build_harness()


def test_symbols_declared_and_exported(rbd):
    header = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in rbd._capi.SYMBOLS, name
    assert "#define RBD_HIP_H_VERSION 700" in header and rbd._capi.HEADER_VERSION == 700
    lib = ctypes.CDLL(rbd._capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name


def inputs(rbd, flat, B, seed, with_fext):
    rng = np.random.default_rng(seed)
    q = rbd.rand_configuration(flat, B, rng)
    v = rbd.rand_velocity(flat, B, rng)
    vd = rng.standard_normal((B, flat.nv))
    fext = rng.standard_normal((B, 6 * flat.n_bodies)) if with_fext else None
    return rng, q, v, vd, fext


@pytest.mark.parametrize("with_fext", [False, True])
@pytest.mark.parametrize("name", MODELS)
def test_adjoint_is_the_transpose_of_the_tangent(harness, models, oracle, rbd, name, with_fext):
    """⟨λ, J d⟩ = ⟨q̄, dq⟩ + ⟨v̄, dv⟩ + ⟨v̇̄, dv̇⟩ + ⟨f̄ext, dfext⟩ per state, to 1e-12 of the terms' magnitude; dq is not projected on any quaternion's sphere."""
    flat = models[name]
    B = 6
    rng, q, v, vd, fext = inputs(rbd, flat, B, 17, with_fext)
    lam = rng.standard_normal((B, flat.nv))
    tau, qb, vb, vdb, fb = emu_vjp(harness, flat, q, v, vd, fext, lam)
    ref_tau = oracle.inverse_dynamics(flat, q, v, vd, fext)
    assert np.abs(tau - ref_tau).max() <= 1e-10 * (1 + np.abs(ref_tau).max())
    for trial in range(3):
        dq = rng.standard_normal((B, flat.nq))
        dv = rng.standard_normal((B, flat.nv))
        dvd = rng.standard_normal((B, flat.nv))
        dfe = rng.standard_normal((B, 6 * flat.n_bodies))
        if trial == 1:  # (separately: q alone, v alone)
            dv[:] = dvd[:] = dfe[:] = 0
        Jd = emu_jvp(harness, flat, q, v, vd, fext, dq, dv, dvd, dfe)
        lhs = np.sum(lam * Jd, axis=1)
        terms = [qb * dq, vb * dv, vdb * dvd, fb * dfe]
        rhs = sum(np.sum(t, axis=1) for t in terms)
        mag = sum(np.sum(np.abs(t), axis=1) for t in terms) + np.sum(np.abs(lam * Jd), axis=1)
        assert (np.abs(lhs - rhs) <= 1e-12 * mag).all(), (name, trial, np.abs(lhs - rhs) / mag)


@pytest.mark.parametrize("name", MODELS)
def test_adjoint_against_the_oracle(harness, models, oracle, rbd, name):
    """q̄, v̄, v̇̄ against Jᵀλ with the Jacobians of the quad-precision oracle, f̄ext against λᵀ ∂τ/∂f_ext from its derivative along every wrench coordinate, at the
    fp64 parity number 1e-10 (no solve in τ); v̇̄ = Mλ with M from the oracle."""
    flat = models[name]
    B = 3
    rng, q, v, vd, fext = inputs(rbd, flat, B, 23, True)
    lam = rng.standard_normal((B, flat.nv))
    _, qb, vb, vdb, fb = emu_vjp(harness, flat, q, v, vd, fext, lam)
    J = oracle.jacobians(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext)
    nf = 6 * flat.n_bodies
    Jf = oracle.jvp(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext, dfext=np.tile(np.eye(nf)[None], (B, 1, 1)))  # [b, wrench coordinate, i]
    for got, ref in ((qb, np.einsum("bij,bi->bj", J["q"], lam)), (vb, np.einsum("bij,bi->bj", J["v"], lam)), (vdb, np.einsum("bij,bi->bj", J["x"], lam)),
                     (fb, np.einsum("bji,bi->bj", Jf, lam))):
        assert np.abs(got - ref).max() <= 1e-10 * (1 + np.abs(ref).max()), (name, np.abs(got - ref).max())
    Mo = oracle.mass_matrix(flat, q)
    Ms = np.tril(Mo) + np.transpose(np.tril(Mo, -1), (0, 2, 1))
    ref = np.einsum("bij,bj->bi", Ms, lam)
    assert np.abs(vdb - ref).max() <= 1e-12 * (1 + np.abs(ref).max())
