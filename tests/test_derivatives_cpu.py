"""Forward-mode derivatives of inverse_dynamics! without a GPU (header 700): the four entry points are declared and exported, and the per-state tangent
routine of the derivative kernels (csrc/rbd_tangent.hpp tangent_rnea_state), compiled as plain C++ for the host like tests/emu/spec_emu.py does, matches the
directional derivative of the quad-precision oracle (oracle.jvp: exact to double rounding) at the project's fp64 parity number 1e-10 — every joint type, random
directions, quaternion directions off the unit sphere included."""
import ctypes
import os

import numpy as np
import pytest

from host_harness import CLANG, ROOT, build

NEW = ("rbd_inverse_dynamics_jvp", "rbd_dynamics_jvp", "rbd_inverse_dynamics_derivatives", "rbd_dynamics_derivatives")

HARNESS = r"""
#include <hip/hip_runtime.h>
#include "rbd_tangent.hpp"
thread_local EmuDim3 threadIdx, blockIdx, blockDim, gridDim;
int emu_unreachable(const char*) { __builtin_trap(); return 0; }
// one (state, chunk) after the other, state-major (AOS) buffers; scratch of one thread
extern "C" void emu_tangent_rnea(int nb, int nq, int nv, const int* tbl, const double* rb, const double* g, long B, int ntan, const double* q, const double* v,
                                 const double* vdot, const double* fext, const double* dq, const double* dv, const double* dvdot, const double* dfext, double* tau,
                                 double* dtau) {
  constexpr int N = 2;
  rbd::BigModel M{nb, nq, nv, 0, tbl, rb, {g[0], g[1], g[2]}};
  rbd::TanArgs<double> A{};
  A.B = B; A.ntan = ntan; A.q = q; A.v = v; A.vdot = vdot; A.fext = fext; A.dq = dq; A.dv = dv; A.dvdot = dvdot; A.dfext = dfext;
  A.Lq = rbd::Layout{1, nq}; A.Lv = rbd::Layout{1, nv}; A.Lf = rbd::Layout{1, 6L * nb};
  A.Ldq = rbd::Layout{1, (long)nq * ntan}; A.Ldv = rbd::Layout{1, (long)nv * ntan}; A.Ldf = rbd::Layout{1, 6L * nb * ntan};
  A.tau = tau; A.sign = 1.0; A.dadd = nullptr;
  A.out = rbd::ColOut<double>::single(dtau, A.Ldv, nv);
  double* sc = new double[(size_t)rbd::TAN_FIELDS * (N + 1) * nb];
  for (int c = 0; c < (ntan + N - 1) / N; ++c)
    for (long st = 0; st < B; ++st) rbd::tangent_rnea_state<double, N>(M, A, st, c, sc, 1, 0);
  delete[] sc;
}
"""


def build_harness():
    return build(HARNESS, "rbd_tangent_emu")


def tables(flat):
    """BigModel's tables in the reference's order: (parent, joint type, q offset, v offset), RB_* records (rbd_device.hpp)."""
    n = flat.n_bodies
    tbl = np.stack([flat.parent, flat.joint_type, flat.q_offset, flat.v_offset], axis=1).astype(np.int32).ravel()
    rb = np.zeros((n, 28))
    rb[:, 0:3] = flat.joint_axis
    rb[:, 3:6] = flat.joint_axis2
    rb[:, 6:15] = flat.pred_rot.reshape(n, 9)
    rb[:, 15:18] = flat.pred_trans
    J = flat.inertia_moment
    rb[:, 18:24] = np.stack([J[:, 0, 0], J[:, 0, 1], J[:, 0, 2], J[:, 1, 1], J[:, 1, 2], J[:, 2, 2]], axis=1)
    rb[:, 24:27] = flat.inertia_cross
    rb[:, 27] = flat.inertia_mass
    return tbl, rb.ravel()


def emu_jvp(lib, flat, q, v, vd, fext, dq, dv, dvd, dfext, ntan):
    B = q.shape[0]
    tbl, rb = tables(flat)
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    args = [c(x) for x in (q, v, vd, fext, dq, dv, dvd, dfext)]
    tau = np.full((B, flat.nv), np.nan)
    dtau = np.full((B, flat.nv * ntan), np.nan)
    g = np.asarray(flat.gravity, dtype=np.float64)
    lib.emu_tangent_rnea(ctypes.c_int(flat.n_bodies), ctypes.c_int(flat.nq), ctypes.c_int(flat.nv), p(tbl), p(rb), p(g), ctypes.c_long(B), ctypes.c_int(ntan),
                         *[p(a) for a in args], p(tau), p(dtau))
    return tau, dtau


def quad_jvp(oracle, flat, q, v, vd, fext, dq, dv, dvd, dfext):
    """The directional derivative of the oracle's inverse_dynamics in raw coordinates, evaluated in quad precision: one direction per state."""
    return oracle.jvp(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext, dq, dv, dvd, dfext)


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


@pytest.mark.parametrize("name", ["randmech1", "randmech2", "randmech3", "inner_floating", "mixed20", "double_pendulum"])
def test_tangent_routine_matches_central_difference(harness, models, oracle, rbd, name):
    flat = models[name]
    B, ntan = 3, 3
    rng = np.random.default_rng(5)
    q = rbd.rand_configuration(flat, B, rng)
    v = rbd.rand_velocity(flat, B, rng)
    vd = rng.standard_normal((B, flat.nv))
    fext = rng.standard_normal((B, 6 * flat.n_bodies))
    # directions: q tangents NOT projected on the unit sphere of a quaternion (the raw-coordinate derivative), plus v, v̇ and f_ext directions
    dq = rng.standard_normal((B, ntan, flat.nq))
    dv = rng.standard_normal((B, ntan, flat.nv))
    dvd = rng.standard_normal((B, ntan, flat.nv))
    dfe = rng.standard_normal((B, ntan, 6 * flat.n_bodies))
    dfe[:, 1] = 0  # (one direction without a wrench part)
    tau, dtau = emu_jvp(harness, flat, q, v, vd, fext, dq.reshape(B, -1), dv.reshape(B, -1), dvd.reshape(B, -1), dfe.reshape(B, -1), ntan)
    ref_tau = oracle.inverse_dynamics(flat, q, v, vd, fext)
    assert np.abs(tau - ref_tau).max() <= 1e-10 * (1 + np.abs(ref_tau).max())
    got = dtau.reshape(B, ntan, flat.nv)
    for d in range(ntan):
        ref = quad_jvp(oracle, flat, q, v, vd, fext, dq[:, d], dv[:, d], dvd[:, d], dfe[:, d])
        err = np.abs(got[:, d] - ref).max()
        assert err <= 1e-10 * (1 + np.abs(ref).max()), (name, d, err)  # (no solve in τ: the fp64 parity number; it was 1e-7 against an fp64 difference)


def test_tangent_routine_pure_q_directions(harness, models, oracle, rbd):
    """∂τ/∂q alone, radially along q itself (off the unit sphere for every quaternion: the part a Lie-algebra derivative would leave out) and along a random
    direction; NULL v, v̇ and wrench tangents are zero directions."""
    flat = models["inner_floating"]
    B, ntan = 2, 2
    rng = np.random.default_rng(9)
    q = rbd.rand_configuration(flat, B, rng)
    v = rbd.rand_velocity(flat, B, rng)
    vd = rng.standard_normal((B, flat.nv))
    fext = np.zeros((B, 6 * flat.n_bodies))
    dq = np.zeros((B, ntan, flat.nq))
    dq[:, 0] = q  # radial: along q itself (off the sphere for the quaternions)
    dq[:, 1] = rng.standard_normal((B, flat.nq))
    _, dtau = emu_jvp(harness, flat, q, v, vd, None, dq.reshape(B, -1), None, None, None, ntan)
    got = dtau.reshape(B, ntan, flat.nv)
    for d in range(ntan):
        ref = quad_jvp(oracle, flat, q, v, vd, None, dq[:, d], None, None, None)
        assert np.abs(got[:, d] - ref).max() <= 1e-10 * (1 + np.abs(ref).max())
