"""Derivatives of simulate steps without a GPU (rbd_simulate_jvp, rbd_simulate_step_derivatives): the two entry points are declared and exported, and the
per-joint tangent of the integrator's stage map (csrc/rbd_tangent_mk.hpp tan_joint_local_rate / tan_joint_global), compiled as plain C++ for the host like
tests/test_derivatives_cpu.py does, matches a 4th-order central difference of oracle/simulate_np.py's local_rate / global_coordinates — every joint type,
quaternion directions off the unit sphere, and the points where the reference branches: q = q0, ϕ_rot = 0 with ϕ_trans ≠ 0, θ on either side of eps and of
the Bortz series threshold.  Every output must be finite."""
import ctypes
import os
import types

import numpy as np
import pytest

from host_harness import CLANG, ROOT, build

NEW = ("rbd_simulate_jvp", "rbd_simulate_step_derivatives")

HARNESS = r"""
#include <hip/hip_runtime.h>
#include "rbd_tangent_mk.hpp"
thread_local EmuDim3 threadIdx, blockIdx, blockDim, gridDim;
int emu_unreachable(const char*) { __builtin_trap(); return 0; }
template <typename T> using D = rbd::Dual<T, 1>;
template <typename T> void pack(int n, const double* x, const double* dx, D<T>* o) {
  for (int k = 0; k < n; ++k) { o[k] = D<T>(T(x[k])); o[k].d[0] = T(dx[k]); }
}
template <typename T> void unpack(int n, const D<T>* x, double* o, double* d) {
  for (int k = 0; k < n; ++k) { o[k] = x[k].v; d[k] = x[k].d[0]; }
}
// ϕ̇ of one joint and its derivative along (dq0, dq, dv)
template <typename T> void rate(int jt, const double* q0, const double* dq0, const double* q, const double* dq, const double* v, const double* dv, double* o, double* d) {
  D<T> a[7], b[7], c[6], r[6];
  pack(7, q0, dq0, a); pack(7, q, dq, b); pack(6, v, dv, c);
  rbd::tan_joint_local_rate(jt, a, b, c, r);
  unpack(6, r, o, d);
}
// global_coordinates! of one joint and its derivative along (dq0, dϕ)
template <typename T> void global(int jt, const double* q0, const double* dq0, const double* phi, const double* dphi, double* o, double* d) {
  D<T> a[7], b[6], r[7];
  pack(7, q0, dq0, a); pack(6, phi, dphi, b);
  rbd::tan_joint_global(jt, a, b, r);
  unpack(7, r, o, d);
}
extern "C" void emu_rate_f64(int jt, const double* q0, const double* dq0, const double* q, const double* dq, const double* v, const double* dv, double* o, double* d) { rate<double>(jt, q0, dq0, q, dq, v, dv, o, d); }
extern "C" void emu_rate_f32(int jt, const double* q0, const double* dq0, const double* q, const double* dq, const double* v, const double* dv, double* o, double* d) { rate<float>(jt, q0, dq0, q, dq, v, dv, o, d); }
extern "C" void emu_global_f64(int jt, const double* q0, const double* dq0, const double* phi, const double* dphi, double* o, double* d) { global<double>(jt, q0, dq0, phi, dphi, o, d); }
extern "C" void emu_global_f32(int jt, const double* q0, const double* dq0, const double* phi, const double* dphi, double* o, double* d) { global<float>(jt, q0, dq0, phi, dphi, o, d); }
"""

FIXED, REVOLUTE, PRISMATIC, FLOATING, PLANAR, SPHERICAL, SINCOS = range(7)
NQ = {REVOLUTE: 1, PRISMATIC: 1, FLOATING: 7, PLANAR: 3, SPHERICAL: 4, SINCOS: 2}
NV = {REVOLUTE: 1, PRISMATIC: 1, FLOATING: 6, PLANAR: 3, SPHERICAL: 3, SINCOS: 1}
EPS64 = np.finfo(np.float64).eps


def build_harness():
    return build(HARNESS, "rbd_tangent_mk_emu")


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang")
    return build_harness()


@pytest.fixture(scope="module")
def sim(oracle):
    import simulate_np
    return simulate_np


def one_joint(t):
    return types.SimpleNamespace(n_bodies=1, joint_type=np.array([t]), q_offset=np.array([0]), v_offset=np.array([0]), nq=NQ[t], nv=NV[t])


def pad(x, n):
    out = np.zeros(n)
    out[:len(x)] = x
    return out


P = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.c_void_p)


def emu_rate(lib, prec, t, q0, dq0, q, dq, v, dv):
    o, d = np.zeros(6), np.zeros(6)
    getattr(lib, "emu_rate_" + prec)(t, P(pad(q0, 7)), P(pad(dq0, 7)), P(pad(q, 7)), P(pad(dq, 7)), P(pad(v, 6)), P(pad(dv, 6)), P(o), P(d))
    return o[:NV[t]], d[:NV[t]]


def emu_global(lib, prec, t, q0, dq0, phi, dphi):
    o, d = np.zeros(7), np.zeros(7)
    getattr(lib, "emu_global_" + prec)(t, P(pad(q0, 7)), P(pad(dq0, 7)), P(pad(phi, 6)), P(pad(dphi, 6)), P(o), P(d))
    return o[:NQ[t]], d[:NQ[t]]


def cd(f, h=1e-3):
    return (8 * (f(h) - f(-h)) - (f(2 * h) - f(-2 * h))) / (12 * h)


def quat(rng):
    x = rng.standard_normal(4)
    return x / np.linalg.norm(x)


def q_of(t, rng):
    if t == FLOATING:
        return np.r_[quat(rng), rng.standard_normal(3)]
    if t == SPHERICAL:
        return quat(rng)
    if t == SINCOS:
        a = rng.standard_normal()
        return np.array([np.sin(a), np.cos(a)])
    return rng.standard_normal(NQ[t])


def q_near(sim, t, q0, rot, trans):
    """q0 moved by the local coordinates (rot, trans): global_coordinates with ϕ = (rot, trans) (rotation part of a quaternion joint, else the first
    coordinates)."""
    m = one_joint(t)
    if t == FLOATING:
        return sim.global_coordinates(m, q0, np.r_[rot, trans])
    if t == SPHERICAL:
        return sim.global_coordinates(m, q0, np.asarray(rot))
    return sim.global_coordinates(m, q0, np.r_[rot, trans][:NV[t]])


def check_rate(lib, sim, t, q0, q, v, rng, tol=1e-7, prec="f64", values=True):
    m = one_joint(t)
    for d in range(3):
        dq0 = rng.standard_normal(NQ[t])
        # direction 1 at q = q0: q and q0 moved together, the first stage of every step.  (Elsewhere a curve on which the relative rotation stays exactly
        # zero would sit in the reference's small-angle branch for every h, which drops ½ q_v × ω: the difference would be that of the branch.)
        dq = dq0.copy() if d == 1 and np.array_equal(q, q0) else rng.standard_normal(NQ[t])
        dv = rng.standard_normal(NV[t])
        val, got = emu_rate(lib, prec, t, q0, dq0, q, dq, v, dv)
        assert np.isfinite(val).all() and np.isfinite(got).all(), (t, val, got)
        ref = cd(lambda h: sim.local_rate(m, q0 + h * dq0, q + h * dq, v + h * dv))
        assert np.abs(got - ref).max() <= tol * (1 + np.abs(ref).max()), (t, prec, d, got, ref)
        if prec == "f64" and values:
            r0 = sim.local_rate(m, q0, q, v)
            assert np.abs(val - r0).max() <= 1e-9 * (1 + np.abs(r0).max())  # (the oracle's closed forms lose digits at small θ)


def check_global(lib, sim, t, q0, phi, rng, tol=1e-7, prec="f64", values=True):
    m = one_joint(t)
    for d in range(3):
        dq0 = rng.standard_normal(NQ[t])
        dphi = rng.standard_normal(NV[t])
        if d == 2 and t in (FLOATING, SPHERICAL):
            dphi[3:] = 0 if t == FLOATING else dphi[3:]
            dq0[:4] = q0[:4]  # (radially: off the unit sphere)
        val, got = emu_global(lib, prec, t, q0, dq0, phi, dphi)
        assert np.isfinite(val).all() and np.isfinite(got).all(), (t, val, got)
        ref = cd(lambda h: sim.global_coordinates(m, q0 + h * dq0, phi + h * dphi))
        assert np.abs(got - ref).max() <= tol * (1 + np.abs(ref).max()), (t, prec, d, got, ref)
        if prec == "f64" and values:
            g0 = sim.global_coordinates(m, q0, phi)
            assert np.abs(val - g0).max() <= 1e-9 * (1 + np.abs(g0).max())


def test_symbols_declared_and_exported(rbd):
    header = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in rbd._capi.SYMBOLS, name
    assert "#define RBD_HIP_H_VERSION 700" in header and rbd._capi.HEADER_VERSION == 700
    lib = ctypes.CDLL(rbd._capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    for name in ("simulate_jvp_", "simulate_step_derivatives_"):
        assert callable(getattr(rbd, name))


@pytest.mark.parametrize("t", [REVOLUTE, PRISMATIC, SINCOS, PLANAR, SPHERICAL, FLOATING])
def test_generic_points(harness, sim, t):
    rng = np.random.default_rng(100 + t)
    for _ in range(4):
        q0 = q_of(t, rng)
        q = q_near(sim, t, q0, 0.3 * rng.standard_normal(3), rng.standard_normal(3))
        v = rng.standard_normal(NV[t])
        check_rate(harness, sim, t, q0, q, v, rng)
        check_global(harness, sim, t, q0, 0.4 * rng.standard_normal(NV[t]), rng)


# the points where the reference branches: θ = 0 exactly, around eps, around the series threshold of 1e-2 (fp64)
THETAS = [0.0, 0.5 * EPS64, 2 * EPS64, 1e-9, 1e-2 * (1 - 1e-6), 1e-2 * (1 + 1e-6), 0.2]


@pytest.mark.parametrize("t", [SPHERICAL, FLOATING])
@pytest.mark.parametrize("theta", THETAS)
def test_special_points(harness, sim, t, theta):
    rng = np.random.default_rng(7)
    q0 = q_of(t, rng)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    trans = rng.standard_normal(3)  # (ϕ_rot = θ axis with ϕ_trans ≠ 0: θ = 0 is the case exp's branch gets wrong)
    v = rng.standard_normal(NV[t])
    q = q_near(sim, t, q0, theta * axis, trans)
    # (values: the oracle's closed forms lose up to all digits for 0 < θ < 1e-6, and at a few eps its branch flips with the rounding of θ itself)
    check_rate(harness, sim, t, q0, q, v, rng, values=not 0 < theta < 1e-6)
    if theta == 0:  # q = q0 itself, bit for bit: the first stage of every step
        check_rate(harness, sim, t, q0, q0.copy(), v, rng)
        vz = v.copy()
        vz[:3] = 0  # ω = 0 with a nonzero linear velocity
        check_rate(harness, sim, t, q0, q0.copy(), vz, rng)
    check_global(harness, sim, t, q0, np.r_[theta * axis, trans][:NV[t]], rng, values=not 0 < theta < 1e-6)


@pytest.mark.parametrize("t", [SPHERICAL, FLOATING])
@pytest.mark.parametrize("theta", [0.0, 1e-3, 0.5 * (1 - 1e-4), 0.5 * (1 + 1e-4), 1.0])
def test_special_points_fp32(harness, sim, t, theta):
    """The fp32 instantiation around its own series threshold (θ = 0.5): an fp32 tolerance."""
    rng = np.random.default_rng(8)
    q0 = q_of(t, rng)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    trans = rng.standard_normal(3)
    v = rng.standard_normal(NV[t])
    q = q_near(sim, t, q0, theta * axis, trans)
    check_rate(harness, sim, t, q0, q, v, rng, tol=2e-5, prec="f32")
    check_global(harness, sim, t, q0, np.r_[theta * axis, trans][:NV[t]], rng, tol=2e-5, prec="f32")
