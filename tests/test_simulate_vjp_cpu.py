"""Reverse mode through simulate steps without a GPU (rbd_simulate_vjp): the entry point is declared and exported, and the per-joint pullback of the
integrator's stage map (csrc/rbd_adjoint_mk.hpp adj_mk_stage_joint), compiled as plain C++ for the host beside tan_mk_stage_joint (as
tests/test_simulate_derivatives_cpu.py does), is its exact transpose: ⟨ȳ, J d⟩ = ⟨Jᵀȳ, d⟩ for every joint type, all four stages, random cotangents and
directions (quaternion directions off the unit sphere), at the points where the reference branches (q = q0; ϕ_rot = 0 with ϕ_trans ≠ 0; θ on either side
of eps and of the series threshold), in fp64 and fp32, for both kernel instantiations (the 1-coordinate class without Duals, and the generic one).  The
pullback ADDS to the inputs' cotangents, and the value stage map of the reverse pass computes tan_mk_stage_joint's values.  Every output must be finite."""
import ctypes
import os

import numpy as np
import pytest

from host_harness import CLANG, ROOT, build

# inputs x (44): q0 7, v0 6, qs 7, vs 6, v̇ 6, the sums in 6 + 6; outputs y (25): q_n 7, v_n 6, the sums out 6 + 6 (each block zero past the joint's size)
HARNESS = r"""
#include <hip/hip_runtime.h>
#include "rbd_adjoint_mk.hpp"
thread_local EmuDim3 threadIdx, blockIdx, blockDim, gridDim;
int emu_unreachable(const char*) { __builtin_trap(); return 0; }
template <typename T> void jvp(int jt, int stage, double dt, const double* x, const double* dx, double* y, double* dy) {
  using D = rbd::Dual<T, 1>;
  D in[44], qn[7], vn[6];
  for (int k = 0; k < 44; ++k) { in[k] = D(T(x[k])); in[k].d[0] = T(dx[k]); }
  rbd::tan_mk_stage_joint<T, 1>(jt, stage, T(dt), in, in + 7, in + 13, in + 20, in + 26, in + 32, in + 38, qn, vn);
  for (int k = 0; k < 7; ++k) { y[k] = qn[k].v; dy[k] = qn[k].d[0]; }
  for (int k = 0; k < 6; ++k) {
    y[7 + k] = vn[k].v; dy[7 + k] = vn[k].d[0];
    y[13 + k] = in[32 + k].v; dy[13 + k] = in[32 + k].d[0];
    y[19 + k] = in[38 + k].v; dy[19 + k] = in[38 + k].d[0];
  }
}
// xb: added to (q0, v0, qs, vs, v̇), overwritten with the sums' cotangents in
template <typename T, bool WIDE> void vjp(int jt, int stage, double dt, const double* x, const double* yb, double* xb) {
  T v[44], b[44], y[25];
  for (int k = 0; k < 44; ++k) { v[k] = T(x[k]); b[k] = T(xb[k]); }
  for (int k = 0; k < 25; ++k) y[k] = T(yb[k]);
  for (int k = 0; k < 6; ++k) { b[32 + k] = y[13 + k]; b[38 + k] = y[19 + k]; }
  rbd::adj_mk_stage_joint<T, WIDE>(jt, stage, T(dt), v, v + 13, v + 20, v + 32, y, y + 7, b + 32, b + 38, b, b + 7, b + 13, b + 20, b + 26);
  for (int k = 0; k < 44; ++k) xb[k] = b[k];
}
template <typename T, bool WIDE> void value(int jt, int stage, double dt, const double* x, double* y) {
  T v[44], qn[7], vn[6];
  for (int k = 0; k < 44; ++k) v[k] = T(x[k]);
  for (int k = 0; k < 7; ++k) qn[k] = T(0);
  for (int k = 0; k < 6; ++k) vn[k] = T(0);
  rbd::mk_stage_value_joint<T, WIDE>(jt, stage, T(dt), v, v + 7, v + 13, v + 20, v + 26, v + 32, v + 38, qn, vn);
  for (int k = 0; k < 7; ++k) y[k] = qn[k];
  for (int k = 0; k < 6; ++k) { y[7 + k] = vn[k]; y[13 + k] = v[32 + k]; y[19 + k] = v[38 + k]; }
}
extern "C" void emu_jvp_f64(int jt, int s, double dt, const double* x, const double* dx, double* y, double* dy) { jvp<double>(jt, s, dt, x, dx, y, dy); }
extern "C" void emu_jvp_f32(int jt, int s, double dt, const double* x, const double* dx, double* y, double* dy) { jvp<float>(jt, s, dt, x, dx, y, dy); }
extern "C" void emu_vjp_f64(int jt, int s, double dt, const double* x, const double* yb, double* xb) { vjp<double, true>(jt, s, dt, x, yb, xb); }
extern "C" void emu_vjp_f32(int jt, int s, double dt, const double* x, const double* yb, double* xb) { vjp<float, true>(jt, s, dt, x, yb, xb); }
extern "C" void emu_vjp_narrow_f64(int jt, int s, double dt, const double* x, const double* yb, double* xb) { vjp<double, false>(jt, s, dt, x, yb, xb); }
extern "C" void emu_vjp_narrow_f32(int jt, int s, double dt, const double* x, const double* yb, double* xb) { vjp<float, false>(jt, s, dt, x, yb, xb); }
extern "C" void emu_value_f64(int jt, int s, double dt, const double* x, double* y) { value<double, true>(jt, s, dt, x, y); }
extern "C" void emu_value_narrow_f64(int jt, int s, double dt, const double* x, double* y) { value<double, false>(jt, s, dt, x, y); }
"""

FIXED, REVOLUTE, PRISMATIC, FLOATING, PLANAR, SPHERICAL, SINCOS = range(7)
NQ = {REVOLUTE: 1, PRISMATIC: 1, FLOATING: 7, PLANAR: 3, SPHERICAL: 4, SINCOS: 2}
NV = {REVOLUTE: 1, PRISMATIC: 1, FLOATING: 6, PLANAR: 3, SPHERICAL: 3, SINCOS: 1}
NARROW = (REVOLUTE, PRISMATIC, SINCOS)
ALL = (REVOLUTE, PRISMATIC, SINCOS, PLANAR, SPHERICAL, FLOATING)
EPS64 = np.finfo(np.float64).eps
DT = 5e-3
X_BLOCKS = [(0, "q"), (7, "v"), (13, "q"), (20, "v"), (26, "v"), (32, "v"), (38, "v")]
Y_BLOCKS = [(0, "q"), (7, "v"), (13, "v"), (19, "v")]


def build_harness():
    return build(HARNESS, "rbd_adjoint_mk_emu")


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang")
    return build_harness()


P = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.c_void_p)


def mask(t, blocks, n):
    m = np.zeros(n)
    for off, kind in blocks:
        m[off:off + (NQ[t] if kind == "q" else NV[t])] = 1
    return m


def quat_of(r):
    th = np.linalg.norm(r)
    return np.r_[np.cos(th / 2), (np.sin(th / 2) / th if th > 0 else 0.5) * r]


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])


def point(t, rng, rot=None, trans=None, omega_zero=False, same=False):
    """inputs x: a random base point, the stage state q0 moved by the rotation `rot` (and translation `trans`), velocities, v̇, sums"""
    x = rng.standard_normal(44) * mask(t, X_BLOCKS, 44)
    if t in (FLOATING, SPHERICAL):
        q0 = rng.standard_normal(4)
        q0 /= np.linalg.norm(q0)
        x[0:4] = q0
        r = 0.3 * rng.standard_normal(3) if rot is None else np.asarray(rot, dtype=float)
        x[13:17] = q0 if same else qmul(q0, quat_of(r))
        if t == FLOATING and same:
            x[17:20] = x[4:7]
        elif t == FLOATING and trans is not None:
            x[17:20] = x[4:7] + trans
    elif t == SINCOS:
        a, b = rng.standard_normal(2)
        x[0:2] = np.sin(a), np.cos(a)
        x[13:15] = (x[0:2] if same else np.array([np.sin(b), np.cos(b)]))
    elif same:
        x[13:13 + NQ[t]] = x[0:NQ[t]]
    if omega_zero:
        x[20:23] = 0
    return x


def dot_identity(lib, t, stage, x, rng, prec="f64", narrow=False, radial=False):
    mx, my = mask(t, X_BLOCKS, 44), mask(t, Y_BLOCKS, 25)
    if stage == 0:
        mx[32:44] = 0  # (no sums in)
    if stage == 3:
        my[13:25] = 0  # (no sums out)
    d = rng.standard_normal(44) * mx
    if radial and t in (FLOATING, SPHERICAL):  # (q0 and qs moved along themselves: off the unit sphere)
        d[0:4], d[13:17] = x[0:4], x[13:17]
    yb = rng.standard_normal(25) * my
    y, dy = np.zeros(25), np.zeros(25)
    getattr(lib, "emu_jvp_" + prec)(t, stage, ctypes.c_double(DT), P(x), P(d), P(y), P(dy))
    xb0 = rng.standard_normal(44) * mx  # (the pullback ADDS to (q0, v0, qs, vs, v̇): start from nonzero cotangents)
    xb = xb0.copy()
    getattr(lib, ("emu_vjp_narrow_" if narrow else "emu_vjp_") + prec)(t, stage, ctypes.c_double(DT), P(x), P(yb), P(xb))
    assert np.isfinite(y).all() and np.isfinite(dy).all() and np.isfinite(xb).all(), (t, stage)
    g = xb - np.r_[xb0[:32], np.zeros(12)]
    lhs, rhs = yb @ dy, g @ d
    scale = np.abs(yb * dy).sum() + np.abs(g * d).sum()
    tol = 1e-12 if prec == "f64" else 2e-5
    assert abs(lhs - rhs) <= tol * scale, (t, stage, prec, lhs, rhs, scale)
    assert scale > 0


def test_symbol_declared_and_exported(rbd):
    header = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    assert "rbd_simulate_vjp(" in header
    assert "rbd_simulate_vjp" in rbd._capi.SYMBOLS
    assert "#define RBD_HIP_H_VERSION 700" in header and rbd._capi.HEADER_VERSION == 700
    assert hasattr(ctypes.CDLL(rbd._capi.LIB_PATH), "rbd_simulate_vjp")
    assert callable(rbd.simulate_vjp_)
    from rbd_amd import autograd
    assert callable(autograd.simulate)


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
@pytest.mark.parametrize("t", ALL)
def test_generic_points(harness, t, stage):
    rng = np.random.default_rng(10 * t + stage)
    for i in range(4):
        x = point(t, rng)
        dot_identity(harness, t, stage, x, rng, radial=i == 3)
        dot_identity(harness, t, stage, x, rng, prec="f32")
        if t in NARROW:
            dot_identity(harness, t, stage, x, rng, narrow=True)
            dot_identity(harness, t, stage, x, rng, prec="f32", narrow=True)


# the points where the reference branches: θ = 0 exactly, around eps, around the series threshold of 1e-2 (fp64)
THETAS = [0.0, 0.5 * EPS64, 2 * EPS64, 1e-9, 1e-2 * (1 - 1e-6), 1e-2 * (1 + 1e-6), 0.2]


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
@pytest.mark.parametrize("t", [SPHERICAL, FLOATING])
@pytest.mark.parametrize("theta", THETAS)
def test_special_points(harness, t, stage, theta):
    rng = np.random.default_rng(7)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    trans = rng.standard_normal(3)
    # log's θ: the relative rotation of the stage state
    dot_identity(harness, t, stage, point(t, rng, rot=theta * axis, trans=trans), rng)
    # exp's θ: ϕ_rot of the stage map (stages 0-2: dt a ϕ̇ — q = q0 with ω set; stage 3: the sums in, chosen so that ϕ_rot = θ axis)
    x = point(t, rng, same=True, omega_zero=theta == 0)
    if theta > 0:
        x[20:23] = theta * axis / (DT * (1.0 if stage == 2 else 0.5))
    if stage == 3:
        x[20:23] = 0
        x[32:35] = theta * axis
    dot_identity(harness, t, stage, x, rng)
    if theta == 0:  # q = q0 bit for bit with ω = 0 and a linear velocity: ϕ_rot = 0, ϕ_trans ≠ 0
        x = point(t, rng, same=True, omega_zero=True)
        dot_identity(harness, t, stage, x, rng)
        dot_identity(harness, t, stage, x, rng, radial=True)


@pytest.mark.parametrize("stage", [0, 3])
@pytest.mark.parametrize("t", [SPHERICAL, FLOATING])
@pytest.mark.parametrize("theta", [0.0, 1e-3, 0.5 * (1 - 1e-4), 0.5 * (1 + 1e-4), 1.0])
def test_special_points_fp32(harness, t, stage, theta):
    """The fp32 instantiation around its own series threshold (θ = 0.5)."""
    rng = np.random.default_rng(8)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    dot_identity(harness, t, stage, point(t, rng, rot=theta * axis, trans=rng.standard_normal(3)), rng, prec="f32")
    x = point(t, rng, same=True, omega_zero=True)
    x[32:35] = theta * axis if stage == 3 else 0
    dot_identity(harness, t, stage, x, rng, prec="f32")


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
@pytest.mark.parametrize("t", ALL)
def test_value_map_equals_the_tangent_values(harness, t, stage):
    """The reverse pass's value stage map (both instantiations where they apply) computes tan_mk_stage_joint's values."""
    rng = np.random.default_rng(50 + 10 * t + stage)
    for _ in range(3):
        x = point(t, rng)
        if stage == 0:
            x[32:44] = 0
        y, dy, got = np.zeros(25), np.zeros(25), np.zeros(25)
        harness.emu_jvp_f64(t, stage, ctypes.c_double(DT), P(x), P(np.zeros(44)), P(y), P(dy))
        fns = ["emu_value_f64"] + (["emu_value_narrow_f64"] if t in NARROW else [])
        for fn in fns:
            getattr(harness, fn)(t, stage, ctypes.c_double(DT), P(x), P(got))
            m = mask(t, Y_BLOCKS, 25)
            if stage == 3:
                m[13:25] = 0
            assert np.isfinite(got).all()
            assert np.abs((got - y) * m).max() <= 4 * EPS64 * (1 + np.abs(y).max()), (fn, t, stage)
