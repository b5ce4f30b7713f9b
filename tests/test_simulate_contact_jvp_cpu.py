"""Forward mode through simulate steps with soft contact without a GPU (rbd_simulate_contact_jvp, rbd_simulate_contact_step_derivatives): the entry points
are declared, listed and exported; and the friction state's Runge–Kutta tableau on Duals (csrc/rbd_contact.hpp contact_stage_value<Dual<double, 2>>, what
tangent_contact_stage_kernel runs per value), compiled as plain C++ for the host as tests/test_simulate_contact_vjp_cpu.py does, against torch.func.jvp through
classical RK4 of the same right-hand side.  No difference quotients."""
import ctypes
import os

import numpy as np
import pytest
import torch

from host_harness import CLANG, ROOT, build
from test_contact_vjp_cpu import _p

NEW = ("rbd_simulate_contact_jvp", "rbd_simulate_contact_step_derivatives")

HARNESS = r"""
#include <hip/hip_runtime.h>
#include <cmath>
#include "rbd_contact.hpp"
thread_local EmuDim3 threadIdx, blockIdx, blockDim, gridDim;
int emu_unreachable(const char*) { __builtin_trap(); return 0; }
using namespace rbd;
using D = Dual<double, 2>;
// One RK4 step of ṡ = −k s + c sin(s) per value with two tangent directions, the four stages of contact_stage_value<D>; ṡ_k from the closed form on Duals at
// the stage state.  ds0, ds1: [value][direction].  The running sum is poisoned before stage 0, which must not read it.
extern "C" void emu_tableau_step(long n, const double* dt, const double* s0, const double* ds0, const double* k, const double* c, double* s1, double* ds1) {
  for (long i = 0; i < n; ++i) {
    D base(s0[i]), s, acc(std::nan(""));
    for (int j = 0; j < 2; ++j) { base.d[j] = ds0[2 * i + j]; acc.d[j] = std::nan(""); }
    s = base;
    for (int stage = 0; stage < 4; ++stage) {
      D sn, cs, sdot;
      sincos_t(s, &sn, &cs);
      sdot = (-k[i]) * s + c[i] * sn;
      contact_stage_value<D>(stage, dt[i], base, sdot, acc, s);
    }
    s1[i] = s.v;
    for (int j = 0; j < 2; ++j) ds1[2 * i + j] = s.d[j];
  }
}
"""


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang")
    return build(HARNESS, "rbd_simulate_contact_jvp_emu")


def test_symbols_declared_listed_and_exported(rbd):
    header = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    lib = ctypes.CDLL(rbd._capi.LIB_PATH)
    for name in NEW:
        assert name + "(" in header, name
        assert name in rbd._capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert callable(rbd.simulate_contact_jvp_) and callable(rbd.simulate_contact_step_derivatives_)


def test_tableau_on_duals_is_the_jvp_of_rk4(harness):
    """200 random (s₀, ds₀, k, c, dt): s⁺ and ds⁺ of the four stages of contact_stage_value<Dual<double, 2>> equal torch.func.jvp through classical RK4 of
    ṡ = −k·s + c·sin(s) in float64 at 1e-13·(1 + max|ref|); stage 0 does not read the running sum (the harness poisons it with NaN)."""
    rng = np.random.default_rng(41)
    n = 200
    s0, k, c = rng.standard_normal(n), rng.uniform(0.5, 50.0, n), 5.0 * rng.standard_normal(n)
    dt = 10.0 ** rng.uniform(-4, -1.5, n)
    ds0 = rng.standard_normal((n, 2))
    s1, ds1 = np.full(n, np.nan), np.full((n, 2), np.nan)
    harness.emu_tableau_step(ctypes.c_long(n), _p(dt), _p(s0), _p(ds0), _p(k), _p(c), _p(s1), _p(ds1))
    tk, tc, tdt = (torch.as_tensor(x) for x in (k, c, dt))

    def rk4(s):
        f = lambda x: -tk * x + tc * torch.sin(x)
        k1 = f(s)
        k2 = f(s + 0.5 * tdt * k1)
        k3 = f(s + 0.5 * tdt * k2)
        k4 = f(s + tdt * k3)
        return s + tdt * (k1 + 2 * k2 + 2 * k3 + k4) / 6

    for j in range(2):
        ref, dref = torch.func.jvp(rk4, (torch.as_tensor(s0),), (torch.as_tensor(np.ascontiguousarray(ds0[:, j])),))
        ref, dref = ref.numpy(), dref.numpy()
        assert np.isfinite(s1).all() and np.isfinite(ds1).all()
        assert np.abs(s1 - ref).max() <= 1e-13 * (1 + np.abs(ref).max())
        assert np.abs(ds1[:, j] - dref).max() <= 1e-13 * (1 + np.abs(dref).max()), j
