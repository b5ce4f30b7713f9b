"""Forward mode through soft contact without a GPU (rbd_contact_dynamics_jvp, rbd_dynamics_contact_jvp, rbd_dynamics_contact_derivatives): the three calls are
declared and exported; the per-state contact step of the tangent pass (csrc/rbd_contact.hpp contact_point_step), compiled as plain C++ for the host on
Dual<double, 2>, against torch.func.jvp of a torch restatement (pos = R r + p, vel = ω × pos + v, contact_model_ref.pair_model, (pos × f; f)) on the 2000
random pairs of test_contact_vjp_cpu.py; the Python mirrors' argument checks.  No difference quotients."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import contact_model_ref as cm
from host_harness import CLANG, ROOT, build
from test_contact_vjp_cpu import N, random_pairs

NEW = ("rbd_contact_dynamics_jvp", "rbd_dynamics_contact_jvp", "rbd_dynamics_contact_derivatives")
ND = 2  # tangent sets per pair: Dual<double, 2>

HARNESS = r"""
#include <hip/hip_runtime.h>
#include "rbd_contact.hpp"
thread_local EmuDim3 threadIdx, blockIdx, blockDim, gridDim;
int emu_unreachable(const char*) { __builtin_trap(); return 0; }
using namespace rbd;
// per pair: K (18: R row-major, p, twist), x (3), c (CP_STRIDE, the location included), H (6); tangents dK (2 x 18), dx (2 x 3), direction-major per pair.
// out: the wrench (6), ẋ and x after the reset (3 each) and their two tangents each
extern "C" void emu_point_step_jvp(long n, const double* K, const double* x, const double* c, const double* H, const double* dK, const double* dx, int* inside,
                                   double* w, double* xd, double* xo, double* dw, double* dxd, double* dxo) {
  using D = Dual<double, 2>;
  for (long i = 0; i < n; ++i) {
    D Kd[18], wd[6];
    for (int k = 0; k < 18; ++k) { Kd[k].v = K[18 * i + k]; for (int j = 0; j < 2; ++j) Kd[k].d[j] = dK[(2 * i + j) * 18 + k]; }
    contact_point_step<D>(
        Kd, c + CP_STRIDE * i, H + 6 * i, 1,
        [&](int, D* s) {
          for (int k = 0; k < 3; ++k) { s[k].v = x[3 * i + k]; for (int j = 0; j < 2; ++j) s[k].d[j] = dx[(2 * i + j) * 3 + k]; }
        },
        [&](int, bool in, const D* sd, const D* so) {
          inside[i] = in;
          for (int k = 0; k < 3; ++k) {
            xd[3 * i + k] = sd[k].v; xo[3 * i + k] = so[k].v;
            for (int j = 0; j < 2; ++j) { dxd[(2 * i + j) * 3 + k] = sd[k].d[j]; dxo[(2 * i + j) * 3 + k] = so[k].d[j]; }
          }
        },
        wd);
    for (int k = 0; k < 6; ++k) { w[6 * i + k] = wd[k].v; for (int j = 0; j < 2; ++j) dw[(2 * i + j) * 6 + k] = wd[k].d[j]; }
  }
}
"""


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang")
    return build(HARNESS, "rbd_contact_jvp_emu")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_declared_and_exported(rbd):
    header = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in rbd._capi.SYMBOLS, name
    lib = ctypes.CDLL(rbd._capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name


@pytest.fixture(scope="module")
def bodies():
    """The pairs of random_pairs, each on a random body: a random rotation R and point r with p = pos − R r, a random ω with v = vel − ω × pos — the contact
    point's position and velocity are the pair's own —, two random tangent sets of K and of x."""
    pos, vel, x, par, c, H, rng = random_pairs()
    Q, _ = np.linalg.qr(rng.standard_normal((N, 3, 3)))
    r = 0.3 * rng.standard_normal((N, 3))
    om = rng.standard_normal((N, 3))
    p = pos - np.einsum("nij,nj->ni", Q, r)
    lin = vel - np.cross(om, pos)
    K = np.ascontiguousarray(np.concatenate([Q.reshape(N, 9), p, om, lin], axis=1))
    cc = c.copy()
    cc[:, :3] = r
    dK, dx = rng.standard_normal((N, ND, 18)), 1e-3 * rng.standard_normal((N, ND, 3))
    return dict(K=K, x=x, c=np.ascontiguousarray(cc), H=H, par=par, r=r, dK=dK, dx=dx)


def torch_step(K, x, r, par, h, n):
    """The restatement: (w, ẋ, x_out) of one point against one half-space from its body's K."""
    R, p, om, lin = K[:, :9].reshape(-1, 3, 3), K[:, 9:12], K[:, 12:15], K[:, 15:18]
    pos = torch.einsum("nij,nj->ni", R, r) + p
    vel = torch.linalg.cross(om, pos) + lin
    f, xd, x_out, info = cm.pair_model(pos, vel, x, par, h, n)
    return torch.cat([torch.linalg.cross(pos, f), f], dim=1), xd, x_out, info


def test_point_step_jvp_equals_torch_jvp(harness, bodies):
    """Values, and the tangents of the wrench, ẋ and x_out for both tangent sets, at 1e-13·(1 + max|ref|) (the bound of test_pair_force_equals_the_torch_model);
    outside pairs give exact zeros."""
    b = bodies
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)
    args = (T(b["r"]), T(b["par"]), T(b["H"][:, :3]), T(b["H"][:, 3:]))
    inside = np.full(N, -1, dtype=np.int32)
    w, xd, xo = np.full((N, 6), np.nan), np.full((N, 3), np.nan), np.full((N, 3), np.nan)
    dw, dxd, dxo = np.full((N, ND, 6), np.nan), np.full((N, ND, 3), np.nan), np.full((N, ND, 3), np.nan)
    harness.emu_point_step_jvp(ctypes.c_long(N), _p(b["K"]), _p(b["x"]), _p(b["c"]), _p(b["H"]), _p(b["dK"]), _p(b["dx"]), _p(inside), _p(w), _p(xd), _p(xo),
                               _p(dw), _p(dxd), _p(dxo))
    fn = lambda K, x: torch_step(K, x, *args)[:3]
    info = torch_step(T(b["K"]), T(b["x"]), *args)[3]
    assert np.array_equal(inside.astype(bool), info["inside"].numpy())
    assert min(cm.coverage(info)) >= 0.05 and bool(cm.margins_ok(info).all())
    out = ~info["inside"].numpy()
    for j in range(ND):
        vals, tans = torch.func.jvp(fn, (T(b["K"]), T(b["x"])), (T(b["dK"][:, j]), T(b["dx"][:, j])))
        for what, got, ref in (("w", w, vals[0]), ("xd", xd, vals[1]), ("x_out", xo, vals[2]), ("dw", dw[:, j], tans[0]), ("dxd", dxd[:, j], tans[1]),
                               ("dx_out", dxo[:, j], tans[2])):
            ref = ref.numpy()
            err = np.abs(got - ref).max()
            print("set %d %-6s max|err| %.3e  max|ref| %.3e" % (j, what, err, np.abs(ref).max()))
            assert np.isfinite(got).all() and np.isfinite(ref).all(), what
            assert err <= 1e-13 * (1 + np.abs(ref).max()), (j, what, err)
            assert (got[out] == 0).all(), (j, what)
    assert (np.abs(dxo[~out]).sum(axis=(1, 2)) > 0).all()  # (inside, dx passes through)


class _NoWorkspace:
    def __getattr__(self, name):
        raise AssertionError("the library was reached: " + name)


def test_python_mirrors_check_their_arguments(rbd):
    """Wrong shapes and a missing q, v or s are refused by the mirrors themselves: the stand-in state's workspace fails the test when touched."""
    from rigidbodydynamics_jl_amd import state as S
    flat = types.SimpleNamespace(nq=5, nv=4, ns=6, n_bodies=3)
    B = 3
    z = lambda n: torch.zeros(B, n, dtype=torch.float64)
    st = types.SimpleNamespace(flat=flat, batch=B, layout="aos", dtype=torch.float64, q=z(5), v=z(4), s=z(6), ws=_NoWorkspace())

    def check(t, n, what):  # MechanismState._check itself; only its refusal of a tensor that is not on the GPU (the stand-ins here) is let through
        try:
            S.MechanismState._check(st, t, n, what)
        except S.DimensionMismatch:
            raise
        except ValueError as e:
            assert "CUDA" in str(e)
    st._check = check
    calls = (lambda **kw: S.contact_dynamics_jvp_(st, 2, **kw), lambda **kw: S.dynamics_contact_jvp_(st, 2, **kw),
             lambda **kw: S.dynamics_contact_derivatives_(st, **kw))
    for call in calls:
        for name in ("q", "v", "s"):
            with pytest.raises(S.DimensionMismatch):
                call(**{name: z(7)})
            old = getattr(st, name)
            setattr(st, name, None)
            with pytest.raises(ValueError):
                call()
            setattr(st, name, old)
    for call in calls[:2]:
        for name, n in (("dq", 5), ("dv", 4), ("ds", 6), ("dsd", 6), ("ds_out", 6)):
            with pytest.raises(S.DimensionMismatch):
                call(**{name: z(n)})  # (one direction's width, not ntan = 2)
    with pytest.raises(S.DimensionMismatch):
        S.contact_dynamics_jvp_(st, 2, dcw=z(18))
    with pytest.raises(S.DimensionMismatch):
        S.dynamics_contact_jvp_(st, 2, dvd=z(4))
    with pytest.raises(ValueError):
        S.dynamics_contact_jvp_(st, 0)
    for name, n in (("dvd_dq", 4 * 4), ("dvd_ds", 4 * 5), ("dsd_dq", 6 * 6), ("dsd_ds", 6 * 5), ("dvd_dtau", 4 * 5), ("torques", 5), ("sdout", 4)):
        with pytest.raises(S.DimensionMismatch):
            S.dynamics_contact_derivatives_(st, **{name: z(n)})
