"""Reverse mode through soft contact without a GPU (rbd_contact_dynamics_vjp, rbd_dynamics_contact_vjp): the two calls are declared and exported; the pair
model and its hand-written pullback (csrc/rbd_contact.hpp contact_pair_force, contact_pair_adjoint), compiled as plain C++ for the host as
tests/test_point_kinematics_cpu.py does, against exact references — the torch fp64 model of tests/contact_model_ref.py (itself pinned to the oracle's
contact_dynamics!), torch.autograd of it, and J·d from the Dual<double, 1> instantiation of the forward routine.  No difference quotients."""
import ctypes
import os

import numpy as np
import pytest
import torch

import contact_model_ref as cm
from host_harness import CLANG, ROOT, build
from point_kinematics_ref import reference

NEW = ("rbd_contact_dynamics_vjp", "rbd_dynamics_contact_vjp")
N = 2000

HARNESS = r"""
#include <hip/hip_runtime.h>
#include "rbd_contact.hpp"
thread_local EmuDim3 threadIdx, blockIdx, blockDim, gridDim;
int emu_unreachable(const char*) { __builtin_trap(); return 0; }
using namespace rbd;
// per pair: pos, vel, x (3 each), c (CP_STRIDE), H (6)
extern "C" void emu_pair_force(long n, const double* pos, const double* vel, const double* x, const double* c, const double* H, int* inside, double* f,
                               double* xd) {
  for (long i = 0; i < n; ++i)
    inside[i] = contact_pair_force<double>(pos + 3 * i, vel + 3 * i, x + 3 * i, c + CP_STRIDE * i, H + 6 * i, f + 3 * i, xd + 3 * i);
}
extern "C" void emu_pair_adjoint(long n, const double* pos, const double* vel, const double* x, const double* c, const double* H, const double* fb,
                                 const double* tqb, const double* xdb, const double* xob, int* inside, double* pos_bar, double* vel_bar, double* x_bar) {
  for (long i = 0; i < n; ++i)
    inside[i] = contact_pair_adjoint<double>(pos + 3 * i, vel + 3 * i, x + 3 * i, c + CP_STRIDE * i, H + 6 * i, fb ? fb + 3 * i : nullptr, tqb ? tqb + 3 * i : nullptr,
                                             xdb ? xdb + 3 * i : nullptr, xob ? xob + 3 * i : nullptr, pos_bar + 3 * i, vel_bar + 3 * i, x_bar + 3 * i);
}
// the tangents of (f, pos × f, ẋ, x after the reset) along (dpos, dvel, dx): the Dual<double, 1> instantiation of the forward routine
extern "C" void emu_pair_jvp(long n, const double* pos, const double* vel, const double* x, const double* c, const double* H, const double* dpos,
                             const double* dvel, const double* dx, double* df, double* dtq, double* dxd, double* dxo) {
  using D = Dual<double, 1>;
  auto dual = [](double v, double d) { D y(v); y.d[0] = d; return y; };
  for (long i = 0; i < n; ++i) {
    D p[3], w[3], s[3], f[3], xd[3], tq[3];
    for (int k = 0; k < 3; ++k) { p[k] = dual(pos[3 * i + k], dpos[3 * i + k]); w[k] = dual(vel[3 * i + k], dvel[3 * i + k]); s[k] = dual(x[3 * i + k], dx[3 * i + k]); }
    const bool in = contact_pair_force<D>(p, w, s, c + CP_STRIDE * i, H + 6 * i, f, xd);
    cross3(p, f, tq);
    for (int k = 0; k < 3; ++k) { df[3 * i + k] = f[k].d[0]; dtq[3 * i + k] = tq[k].d[0]; dxd[3 * i + k] = xd[k].d[0]; dxo[3 * i + k] = in ? dx[3 * i + k] : 0.0; }
  }
}
"""


def build_harness():
    return build(HARNESS, "rbd_contact_emu")


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang")
    return build_harness()


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def random_pairs(seed=3):
    """N pairs over all four branches: random half-spaces, Hunt–Crossley exponents 1, 3/2 and 2, a quarter of the points outside, a share of the inside ones
    leaving fast enough for the normal force to clamp, and tangential speeds over three decades so that friction both sticks and slips."""
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((N, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    h = rng.standard_normal((N, 3))
    alpha = 0.1 + 0.4 * rng.random(N)
    hck = 2e3 * (1 + rng.random(N))
    par = np.stack([hck, 1.5 * alpha * hck, rng.choice([1.0, 1.5, 2.0], N), 0.3 + rng.random(N), 1e3 * (1 + rng.random(N)), 1e2 * (1 + rng.random(N))], axis=1)
    sep = np.where(rng.random(N) < 0.25, 1e-3 + 0.1 * rng.random(N), -(1e-3 + 0.05 * rng.random(N)))
    t = rng.standard_normal((N, 3))
    t -= (t * n).sum(axis=1, keepdims=True) * n
    pos = h + sep[:, None] * n + t
    vn = np.where(rng.random(N) < 0.3, (0.5 + 1.5 * rng.random(N)) / (1.5 * alpha), 0.3 * rng.standard_normal(N))  # clamps where vel·n > k / λ
    w = rng.standard_normal((N, 3))
    w -= (w * n).sum(axis=1, keepdims=True) * n
    vel = vn[:, None] * n + (10.0 ** rng.uniform(-3, 0, N))[:, None] * w
    x = 1e-3 * rng.standard_normal((N, 3))
    c = np.ascontiguousarray(np.concatenate([np.zeros((N, 3)), par], axis=1))  # CP_STRIDE: the location (unused by the pair routines), then the parameters
    H = np.ascontiguousarray(np.concatenate([h, n], axis=1))
    return pos, vel, x, par, c, H, rng


@pytest.fixture(scope="module")
def pairs():
    pos, vel, x, par, c, H, rng = random_pairs()
    T = lambda a: torch.as_tensor(a, dtype=torch.float64)
    tp, tv, tx = (T(a).requires_grad_(True) for a in (pos, vel, x))
    f, xd, x_out, info = cm.pair_model(tp, tv, tx, T(par), T(H[:, :3]), T(H[:, 3:]))
    return dict(pos=pos, vel=vel, x=x, c=c, H=H, rng=rng, t=(tp, tv, tx), f=f, xd=xd, x_out=x_out, info=info)


def test_symbols_declared_and_exported(rbd):
    header = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in rbd._capi.SYMBOLS, name
    lib = ctypes.CDLL(rbd._capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name


def test_random_pairs_cover_every_branch_with_margins(pairs):
    """At least 5 % of the pairs on each of outside / clamped / stick / slip, and EVERY pair clear of the branch boundaries (a condition on the inputs)."""
    cov = cm.coverage(pairs["info"])
    assert min(cov) >= 0.05, dict(zip(cm.BRANCHES, cov))
    assert bool(cm.margins_ok(pairs["info"]).all())


def test_torch_model_against_the_oracle(rbd, oracle):
    """The helper's own pin: contact wrenches, ṡ and the reset s of oracle.contact_dynamics on the walker states of test_contact.py at 1e-12·(1 + max|ref|),
    from the contact points' positions and velocities formed from the oracle's per-body kinematics."""
    rng = np.random.default_rng(5)
    flat = rbd.flatten(cm.walker(rbd, rng))
    B = 130
    q, v = rbd.rand_configuration(flat, B, rng), rbd.rand_velocity(flat, B, rng)
    q[:, 4:7] *= 0.5
    s = 1e-3 * rng.standard_normal((B, flat.ns))
    s_ref, sd_ref, cw_ref = oracle.contact_dynamics(flat, q, v, s)
    bodies = [c["body"] for c in flat.contact_points]
    pos, vel, _, _ = reference(oracle, flat, q, v, None, bodies, [c["location"] for c in flat.contact_points], jac=False)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)
    cw, sd, s_out, info = cm.contact_model(flat, T(pos.reshape(B, -1)), T(vel.reshape(B, -1)), T(s))
    inside = info["inside"].numpy()
    assert inside.any() and not inside.all()
    for what, got, ref in (("contactwrenches", cw, cw_ref), ("sdot", sd, sd_ref), ("s", s_out, s_ref)):
        err = np.abs(got.numpy() - ref).max()
        assert err <= 1e-12 * (1 + np.abs(ref).max()), (what, err)


def test_pair_force_equals_the_torch_model(harness, pairs):
    """contact_pair_force<double> — f, ẋ and the inside flag — against the torch model at 1e-13·(1 + max|ref|)."""
    pos, vel, x, c, H = (pairs[k] for k in ("pos", "vel", "x", "c", "H"))
    inside, f, xd = np.full(N, -1, dtype=np.int32), np.full((N, 3), np.nan), np.full((N, 3), np.nan)
    harness.emu_pair_force(ctypes.c_long(N), _p(pos), _p(vel), _p(x), _p(c), _p(H), _p(inside), _p(f), _p(xd))
    assert np.array_equal(inside.astype(bool), pairs["info"]["inside"].numpy())
    for what, got, ref in (("f", f, pairs["f"]), ("xd", xd, pairs["xd"])):
        ref = ref.detach().numpy()
        assert np.abs(got - ref).max() <= 1e-13 * (1 + np.abs(ref).max()), (what, np.abs(got - ref).max())


def adjoint(harness, pairs, fb, tqb, xdb, xob):
    pos, vel, x, c, H = (pairs[k] for k in ("pos", "vel", "x", "c", "H"))
    inside = np.full(N, -1, dtype=np.int32)
    pb, vb, xb = np.full((N, 3), np.nan), np.full((N, 3), np.nan), np.full((N, 3), np.nan)
    harness.emu_pair_adjoint(ctypes.c_long(N), _p(pos), _p(vel), _p(x), _p(c), _p(H), _p(fb), _p(tqb), _p(xdb), _p(xob), _p(inside), _p(pb), _p(vb), _p(xb))
    return inside.astype(bool), pb, vb, xb


def test_adjoint_is_the_transpose_of_the_dual_forward(harness, pairs):
    """⟨f̄, df⟩ + ⟨τ̄q, d(pos × f)⟩ + ⟨ẋ̄, dẋ⟩ + ⟨x̄_out, dx_out⟩ = ⟨pos_bar, dpos⟩ + ⟨vel_bar, dvel⟩ + ⟨x̄, dx⟩ per pair to 1e-12 of the summed magnitudes, with
    the tangents from contact_pair_force<Dual<double, 1>>; every cotangent alone (the others NULL) too."""
    pos, vel, x, c, H, rng = (pairs[k] for k in ("pos", "vel", "x", "c", "H", "rng"))
    bars = [rng.standard_normal((N, 3)) for _ in range(4)]
    for use in ((1, 1, 1, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):
        cot = [b if u else None for b, u in zip(bars, use)]
        _, pb, vb, xb = adjoint(harness, pairs, *cot)
        assert np.isfinite(pb).all() and np.isfinite(vb).all() and np.isfinite(xb).all()
        for trial in range(2):
            dpos, dvel, dx = (rng.standard_normal((N, 3)) for _ in range(3))
            outs = [np.full((N, 3), np.nan) for _ in range(4)]
            harness.emu_pair_jvp(ctypes.c_long(N), _p(pos), _p(vel), _p(x), _p(c), _p(H), _p(dpos), _p(dvel), _p(dx), *[_p(o) for o in outs])
            assert all(np.isfinite(o).all() for o in outs)
            left = [b * o for b, o in zip(cot, outs) if b is not None]
            right = [pb * dpos, vb * dvel, xb * dx]
            lhs, rhs = sum(t.sum(axis=1) for t in left), sum(t.sum(axis=1) for t in right)
            mag = sum(np.abs(t).sum(axis=1) for t in left + right) + 1e-300
            assert (np.abs(lhs - rhs) <= 1e-12 * mag).all(), (use, trial, (np.abs(lhs - rhs) / mag).max())


def test_adjoint_equals_torch_autograd(harness, pairs):
    """(pos_bar, vel_bar, x̄) against torch.autograd of the helper at 1e-11·(1 + max|ref|), the wrench's torque part (pos × f) included."""
    rng = pairs["rng"]
    fb, tqb, xdb, xob = (rng.standard_normal((N, 3)) for _ in range(4))
    _, pb, vb, xb = adjoint(harness, pairs, fb, tqb, xdb, xob)
    tp, tv, tx = pairs["t"]
    T = lambda a: torch.as_tensor(a, dtype=torch.float64)
    loss = (pairs["f"] * T(fb)).sum() + (torch.linalg.cross(tp, pairs["f"]) * T(tqb)).sum() + (pairs["xd"] * T(xdb)).sum() + (pairs["x_out"] * T(xob)).sum()
    ref = torch.autograd.grad(loss, (tp, tv, tx), retain_graph=True)
    for what, got, r in zip(("pos_bar", "vel_bar", "x_bar"), (pb, vb, xb), ref):
        r = r.numpy()
        assert np.isfinite(r).all()
        assert np.abs(got - r).max() <= 1e-11 * (1 + np.abs(r).max()), (what, np.abs(got - r).max())


def test_outside_pairs_return_exact_zeros(harness, pairs):
    rng = pairs["rng"]
    inside, pb, vb, xb = adjoint(harness, pairs, *(rng.standard_normal((N, 3)) for _ in range(4)))
    out = ~pairs["info"]["inside"].numpy()
    assert np.array_equal(inside, ~out) and out.sum() >= 0.05 * N
    assert (pb[out] == 0).all() and (vb[out] == 0).all() and (xb[out] == 0).all()
    assert (np.abs(xb[~out]).sum(axis=1) > 0).all()  # (inside, x̄_out passes through)
