"""Reverse mode through simulate steps with soft contact without a GPU (rbd_simulate_contact_vjp): the entry point is declared and exported; the friction
state's Runge–Kutta tableau in value form and its pullback (csrc/rbd_contact.hpp contact_stage_value, contact_stage_adjoint), compiled as plain C++ for the
host as tests/test_contact_vjp_cpu.py does, against J·d of the value form's Dual<double, 1> instantiation — stage by stage, and chained with the pair model
through a whole RK4 step; and the torch step of tests/simulate_contact_ref.py, the reference of the GPU tests, against oracle/simulate_np.py.  No difference
quotients."""
import ctypes
import os

import numpy as np
import pytest
import torch

import contact_model_ref as cm
import simulate_contact_ref as sr
from host_harness import CLANG, ROOT, build
from test_contact_vjp_cpu import N, _p, random_pairs

NEW = ("rbd_simulate_contact_vjp",)
DT = 1e-3

HARNESS = r"""
#include <hip/hip_runtime.h>
#include "rbd_contact.hpp"
thread_local EmuDim3 threadIdx, blockIdx, blockDim, gridDim;
int emu_unreachable(const char*) { __builtin_trap(); return 0; }
using namespace rbd;
using D = Dual<double, 1>;
static D dual(double v, double d) { D y(v); y.d[0] = d; return y; }
// one stage of the tableau per value: (s0, ṡ, the sum in) and their tangents -> the stage's output and the sum out with theirs (the Dual instantiation)
extern "C" void emu_stage_jvp(long n, int stage, double dt, const double* s0, const double* sd, const double* acc, const double* ds0, const double* dsd,
                              const double* dacc, double* sn, double* acc_out, double* dsn, double* dacc_out) {
  for (long i = 0; i < n; ++i) {
    D a = dual(acc[i], dacc[i]), o;
    contact_stage_value<D>(stage, dt, dual(s0[i], ds0[i]), dual(sd[i], dsd[i]), a, o);
    sn[i] = o.v; dsn[i] = o.d[0]; acc_out[i] = a.v; dacc_out[i] = a.d[0];
  }
}
extern "C" void emu_stage_value(long n, int stage, double dt, const double* s0, const double* sd, double* acc, double* sn) {
  for (long i = 0; i < n; ++i) contact_stage_value<double>(stage, dt, s0[i], sd[i], acc[i], sn[i]);
}
// the pullback: snb in; s0b, accb in / out; sdb out
extern "C" void emu_stage_adjoint(long n, int stage, double dt, const double* snb, double* s0b, double* accb, double* sdb) {
  for (long i = 0; i < n; ++i) contact_stage_adjoint<double>(stage, dt, snb[i], s0b[i], accb[i], sdb[i]);
}
// The friction state of one pair through a whole RK4 step, the point's position and velocity frozen per stage (pos, vel: [pair][stage][3]).
// Tangents along (dx0, dpos, dvel) of the state after the step, the Dual chain: pair model and value tableau, stage by stage.  xs: the stage states (values).
extern "C" void emu_step_jvp(long n, double dt, const double* pos, const double* vel, const double* x0, const double* c, const double* H, const double* dpos,
                             const double* dvel, const double* dx0, double* x1, double* dx1, double* xs) {
  for (long i = 0; i < n; ++i) {
    D s0[3], s[3], acc[3];
    for (int j = 0; j < 3; ++j) { s0[j] = dual(x0[3 * i + j], dx0[3 * i + j]); s[j] = s0[j]; acc[j] = D(0.0); }
    for (int k = 0; k < 4; ++k) {
      D p[3], w[3], f[3], xd[3];
      for (int j = 0; j < 3; ++j) {
        p[j] = dual(pos[12 * i + 3 * k + j], dpos[12 * i + 3 * k + j]);
        w[j] = dual(vel[12 * i + 3 * k + j], dvel[12 * i + 3 * k + j]);
        xs[12 * i + 3 * k + j] = s[j].v;
      }
      contact_pair_force<D>(p, w, s, c + CP_STRIDE * i, H + 6 * i, f, xd);
      for (int j = 0; j < 3; ++j) contact_stage_value<D>(k, dt, s0[j], xd[j], acc[j], s[j]);
    }
    for (int j = 0; j < 3; ++j) { x1[3 * i + j] = s[j].v; dx1[3 * i + j] = s[j].d[0]; }
  }
}
// The same step pulled back by the hand-written routines: the values forward, then stages 3 … 0 — contact_stage_adjoint per value, contact_pair_adjoint with
// ẋ̄ of the stage; the stage state's cotangent is the pair's x̄ (stage 0: with the cotangent of x0 collected over the stages).
extern "C" void emu_step_adjoint(long n, double dt, const double* pos, const double* vel, const double* x0, const double* c, const double* H, const double* x1b,
                                 double* x0b, double* posb, double* velb) {
  for (long i = 0; i < n; ++i) {
    double s[4][3], acc[3] = {0, 0, 0}, f[3], xd[3], sn[3];
    for (int j = 0; j < 3; ++j) s[0][j] = x0[3 * i + j];
    for (int k = 0; k < 4; ++k) {
      contact_pair_force<double>(pos + 12 * i + 3 * k, vel + 12 * i + 3 * k, s[k], c + CP_STRIDE * i, H + 6 * i, f, xd);
      for (int j = 0; j < 3; ++j) {
        contact_stage_value<double>(k, dt, x0[3 * i + j], xd[j], acc[j], sn[j]);
        if (k < 3) s[k + 1][j] = sn[j];
      }
    }
    double snb[3], s0b[3] = {0, 0, 0}, accb[3] = {0, 0, 0}, sdb[3], xb[3];
    for (int j = 0; j < 3; ++j) snb[j] = x1b[3 * i + j];
    for (int k = 3; k >= 0; --k) {
      for (int j = 0; j < 3; ++j) contact_stage_adjoint<double>(k, dt, snb[j], s0b[j], accb[j], sdb[j]);
      contact_pair_adjoint<double>(pos + 12 * i + 3 * k, vel + 12 * i + 3 * k, s[k], c + CP_STRIDE * i, H + 6 * i, nullptr, nullptr, sdb, nullptr,
                                   posb + 12 * i + 3 * k, velb + 12 * i + 3 * k, xb);
      for (int j = 0; j < 3; ++j) snb[j] = k == 0 ? s0b[j] + xb[j] : xb[j];
    }
    for (int j = 0; j < 3; ++j) x0b[3 * i + j] = snb[j];
  }
}
"""


def build_harness():
    return build(HARNESS, "rbd_simulate_contact_emu")


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang")
    return build_harness()


def test_symbol_declared_and_exported(rbd):
    header = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    lib = ctypes.CDLL(rbd._capi.LIB_PATH)
    for name in NEW:
        assert name + "(" in header, name
        assert name in rbd._capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert callable(rbd.simulate_contact_vjp_) and callable(rbd.autograd.simulate_contact)


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
def test_tableau_pullback_is_the_transpose_of_the_dual_value_form(harness, stage):
    """⟨s̄n, dsn⟩ + ⟨āout, dacc_out⟩ = ⟨s̄0, ds0⟩ + ⟨ṡ̄, dṡ⟩ + ⟨āin, dacc_in⟩ per value at 1e-12 of the summed magnitudes, J·d from the Dual<double, 1>
    instantiation of contact_stage_value; the sum's cotangent out takes part at stages 0-2 (stage 3 does not write the sum), the sum in at stages 1-3 (stage
    0 does not read it: its cotangent comes back zero).  The value form equals the Dual's values bit for bit."""
    rng = np.random.default_rng(100 + stage)
    n = 500
    s0, sd, acc, ds0, dsd, dacc, snb, accb_out, s0b_before = (rng.standard_normal(n) for _ in range(9))
    sn, acc_out, dsn, dacc_out = (np.full(n, np.nan) for _ in range(4))
    harness.emu_stage_jvp(ctypes.c_long(n), stage, ctypes.c_double(DT), _p(s0), _p(sd), _p(acc), _p(ds0), _p(dsd), _p(dacc), _p(sn), _p(acc_out), _p(dsn),
                          _p(dacc_out))
    a2, sn2 = acc.copy(), np.full(n, np.nan)
    harness.emu_stage_value(ctypes.c_long(n), stage, ctypes.c_double(DT), _p(s0), _p(sd), _p(a2), _p(sn2))
    assert np.array_equal(sn2, sn) and (stage == 3 or np.array_equal(a2, acc_out))
    a, b = (0.5, 0.5, 1.0, 0.0)[stage], (1 / 6, 1 / 3, 1 / 3, 1 / 6)[stage]
    summed = (0.0 if stage == 0 else acc) + DT * b * sd
    assert np.abs(sn - (s0 + DT * a * sd if stage < 3 else s0 + summed)).max() <= 1e-15
    # the pullback: at stage 3 s0b and accb are written, below they hold what the later stages left
    s0b = s0b_before.copy() if stage < 3 else np.full(n, np.nan)
    accb = accb_out.copy() if stage < 3 else np.full(n, np.nan)
    sdb = np.full(n, np.nan)
    harness.emu_stage_adjoint(ctypes.c_long(n), stage, ctypes.c_double(DT), _p(snb), _p(s0b), _p(accb), _p(sdb))
    assert np.isfinite(s0b).all() and np.isfinite(accb).all() and np.isfinite(sdb).all()
    s0_share = s0b - (s0b_before if stage < 3 else 0.0)  # (the stage's own contribution to s̄0)
    if stage == 0:
        assert (accb == 0).all()
    left = [snb * dsn] + ([accb_out * dacc_out] if stage < 3 else [])
    right = [s0_share * ds0, sdb * dsd] + ([accb * dacc] if stage > 0 else [])
    mag = sum(np.abs(t) for t in left + right) + 1e-300
    assert (np.abs(sum(left) - sum(right)) <= 1e-12 * mag).all(), (stage, (np.abs(sum(left) - sum(right)) / mag).max())


@pytest.fixture(scope="module")
def step_pairs():
    """The 2000 pairs of random_pairs() at stage 0; at stages 1-3 the point has moved and changed its velocity (2 cm and 0.3 m/s per component, the scale of
    the pairs' penetrations and speeds), so that pairs change branch between the stages."""
    pos, vel, x, par, c, H, rng = random_pairs()
    P = np.stack([pos] + [pos + 0.02 * rng.standard_normal((N, 3)) for _ in range(3)], axis=1).copy()
    V = np.stack([vel] + [vel + 0.3 * rng.standard_normal((N, 3)) for _ in range(3)], axis=1).copy()
    return dict(pos=P, vel=V, x=x, par=par, c=c, H=H, rng=rng)


def step_jvp(harness, sp, dpos, dvel, dx0):
    x1, dx1, xs = np.full((N, 3), np.nan), np.full((N, 3), np.nan), np.full((N, 4, 3), np.nan)
    harness.emu_step_jvp(ctypes.c_long(N), ctypes.c_double(DT), _p(sp["pos"]), _p(sp["vel"]), _p(sp["x"]), _p(sp["c"]), _p(sp["H"]), _p(dpos), _p(dvel), _p(dx0),
                         _p(x1), _p(dx1), _p(xs))
    return x1, dx1, xs


def test_pairs_change_branch_between_the_stages(harness, step_pairs):
    """A condition on the inputs of the next test: at least 10 % of the pairs take different branches at two stages of the step, and every branch is taken
    by at least 5 % of the (pair, stage) evaluations."""
    sp = step_pairs
    z = np.zeros((N, 4, 3))
    _, _, xs = step_jvp(harness, sp, z, z, np.zeros((N, 3)))
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)
    br = []
    for k in range(4):
        info = cm.pair_model(T(sp["pos"][:, k]), T(sp["vel"][:, k]), T(xs[:, k]), T(sp["par"]), T(sp["H"][:, :3]), T(sp["H"][:, 3:]))[3]
        br.append(cm.branch_of(info).numpy())
    br = np.stack(br, axis=1)
    changed = (br != br[:, :1]).any(axis=1).mean()
    cov = [float((br == i).mean()) for i in range(4)]
    print("changed", changed, dict(zip(cm.BRANCHES, cov)))
    assert changed >= 0.10 and min(cov) >= 0.05


def test_chained_adjoints_through_a_step_equal_the_dual_chain(harness, step_pairs):
    """(x̄0, pos_bar, vel_bar of every stage) of the chained hand-written pullbacks against Jᵀ x̄⁺ with J (3 × 27 per pair) from 27 passes of the Dual chain,
    one per input coordinate, at 1e-12·(1 + max|ref|)."""
    sp = step_pairs
    x1b = sp["rng"].standard_normal((N, 3))
    x0b, posb, velb = np.full((N, 3), np.nan), np.full((N, 4, 3), np.nan), np.full((N, 4, 3), np.nan)
    harness.emu_step_adjoint(ctypes.c_long(N), ctypes.c_double(DT), _p(sp["pos"]), _p(sp["vel"]), _p(sp["x"]), _p(sp["c"]), _p(sp["H"]), _p(x1b), _p(x0b),
                             _p(posb), _p(velb))
    ref = np.zeros((N, 27))
    x1 = None
    for e in range(27):
        d = np.zeros((N, 27))
        d[:, e] = 1.0
        dx0, dpos, dvel = d[:, :3].copy(), d[:, 3:15].reshape(N, 4, 3).copy(), d[:, 15:].reshape(N, 4, 3).copy()
        x1, dx1, _ = step_jvp(harness, sp, dpos, dvel, dx0)
        ref[:, e] = (x1b * dx1).sum(axis=1)
    got = np.concatenate([x0b, posb.reshape(N, 12), velb.reshape(N, 12)], axis=1)
    assert np.isfinite(got).all() and np.isfinite(ref).all() and np.isfinite(x1).all()
    for what, sl in (("x0_bar", slice(0, 3)), ("pos_bar", slice(3, 15)), ("vel_bar", slice(15, 27))):
        err = np.abs(got[:, sl] - ref[:, sl]).max()
        print(what, err, np.abs(ref[:, sl]).max())
        assert np.abs(ref[:, sl]).max() > 0
        assert err <= 1e-12 * (1 + np.abs(ref[:, sl]).max()), (what, err)


# ---- the torch step against oracle/simulate_np.py ---------------------------------------------------------------------------------------------------------

def walker_case(rbd, B=8, seed=5):
    rng = np.random.default_rng(seed)
    flat = rbd.flatten(cm.walker(rbd, rng))
    q, v, s = cm.walker_states(rbd, flat, B, rng)
    return flat, q, v, s, rng.random((B, flat.nv)), rng.random((B, 6 * flat.n_bodies))


T64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)


def test_torch_stage_maps_against_simulate_np(rbd, oracle):
    """local_rate and global_coordinates of the torch helper against simulate_np's, state by state, at 1e-12·(1 + max|ref|): at a stage state a step away
    from q0, and at q = q0 (θ = 0 exactly, the first stage of every step), where the value is the reference's branch."""
    import simulate_np as snp
    flat, q0, v, _, _, _ = walker_case(rbd)
    B = q0.shape[0]
    rng = np.random.default_rng(7)
    for scale in (1e-3, 0.3, 0.0):  # (the step sizes of the tests; beyond the series threshold; the singular point)
        phi = scale * rng.standard_normal((B, flat.nv))
        q = sr.global_coordinates(flat, T64(q0), T64(phi)).numpy()
        ref_q = np.stack([snp.global_coordinates(flat, q0[b], phi[b]) for b in range(B)])
        assert np.abs(q - ref_q).max() <= 1e-12 * (1 + np.abs(ref_q).max()), scale
        if scale == 0.0:
            assert np.array_equal(q, q0)
        rate = sr.local_rate(flat, T64(q0), T64(ref_q), T64(v)).numpy()
        ref_r = np.stack([snp.local_rate(flat, q0[b], ref_q[b], v[b]) for b in range(B)])
        assert np.abs(rate - ref_r).max() <= 1e-12 * (1 + np.abs(ref_r).max()), scale


def test_torch_step_against_simulate_np_step_contact(rbd, oracle):
    """Two steps of the torch helper, the oracle supplying (v̇, ṡ) at every stage state, against simulate_np.step_contact state by state at
    1e-12·(1 + max|ref|), quaternions up to sign; with external wrenches, against the same step written with simulate_np's local_rate /
    global_coordinates around oracle.dynamics_contact (step_contact itself takes none)."""
    import simulate_np as snp
    flat, q, v, s, tau, fext = walker_case(rbd)
    B = q.shape[0]

    def np_step(q0, v0, s0, tau_b, fext_b):  # step_contact with fext
        phids, vds, sds = [], [], []
        for i in range(4):
            a = 0.0 if i == 0 else DT * sr.RK4_A[i - 1]
            qq = snp.global_coordinates(flat, q0, a * phids[-1] if i else np.zeros(flat.nv))
            vv, ss = (v0 + a * vds[-1], s0 + a * sds[-1]) if i else (v0, s0)
            vd, _, sd, _, _ = oracle.dynamics_contact(flat, qq[None], vv[None], ss[None], tau_b[None], fext_b[None])
            vds.append(vd[0]); sds.append(sd[0])
            phids.append(snp.local_rate(flat, q0, qq, vv))
        comb = lambda xs: sum(DT * sr.RK4_B[i] * xs[i] for i in range(4))
        return snp.global_coordinates(flat, q0, comb(phids)), v0 + comb(vds), s0 + comb(sds)

    for fe in (None, fext):
        def f(qq, vv, ss):
            vd, _, sd, _, _ = oracle.dynamics_contact(flat, qq.numpy(), vv.numpy(), ss.numpy(), tau, fe)
            return T64(vd), T64(sd), None
        q1, v1, s1, infos = sr.rollout(flat, T64(q), T64(v), T64(s), DT, 2, f)
        assert len(infos) == 2 and len(infos[0]) == 4
        rq, rv, rs = q.copy(), v.copy(), s.copy()
        for _ in range(2):
            for b in range(B):
                rq[b], rv[b], rs[b] = snp.step_contact(flat, rq[b], rv[b], rs[b], DT, tau[b]) if fe is None else np_step(rq[b], rv[b], rs[b], tau[b], fe[b])
        sign = np.sign((q1.numpy()[:, :4] * rq[:, :4]).sum(axis=1))[:, None]
        got_q = np.concatenate([sign * q1.numpy()[:, :4], q1.numpy()[:, 4:]], axis=1)
        for what, got, ref in (("q", got_q, rq), ("v", v1.numpy(), rv), ("s", s1.numpy(), rs)):
            err = np.abs(got - ref).max()
            print(what, err)
            assert err <= 1e-12 * (1 + np.abs(ref).max()), (what, fe is None, err)
        assert np.abs(rs - s).max() > 0  # (the friction state moves)


def test_autograd_through_the_step_is_finite_at_the_singular_stage(rbd):
    """backward() through a step of the helper from rest and from ω = 0 — every stage state at (or next to) θ = 0 — gives finite gradients, and the gradient
    of ϕ̇ at q = q0 exactly is the limit of the gradient at q → q0 (the series keep the first-order terms; no 0 · NaN through torch.where)."""
    flat, q, v, s, tau, _ = walker_case(rbd)
    for case in ("rest", "no_rotation", "generic"):
        vv = v.copy()
        if case == "rest":
            vv[:] = 0
        elif case == "no_rotation":
            vv[:, :3] = 0
        q0, v0 = T64(q).requires_grad_(True), T64(vv).requires_grad_(True)
        f = lambda qq, w, ss: (torch.sin(qq[:, :flat.nv]) + w * w, None, None)  # (a smooth stand-in for the dynamics)
        q1, v1, _, _ = sr.step(flat, q0, v0, None, DT, f)
        (q1.square().sum() + v1.sum()).backward()
        assert bool(torch.isfinite(q0.grad).all()) and bool(torch.isfinite(v0.grad).all()), case
    w = T64(np.random.default_rng(3).standard_normal(v.shape))
    grads = []
    for shift in (0.0, 1e-9):
        qa, qb = T64(q).requires_grad_(True), T64(q).requires_grad_(True)
        phi = torch.full((q.shape[0], flat.nv), shift, dtype=torch.float64)
        rate = sr.local_rate(flat, qa, sr.global_coordinates(flat, qb, phi), T64(v))
        (rate * w).sum().backward()
        grads.append((qa.grad.clone(), qb.grad.clone()))
    for g0, g1 in zip(*grads):
        assert bool(torch.isfinite(g0).all()) and float((g0 - g1).abs().max()) <= 1e-6 * (1 + float(g1.abs().max()))
    assert float(grads[0][0].abs().max()) > 0
