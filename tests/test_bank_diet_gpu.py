"""The two-bodies-per-lane kernels compiled per mechanism (aba_bank_spec / aba_bank_fused_spec / rnea_bank_spec, csrc/rbd_bank.hpp with the level loops unrolled)
after their commits moved under the exec mask of the lanes that own them (RBD_BANK_COMMIT_INPLACE), the zero fills went (RBD_BANK_LEAN_INIT) and the 6-dof
joint's elements are addressed from one base (RBD_BANK_ONE_BASE): parity with the CPU oracle at the batch sizes around a wavefront's four states and a
workgroup's 64, with and without external wrenches, in both layouts, and the independence of the states that share a wavefront.

Tolerances: fp64 max |x - x_oracle| <= 1e-10 max(1, max |x_oracle|); fp32 the backward error of test_gpu_parity.py (||RNEA(v̇) - τ|| / ||τ - c|| <= 2e-5; τ of
inverse_dynamics! relative 2e-5); `simulate` the bounds of test_gpu_parity.py::test_simulate_matches_oracle_f64."""
import numpy as np
import pytest
import torch

from conftest import rand_inputs, tune
from test_gpu_parity import ND, NT, TD, canon_q, dev, host

pytestmark = pytest.mark.gpu

# atlas_floating: SIMPLE, bodies with three children on levels 0 and 3 (exchange columns on two levels); atlas_fixed: SIMPLE without a 6-dof joint;
# limbs_three: fixed and prismatic joints on a fixed base (the generic instantiation); limbs_humanoid: fixed, prismatic and sin/cos joints below a floating
# base, bodies with three children on levels 0, 2 and 7
MECHS = ["atlas_floating", "atlas_fixed", "limbs_three", "limbs_humanoid"]
BATCHES = [1, 3, 5, 65, 4093]
COMPILED = "compiled for the mechanism at run time"
_ref = {}


def inputs(rbd, model, name, B, dtype):
    """seeded inputs as the device sees them (shared by the layouts), generated once per (mechanism, batch, scalar type)"""
    key = ("in", name, B, dtype)
    if key not in _ref:
        q, v, tau, fe = rand_inputs(rbd, model, B, 1000 + B, fext=True)
        vd = np.random.default_rng(2000 + B).standard_normal((B, model.nv))
        _ref[key] = [a.astype(ND[dtype]).astype(np.float64) for a in (q, v, tau, fe, vd)]
    return _ref[key]


def reference(key, f):
    if key not in _ref:
        _ref[key] = f()
    return _ref[key]


def new_state(rbd, model, B, dtype, layout, q, v):
    state = rbd.MechanismState(model, B, dtype=TD[dtype], layout=layout)
    rbd.set_configuration_(state, q)
    rbd.set_velocity_(state, v)
    return state


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", MECHS)
def test_banked_dynamics_compiled(rbd, oracle, models, name, dtype, layout, monkeypatch):
    tune(monkeypatch, bank_min_batch=1)
    model = models[name]
    for B in BATCHES:
        q, v, tau, fe, _ = inputs(rbd, model, name, B, dtype)
        state = new_state(rbd, model, B, dtype, layout, q, v)
        result = rbd.DynamicsResult(model, B, dtype=TD[dtype], layout=layout)
        for wrenches in (True, False):
            f = fe if wrenches else None
            rbd.dynamics_(result, state, dev(tau, state), dev(f, state) if wrenches else None, algorithm="aba_banks")
            k = rbd.last_kernel(state)
            assert rbd.sync(state) == 0 and "aba_bank_kernel" in k and COMPILED in k, k
            got = host(result.vd, state)
            assert np.isfinite(got).all()
            if dtype == "f64":
                ref, qd_ref = reference(("dyn", name, B, wrenches), lambda: oracle.dynamics(model, q, v, tau, f, want_qdot=True, nthreads=NT))
                err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
                print(f"{name} {layout} B={B} wrenches={wrenches}: rel err {err:.2e}")
                assert err <= 1e-10, (B, wrenches, err)
                assert np.abs(host(result.qd, state) - qd_ref).max() <= 1e-13 * max(1.0, np.abs(qd_ref).max())
            else:
                back = oracle.inverse_dynamics(model, q, v, got, f, nthreads=NT)
                c = reference(("bias32", name, B, wrenches), lambda: oracle.dynamics_bias(model, q, v, f))
                rel = (np.linalg.norm(back - tau, axis=1) / np.linalg.norm(tau - c, axis=1)).max()
                print(f"{name} {layout} B={B} wrenches={wrenches}: fp32 backward error {rel:.2e}")
                assert rel <= 2e-5, (B, wrenches, rel)


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", MECHS)
def test_banked_inverse_dynamics_compiled(rbd, oracle, models, name, dtype, layout, monkeypatch):
    tune(monkeypatch, bank_min_batch=1)
    model = models[name]
    for B in BATCHES:
        q, v, _, fe, vd = inputs(rbd, model, name, B, dtype)
        state = new_state(rbd, model, B, dtype, layout, q, v)
        out = torch.zeros_like(state.v)
        for wrenches in (True, False):
            f = fe if wrenches else None
            rbd.inverse_dynamics_(out, state, dev(vd, state), dev(f, state) if wrenches else None, mapping="banks")
            k = rbd.last_kernel(state)
            assert rbd.sync(state) == 0 and "rnea_bank_kernel" in k and COMPILED in k, k
            ref = reference(("id", name, B, dtype, wrenches), lambda: oracle.inverse_dynamics(model, q, v, vd, f, nthreads=NT))
            got = host(out, state)
            if dtype == "f64":
                err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
                bound = 1e-10
            else:
                err = np.abs(got - ref).max() / np.abs(ref).max()
                bound = 2e-5
            print(f"{name} {layout} {dtype} B={B} wrenches={wrenches}: rel err {err:.2e}")
            assert np.isfinite(got).all() and err <= bound, (B, wrenches, err)


@pytest.mark.parametrize("name,layout", [("atlas_floating", "aos"), ("atlas_floating", "soa"), ("atlas_fixed", "aos"), ("limbs_three", "soa"), ("limbs_humanoid", "aos")])
def test_two_fused_simulate_steps(rbd, oracle, models, name, layout, monkeypatch):
    """Two Munthe-Kaas RK4 steps at 5 states on the banked kernel with the stage fused in (aba_bank_fused_spec: eight launches) against oracle/simulate_np.py."""
    import simulate_np
    # (left to itself `simulate` takes the walk program; here the lane-per-body route with the stage fused in, banked at every batch)
    tune(monkeypatch, bank_min_batch=1, sim_walk_min_batch=1 << 40, walk_min_batch=1 << 40, spec_aba_min_batch=1 << 40)
    model = models[name]
    B, dt, T = 5, 1e-3, 0.0015
    q, v, tau, _ = rand_inputs(rbd, model, B, 151, fext=True)
    state = new_state(rbd, model, B, "f64", layout, q, v)
    ts = rbd.simulate_(state, T, dt=dt, torques=dev(tau, state))
    k = rbd.last_kernel(state)
    assert rbd.sync(state) == 0 and "aba_bank_kernel" in k and COMPILED in k, k
    ts_ref, q_ref, v_ref = simulate_np.simulate(model, q, v, T, dt, tau)
    assert len(ts) == len(ts_ref) == 3
    qg, vg = host(state.q, state), host(state.v, state)
    eq = np.abs(canon_q(model, qg) - canon_q(model, q_ref)).max() / max(1.0, np.abs(q_ref).max())
    ev = np.abs(vg - v_ref).max() / max(1.0, np.abs(v_ref).max())
    print(f"{name} {layout}: q {eq:.2e} v {ev:.2e}")
    assert eq <= 1e-11 and ev <= 1e-9, (eq, ev)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["atlas_floating", "limbs_three"])
def test_states_of_one_wavefront_stay_independent(rbd, models, name, dtype, monkeypatch):
    """Four states share a wavefront (Atlas: 16 lanes each; limbs_three, the generic instantiation: 8 lanes each).  With every input of ONE of them NaN the other three results are, bit for bit, those of the same call without
    the NaN state: nothing a lane does not own is touched by arithmetic outside its exec mask — dynamics! and inverse_dynamics!, with wrenches."""
    # (first_use_check=0: the library's own comparison of a program's first call with the interpreting kernel would find the NaN state and drop the program)
    tune(monkeypatch, bank_min_batch=1, first_use_check=0)
    model = models[name]
    B = 4
    q, v, tau, fe, vd = inputs(rbd, model, name, B, dtype)
    for bad in range(B):
        outs = []
        for poison in (False, True):
            qq, vv, tt, ff, aa = (a.copy() for a in (q, v, tau, fe, vd))
            if poison:
                for a in (qq, vv, tt, ff, aa):
                    a[bad] = np.nan
            state = new_state(rbd, model, B, dtype, "aos", qq, vv)
            result = rbd.DynamicsResult(model, B, dtype=TD[dtype])
            rbd.dynamics_(result, state, dev(tt, state), dev(ff, state), algorithm="aba_banks")
            k = rbd.last_kernel(state)
            assert "aba_bank_kernel" in k and COMPILED in k, k
            out = torch.zeros_like(state.v)
            rbd.inverse_dynamics_(out, state, dev(aa, state), dev(ff, state), mapping="banks")
            k = rbd.last_kernel(state)
            assert rbd.sync(state) == 0 and "rnea_bank_kernel" in k and COMPILED in k, k
            outs.append((result.vd.cpu().numpy().copy(), result.qd.cpu().numpy().copy(), out.cpu().numpy().copy()))
        keep = [b for b in range(B) if b != bad]
        for clean, poisoned in zip(*outs):
            assert np.isfinite(clean).all() and np.isfinite(poisoned[keep]).all()
            assert np.array_equal(clean[keep].view(np.uint8), poisoned[keep].view(np.uint8)), (bad, np.abs(clean[keep] - poisoned[keep]).max())
