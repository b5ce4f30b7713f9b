"""The banked dynamics! kernels compiled per mechanism with the bias accelerations summed by the kinematics sweep (csrc/rbd_bank.hpp RBD_BANK_BIAS_SWEEP:
zt = zt_parent + [Tw_parent, Tw] on every top-down hop, I zt added to the bias force once per bank, the recursion run with c = 0), against the CPU
oracle on states built to show a zt that went astray.  One call per mechanism, scalar type and layout with B = 2 nv + 1 states, random q and τ:
  * state k < nv: velocity k alone is non-zero — a zt that does not reach every descendant of joint k's body (across a level that hops through the exchange
    columns, across the bank boundary) leaves the distal joints' v̇ without their Coriolis terms;
  * states nv .. 2 nv - 1: every velocity scaled by VSCALE — zt is large, and is added to and cancelled against the other bias terms;
  * the last state: v = 0, zt = 0.
B = 1 and B = 5 (a ragged last wavefront) run the first states of the same pattern.

Bounds: fp64 max |v̇ - v̇_oracle| <= 1e-10 max(1, max |v̇_oracle|); fp32 the backward error of test_bank_diet_gpu.py (||RNEA(v̇) - τ|| / ||τ - c|| <= 2e-5).
VSCALE = 8: the first scale tried; the kernels of the parent revision (cb formed per body, Ia cb per hand-off) pass the same file at it with more than a factor 2 to
spare — their largest figures over all cases: fp64 4.1e-13 (a factor 250 inside the bound), fp32 4.0e-6 (a factor 5) — so it was not halved (at 4: 5.5e-13 and
4.0e-6).  This revision's largest: fp64 4.2e-13, fp32 3.3e-6, both on limbs_humanoid."""
import numpy as np
import pytest

from conftest import rand_inputs, tune
from test_gpu_parity import ND, NT, TD, dev, host

pytestmark = pytest.mark.gpu

# atlas_floating: SIMPLE, later children on levels 0 and 3, the bank boundary at level 5; atlas_fixed: SIMPLE, no 6-dof joint; limbs_three: the generic
# instantiation (fixed and prismatic joints, fixed base); limbs_humanoid: generic below a floating base, later children on levels 0, 2 and 7
MECHS = ["atlas_floating", "atlas_fixed", "limbs_three", "limbs_humanoid"]
COMPILED = "compiled for the mechanism at run time"
VSCALE = 8.0
_cache = {}


def pattern(rbd, model, name, dtype, scale=VSCALE):
    """q, v, tau, wrenches of the 2 nv + 1 states, as the device sees them (rounded to the scalar type)"""
    key = (name, dtype, scale)
    if key not in _cache:
        nv = model.nv
        B = 2 * nv + 1
        q, v, tau, fe = rand_inputs(rbd, model, B, 4242, fext=True)
        v = np.sign(v) * (0.5 + np.abs(v))  # (no velocity close to zero: every single-velocity state has its Coriolis terms)
        vv = np.zeros_like(v)
        for k in range(nv):
            vv[k, k] = v[k, k]
        vv[nv:2 * nv] = scale * v[nv:2 * nv]
        _cache[key] = [a.astype(ND[dtype]).astype(np.float64) for a in (q, vv, tau, fe)]
    return _cache[key]


def figure(rbd, oracle, model, name, dtype, layout, B, wrenches, scale=VSCALE):
    """the figure the bound is on, for the first B states of the pattern: fp64 the error relative to max(1, max |oracle|), fp32 the backward error"""
    q, v, tau, fe = (a[:B] for a in pattern(rbd, model, name, dtype, scale))
    state = rbd.MechanismState(model, B, dtype=TD[dtype], layout=layout)
    rbd.set_configuration_(state, q)
    rbd.set_velocity_(state, v)
    result = rbd.DynamicsResult(model, B, dtype=TD[dtype], layout=layout)
    f = fe if wrenches else None
    rbd.dynamics_(result, state, dev(tau, state), dev(f, state) if wrenches else None, algorithm="aba_banks")
    k = rbd.last_kernel(state)
    assert rbd.sync(state) == 0 and "aba_bank_kernel" in k and COMPILED in k, k
    got = host(result.vd, state)
    assert np.isfinite(got).all()
    rkey = ("ref", name, dtype, scale, wrenches)
    if rkey not in _cache:  # (of the whole pattern, once: the shorter batches are its first states)
        Q, V, T, F = pattern(rbd, model, name, dtype, scale)
        _cache[rkey] = (oracle.dynamics(model, Q, V, T, F if wrenches else None, nthreads=NT) if dtype == "f64"
                        else oracle.dynamics_bias(model, Q, V, F if wrenches else None))
    if dtype == "f64":
        ref = _cache[rkey][:B]
        return np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
    back = oracle.inverse_dynamics(model, q, v, got, f, nthreads=NT)
    c = _cache[rkey][:B]
    return (np.linalg.norm(back - tau, axis=1) / np.linalg.norm(tau - c, axis=1)).max()


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", MECHS)
def test_bias_sweep_states(rbd, oracle, models, name, dtype, layout, monkeypatch):
    tune(monkeypatch, bank_min_batch=1)
    model = models[name]
    bound = 1e-10 if dtype == "f64" else 2e-5
    for B in (2 * model.nv + 1, 5, 1):
        for wrenches in (True, False):
            err = figure(rbd, oracle, model, name, dtype, layout, B, wrenches)
            print(f"{name} {dtype} {layout} B={B} wrenches={wrenches}: {err:.2e}")
            assert err <= bound, (B, wrenches, err)
