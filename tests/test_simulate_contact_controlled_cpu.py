"""CPU checks around rbd_simulate_contact_controlled: the numpy reference of its GPU tests (tests/simulate_contact_controlled_ref.py) against
oracle/simulate_np.py, the conditions the GPU parity tests assume of their inputs — checked here, on the reference alone, on the very inputs they run —, and
the entry point's presence in the header, the Python binding and the Julia shim."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import contact_model_ref as cm
import simulate_contact_controlled_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constant_controller_is_step_contact(rbd, oracle):
    """The helper with a constant controller equals simulate_np.step_contact on the walker, state by state, at 1e-13 (3 steps, no external wrenches:
    step_contact takes none)."""
    import simulate_np as snp
    rng = np.random.default_rng(5)
    flat = rbd.flatten(cm.walker(rbd, rng))
    B, n = 6, 3
    q, v, s = cm.walker_states(rbd, flat, B, rng)
    tau = rng.random((B, flat.nv))
    gq, gv, gs, infos = ref.rollout(oracle, flat, q, v, s, ref.constant_control(tau), None, n)
    assert len(infos) == n and all(len(i) == 4 for i in infos)
    for b in range(B):
        rq, rv, rs = q[b], v[b], s[b]
        for _ in range(n):
            rq, rv, rs = snp.step_contact(flat, rq, rv, rs, ref.DT, tau[b])
        for name, g, r in (("q", gq[b], rq), ("v", gv[b], rv), ("s", gs[b], rs)):
            assert np.abs(g - r).max() <= 1e-13 * (1 + np.abs(r).max()), (b, name)


def test_controllers_of_the_helper(rbd):
    """The callbacks restate the C ABI's controller kinds: the PD law touches Revolute / Prismatic coordinates only, NULL q_des and tau are zero, a per-stage
    table is read at 4·step + stage and a per-step one at `step`."""
    w = ref.walker_case(rbd, B=3)
    flat = w["flat"]
    on = ref.one_dof(flat) >= 0
    assert on.sum() == 4 and not on[:6].any()  # the floating joint's six coordinates come first
    q, v = w["q"][1], w["v"][1]
    tau = ref.walker_control(w, "pd")(1, 0.0, q, v)
    assert np.array_equal(tau[:6], w["tau"][1][:6])
    qi = ref.one_dof(flat)[on]
    assert np.allclose(tau[on], w["tau"][1][on] - w["kp"][on] * (q[qi] - w["q_des"][1][qi]) - w["kd"][on] * v[on], rtol=0, atol=1e-13)  # (values up to ~20, a few roundings of 2e-16 relative each)
    tau0 = ref.walker_control(w, "pd_null")(1, 0.0, q, v)
    assert not tau0[:6].any() and np.allclose(tau0[on], -w["kp"][on] * q[qi] - w["kd"][on] * v[on], rtol=0, atol=1e-13)  # (values up to ~20, a few roundings of 2e-16 relative each)
    for per_stage in (True, False):
        c = ref.table_control(w["table"], per_stage)
        seen = [c(2, 0.0, q, v) for _ in range(8)]
        for k in range(8):
            assert np.array_equal(seen[k], w["table"][k if per_stage else k // 4][2])


@pytest.fixture(scope="module")
def walker(rbd):
    return ref.walker_case(rbd)


@pytest.mark.parametrize("case", ref.WALKER_CASES)
def test_walker_inputs_satisfy_the_gpu_tests_conditions(rbd, oracle, walker, case):
    """B = 130, 3 steps, each controller case of the GPU parity test: every (point, half-space) pair at every stage of every step is clear of the branch
    boundaries (rel 1e-6); some pair is in contact and some is not; some pair changes branch between two stages."""
    w = walker
    assert w["flat"].ns == 24 and len(w["flat"].contact_points) == 4 and len(w["flat"].halfspaces) == 2
    *_, infos = ref.rollout(oracle, w["flat"], w["q"], w["v"], w["s"], ref.walker_control(w, case), w["fext"], w["nsteps"])
    assert len(ref.stages(infos)) == 12
    assert ref.conditions(infos) == (True, True, True, True)


def test_atlas_inputs_satisfy_the_gpu_tests_conditions(rbd, oracle, models):
    """Atlas with its eight foot points, B = 65, 2 steps, PD on all 1-dof joints: the same conditions."""
    a = ref.atlas_case(rbd, oracle, models["atlas_floating"])
    flat = a["flat"]
    assert flat.n_bodies == 31 and flat.ns == 24 and (ref.one_dof(flat) >= 0).sum() == 30
    *_, infos = ref.rollout(oracle, flat, a["q"], a["v"], a["s"], ref.pd_control(flat, a["kp"], a["kd"], a["q_des"], a["tau"]), a["fext"], a["nsteps"])
    assert ref.conditions(infos) == (True, True, True, True)


def test_entry_point_is_declared_bound_and_called_from_julia(rbd):
    """rbd_simulate_contact_controlled is in the header, in _capi.SYMBOLS, exported by the library, and the Julia shim's ccall of it matches the header."""
    header = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    assert re.search(r"\bint rbd_simulate_contact_controlled\s*\(rbd_ws_t\* ws, int32_t B, void\* q, void\* v, void\* s, const rbd_control_t\* control,", header)
    assert "rbd_simulate_contact_controlled" in rbd._capi.SYMBOLS
    assert hasattr(rbd._capi.lib(), "rbd_simulate_contact_controlled")
    assert ":rbd_simulate_contact_controlled" in open(os.path.join(ROOT, "julia", "RigidBodyDynamicsGPU.jl")).read()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_julia_ccalls.py")], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout, out.stdout + out.stderr
