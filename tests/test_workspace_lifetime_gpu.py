"""A workspace returns its device memory: rbd_workspace_destroy after every family of calls that allocates lazily leaves the device as it found it."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from conftest import tune
from test_gpu_parity import four_bar_inputs

pytestmark = pytest.mark.gpu
B, DT = 4, 1e-3


def two_point_contact(rbd):
    """A floating body and three revolute ones, a contact point on each of two bodies, one half-space (built as test_contact_vjp_gpu.py builds its 70-body tree)."""
    rng = np.random.default_rng(15)
    mech = rbd.rand_tree_mechanism(rng, ["QuaternionFloating"] + ["Revolute"] * 3)
    for k in (1, 3):
        model = rbd.SoftContactModel(rbd.hunt_crossley_hertz(k=2e3 * (1 + rng.random()), alpha=0.3 * rng.random()),
                                     rbd.ViscoelasticCoulombModel(0.3 + rng.random(), 1e3 * (1 + rng.random()), 1e2 * (1 + rng.random())))
        rbd.add_contact_point_(mech.bodies[1:][k], rbd.ContactPoint(0.3 * rng.standard_normal(3), model))
    rbd.add_environment_primitive_(mech, rbd.HalfSpace3D([0, 0, 0.2], [0.1, -0.2, 1.0]))
    return rbd.flatten(mech)


def chain65(rbd):
    """65 revolute bodies in one chain: more bodies than a wavefront has lanes (the any-size kernels), nv = 65 > 64 (the solves' own vectors)."""
    return rbd.flatten(rbd.rand_tree_mechanism(np.random.default_rng(65), ["Revolute"] * 65, parentselector=lambda mech, rng: mech.bodies[-1]))


# what each mechanism's cycle calls: every family that accepts it (loop joints: no derivatives, no points; contact points: their own VJPs, no others)
TREE = ("dynamics_result", "simulate", "host", "dynamics_derivatives", "simulate_step_derivatives", "dynamics_vjp", "simulate_vjp", "points")
CASES = {
    "double_pendulum": TREE,
    "four_bar": ("dynamics_result", "simulate", "host"),
    "inner_floating": TREE,
    "two_point_contact": ("dynamics_result", "simulate", "host", "points", "dynamics_contact_vjp", "simulate_contact_vjp"),
    "chain65": TREE,
}


@pytest.mark.parametrize("name", list(CASES))
def test_workspace_destroy_returns_device_memory(rbd, models, monkeypatch, name):
    """Per mechanism, B = 4, fp64: build a MechanismState, call once every family that allocates lazily — dynamics! with a result (the CRBA route), simulate,
    host-memory staging, dynamics_derivatives, simulate_step_derivatives, dynamics_vjp_, simulate_vjp (2 steps, then 3 with room for one step start, so that the
    checkpoint buffer regrows), set_points twice with different point counts and point_kinematics, and for the mechanism with contact points
    dynamics_contact_vjp and simulate_contact_vjp —, delete it, collect, synchronise.  Once as a warm-up (the HIP runtime's own first-use allocations, the
    code objects loaded on first use, torch's cached blocks); then torch.cuda.mem_get_info()[0] is the same before and after an identical cycle.  Every tensor
    the cycle needs is made before the first reading.  The kernels compiled per mechanism are off (RBD_JIT=0: no test waits for hiprtc) except for four_bar,
    whose loop program build() compiles: its module is loaded and unloaded by every cycle."""
    if name != "four_bar":
        monkeypatch.setenv("RBD_JIT", "0")
    flat = {"two_point_contact": two_point_contact, "chain65": chain65}[name](rbd) if name in ("two_point_contact", "chain65") else models[name]
    nq, nv, nb, ns = flat.nq, flat.nv, flat.n_bodies, getattr(flat, "ns", 0)
    nx = nq + nv
    rng = np.random.default_rng(7)
    if name == "four_bar":
        q, v, tau = four_bar_inputs(rbd, B, 8)
    else:
        q, v, tau = rbd.rand_configuration(flat, B, rng), rbd.rand_velocity(flat, B, rng), rng.random((B, nv))
    D = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()
    E = lambda n: torch.empty(B, n, dtype=torch.float64, device="cuda")
    qd, vd, td = D(q), D(v), D(tau)
    sd = D(1e-3 * rng.standard_normal((B, ns)))
    bar = {n: D(rng.standard_normal((B, n))) for n in {nq, nv, ns}}
    out = {k: E(n) for k, n in dict(q=nq, v=nv, s=ns, tau=nv, fext=6 * nb, dq=nv * nq, dv=nv * nv, dtau=nv * nv, dxdx=nx * nx, dxdtau=nx * nv, pos2=6, pos3=9).items()}
    hq, hv, htau, hvd, hqd, hlam = q.copy(), v.copy(), tau.copy(), np.zeros((B, nv)), np.zeros((B, nq)), np.zeros((B, max(flat.nc, 1)))
    hM = np.zeros((B, nv * nv))
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L = rbd._capi.lib()
    hopts = rbd._capi.Opts(rbd._capi.LAYOUT_AOS, rbd._capi.MEM_HOST, rbd._capi.ALGO_ABA, 1)

    def reset(st):
        st.q.copy_(qd); st.v.copy_(vd); st.s.copy_(sd)

    def cycle():
        st = rbd.MechanismState(flat, B)
        res = rbd.DynamicsResult(flat, B)
        for family in CASES[name]:
            reset(st)
            if family == "dynamics_result":
                rbd.dynamics_(res, st, td, algorithm="crba")
            elif family == "simulate":
                rbd.simulate_(st, 2 * DT, dt=DT, torques=td)
            elif family == "host" and ns == 0:
                assert L.rbd_dynamics(st.ws.handle, B, P(hq), P(hv), P(htau), None, P(hvd), P(hqd), P(hlam) if flat.nc else None, ctypes.byref(hopts)) == 0
            elif family == "host":  # (rbd_dynamics refuses contact points: the staging of rbd_mass_matrix)
                assert L.rbd_mass_matrix(st.ws.handle, B, P(hq), P(hM), ctypes.byref(hopts)) == 0
            elif family == "dynamics_derivatives":
                rbd.dynamics_derivatives_(st, td, out["dq"], out["dv"], out["dtau"])
            elif family == "simulate_step_derivatives":
                rbd.simulate_step_derivatives_(st, DT, td, out["dxdx"], out["dxdtau"])
            elif family == "dynamics_vjp":
                rbd.dynamics_vjp_(st, bar[nv], td, out["q"], out["v"], out["tau"], fext_bar=out["fext"])
            elif family == "simulate_vjp":
                out["q"].copy_(bar[nq]); out["v"].copy_(bar[nv])
                rbd.simulate_vjp_(out["q"], out["v"], st, DT, 2, torques=td, tau_bar=out["tau"], fext_bar=out["fext"])
                with monkeypatch.context() as mp:
                    tune(mp, sim_vjp_ckpt_steps=1)
                    rbd.simulate_vjp_(out["q"], out["v"], st, DT, 3, torques=td, tau_bar=out["tau"], fext_bar=out["fext"])
            elif family == "points":
                rbd.set_points_(st, [0, nb - 1, nb - 1], [[0.1, 0.2, 0.3], [-0.2, 0.0, 0.4], [0.0, 0.3, 0.1]])
                rbd.point_kinematics_(st, out["pos3"])
                rbd.set_points_(st, [nb - 1, 0], [[0.1, 0.2, 0.3], [-0.2, 0.0, 0.4]])
                rbd.point_kinematics_(st, out["pos2"])
            elif family == "dynamics_contact_vjp":
                rbd.dynamics_contact_vjp_(st, bar[nv], bar[ns], bar[ns], td, None, out["q"], out["v"], out["s"], out["tau"], out["fext"])
            elif family == "simulate_contact_vjp":
                out["q"].copy_(bar[nq]); out["v"].copy_(bar[nv]); out["s"].copy_(bar[ns])
                rbd.simulate_contact_vjp_(out["q"], out["v"], out["s"], st, DT, 2, torques=td, tau_bar=out["tau"], fext_bar=out["fext"])
            else:
                raise AssertionError(family)
        torch.cuda.synchronize()
        del st, res
        gc.collect()
        torch.cuda.synchronize()

    cycle()
    free0 = torch.cuda.mem_get_info()[0]
    cycle()
    free1 = torch.cuda.mem_get_info()[0]
    print("%s: free before %d, after %d" % (name, free0, free1))
    assert free1 == free0
