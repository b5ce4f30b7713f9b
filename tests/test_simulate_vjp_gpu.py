"""Reverse mode through simulate steps on the GPU (rbd_simulate_vjp, header 700 addition, and autograd.simulate): the dot-product identity against
rbd_simulate_jvp per state, one step against [A B]ᵀ x̄ from rbd_simulate_step_derivatives, singular starting points, the two-level checkpoint path, the
state advanced as the JVP advances it, fp32, the edge cases, allocation, gradcheck (reverse and forward mode) and loss.backward() through a Python loop
of steps with per-step torques."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rand_inputs
from test_simulate_derivatives_gpu import DT, dev, host, jvp, make_state, model, step_jacobians

pytestmark = pytest.mark.gpu

MODELS = ["atlas_floating", "atlas_fixed", "double_pendulum", "randmech1", "randmech2", "randmech3", "inner_floating", "mixed20", "chain70"]
FLOATING = 3


def vjp(rbd, flat, q, v, tau, qb, vb, fext=None, nsteps=1, layout="aos", dtype=torch.float64):
    """(q, v after the steps, q̄, v̄ of the initial state, τ̄, f̄ext or None)"""
    B = q.shape[0]
    s = make_state(rbd, flat, q, v, dtype=dtype, layout=layout)
    Qb, Vb = dev(qb, layout, dtype), dev(vb, layout, dtype)
    Tb = dev(np.full((B, flat.nv), np.nan), layout, dtype)
    Fb = None if fext is None else dev(np.full((B, 6 * flat.n_bodies), np.nan), layout, dtype)
    rbd.simulate_vjp_(Qb, Vb, s, DT, nsteps, torques=dev(tau, layout, dtype), externalwrenches=None if fext is None else dev(fext, layout, dtype),
                      tau_bar=Tb, fext_bar=Fb)
    assert "adjoint_mk_stage_kernel" in rbd.last_kernel(s)
    return host(s.q, layout), host(s.v, layout), host(Qb, layout), host(Vb, layout), host(Tb, layout), None if Fb is None else host(Fb, layout)


def check_identity(rbd, flat, q, v, tau, rng, fext=None, nsteps=1, layout="aos", dtype=torch.float64, tol=1e-10):
    """⟨(q̄⁺, v̄⁺), J·(dq, dv, dτ, dfext)⟩ = ⟨(q̄, v̄, τ̄, f̄ext), (dq, dv, dτ, dfext)⟩ per state, J·d from rbd_simulate_jvp"""
    B = q.shape[0]
    dq, dv, dtau = rng.standard_normal((B, 1, flat.nq)), rng.standard_normal((B, 1, flat.nv)), rng.standard_normal((B, 1, flat.nv))
    dfe = None if fext is None else rng.standard_normal((B, 1, 6 * flat.n_bodies))
    qb1, vb1 = rng.standard_normal((B, flat.nq)), rng.standard_normal((B, flat.nv))
    q1, v1, gq, gv = jvp(rbd, flat, q, v, tau, dq, dv, dtau, fext=fext, dfext=dfe, nsteps=nsteps, layout=layout, dtype=dtype)
    r1, w1, Qb, Vb, Tb, Fb = vjp(rbd, flat, q, v, tau, qb1, vb1, fext=fext, nsteps=nsteps, layout=layout, dtype=dtype)
    for x in (Qb, Vb, Tb) + (() if Fb is None else (Fb,)):
        assert np.isfinite(x).all()
    # the state advanced as rbd_simulate_jvp advances it (fp32: the factorisations of M at every stage amplify the rounding of the stage map's values)
    st = 1e-12 if dtype == torch.float64 else 1e-3
    assert np.abs(r1 - q1).max() <= st * (1 + np.abs(q1).max())
    assert np.abs(w1 - v1).max() <= st * (1 + np.abs(v1).max())
    lt = [qb1 * gq[:, 0], vb1 * gv[:, 0]]
    rt = [Qb * dq[:, 0], Vb * dv[:, 0], Tb * dtau[:, 0]] + ([] if fext is None else [Fb * dfe[:, 0]])
    lhs, rhs = sum(t.sum(axis=1) for t in lt), sum(t.sum(axis=1) for t in rt)
    scale = sum(np.abs(t).sum(axis=1) for t in lt + rt)
    err = np.abs(lhs - rhs) / scale
    assert err.max() <= tol, (flat.nq, nsteps, layout, err.max())


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", MODELS)
def test_dot_product_identity_against_jvp(rbd, models, name, layout):
    flat = model(rbd, models, name)
    B = 4096 if name == "atlas_floating" else 8
    rng = np.random.default_rng(31)
    q, v, tau, fext = rand_inputs(rbd, flat, B, 32, fext=True)
    for nsteps in (1, 5):
        for fe in (None, fext):
            check_identity(rbd, flat, q, v, tau, rng, fext=fe, nsteps=nsteps, layout=layout)


@pytest.mark.parametrize("name", ["atlas_floating", "mixed20"])
def test_dot_product_identity_fp32(rbd, models, name):
    flat = model(rbd, models, name)
    rng = np.random.default_rng(33)
    q, v, tau, fext = rand_inputs(rbd, flat, 64, 34, fext=True)
    check_identity(rbd, flat, q, v, tau, rng, fext=fext, nsteps=5, dtype=torch.float32, tol=1e-4)


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", ["atlas_floating", "inner_floating", "mixed20", "chain70"])
def test_one_step_equals_transposed_step_jacobians(rbd, models, name, layout):
    flat = model(rbd, models, name)
    B = 16
    rng = np.random.default_rng(35)
    q, v, tau = rand_inputs(rbd, flat, B, 36)
    qb1, vb1 = rng.standard_normal((B, flat.nq)), rng.standard_normal((B, flat.nv))
    _, _, A, Bt = step_jacobians(rbd, flat, q, v, tau, layout=layout)
    _, _, Qb, Vb, Tb, _ = vjp(rbd, flat, q, v, tau, qb1, vb1, layout=layout)
    x = np.concatenate([qb1, vb1], axis=1)
    ref_x, ref_t = np.einsum("bij,bi->bj", A, x), np.einsum("bij,bi->bj", Bt, x)
    got_x = np.concatenate([Qb, Vb], axis=1)
    assert np.abs(got_x - ref_x).max() <= 1e-10 * (1 + np.abs(ref_x).max())
    assert np.abs(Tb - ref_t).max() <= 1e-10 * (1 + np.abs(ref_t).max())


@pytest.mark.parametrize("case", ["rest", "no_rotation"])
@pytest.mark.parametrize("name", ["atlas_floating", "inner_floating"])
def test_singular_starting_points(rbd, models, name, case):
    """From rest (v = 0), and with every floating joint at ω = 0 and a linear velocity: the stage states sit at (or next to) θ = 0 of the quaternion joints'
    branches, where the stage map's pullback goes through the θ²-series and the value-of-the-branch convention."""
    flat = model(rbd, models, name)
    rng = np.random.default_rng(37)
    q, v, tau, fext = rand_inputs(rbd, flat, 8, 38, fext=True)
    if case == "rest":
        v[:] = 0
    else:
        for i in range(flat.n_bodies):
            if int(flat.joint_type[i]) == FLOATING:
                vo = int(flat.v_offset[i])
                v[:, vo:vo + 3] = 0
    for nsteps in (1, 5):
        check_identity(rbd, flat, q, v, tau, rng, fext=fext, nsteps=nsteps)


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_checkpoint_recompute_path(rbd, models, monkeypatch, layout):
    """Two-level checkpointing (room for 4 step starts: every 5th kept, the segments' others recomputed; 17 steps are no multiple of 5) gives what keeping
    every start gives, to rounding."""
    flat = models["atlas_floating"]
    B = 64
    rng = np.random.default_rng(39)
    q, v, tau, fext = rand_inputs(rbd, flat, B, 40, fext=True)
    qb1, vb1 = rng.standard_normal((B, flat.nq)), rng.standard_normal((B, flat.nv))
    ref = vjp(rbd, flat, q, v, tau, qb1, vb1, fext=fext, nsteps=17, layout=layout)
    monkeypatch.setenv("RBD_TUNE", "sim_vjp_ckpt_steps=4")
    got = vjp(rbd, flat, q, v, tau, qb1, vb1, fext=fext, nsteps=17, layout=layout)
    for a, b in zip(got, ref):
        assert np.abs(a - b).max() <= 1e-13 * (1 + np.abs(b).max())
    check_identity(rbd, flat, q, v, tau, rng, fext=fext, nsteps=17, layout=layout)


def test_errors_and_noops(rbd, models):
    flat = models["mixed20"]
    B = 4
    q, v, tau = rand_inputs(rbd, flat, B, 41)
    s = make_state(rbd, flat, q, v)
    nq, nv, nf = flat.nq, flat.nv, 6 * flat.n_bodies
    p = lambda x: rbd.state._ptr(x)
    L, opts = rbd._capi.lib(), s._opts()
    qb, vb = torch.ones_like(s.q), torch.ones_like(s.v)
    tb, fb = torch.full_like(s.v, float("nan")), torch.full((B, nf), float("nan"), dtype=torch.float64, device="cuda")
    call = lambda B_, q_, v_, dt, n, qb_, vb_, o=opts: L.rbd_simulate_vjp(s.ws.handle, B_, p(q_), p(v_), None, None, ctypes.c_double(dt), n, p(qb_), p(vb_),
                                                                           p(tb), p(fb), ctypes.byref(o))
    # NULL q, v, q̄ or v̄, dt <= 0, nsteps < 0: RBD_ERR_INVALID_ARGUMENT
    for args in ((None, s.v, DT, 1, qb, vb), (s.q, None, DT, 1, qb, vb), (s.q, s.v, DT, 1, None, vb), (s.q, s.v, DT, 1, qb, None), (s.q, s.v, 0.0, 1, qb, vb),
                 (s.q, s.v, -DT, 1, qb, vb), (s.q, s.v, DT, -1, qb, vb)):
        assert call(B, *args) == 1
    # RBD_MEM_HOST: RBD_ERR_UNSUPPORTED
    assert call(B, s.q, s.v, DT, 1, qb, vb, o=rbd._capi.Opts(rbd._capi.LAYOUT_AOS, rbd._capi.MEM_HOST, 0, 1)) == 3
    q0, v0 = s.q.clone(), s.v.clone()
    # B == 0: a successful no-op
    assert call(0, s.q, s.v, DT, 3, qb, vb) == 0
    torch.cuda.synchronize()
    assert torch.isnan(tb).all() and torch.isnan(fb).all() and torch.equal(s.q, q0) and torch.equal(s.v, v0) and bool((qb == 1).all())
    # nsteps == 0: q, v, q̄, v̄ as they were, τ̄ and f̄ext zeroed
    assert call(B, s.q, s.v, DT, 0, qb, vb) == 0
    torch.cuda.synchronize()
    assert bool((tb == 0).all()) and bool((fb == 0).all()) and torch.equal(s.q, q0) and torch.equal(s.v, v0) and bool((qb == 1).all() and (vb == 1).all())
    with pytest.raises(rbd.DimensionMismatch):
        rbd.simulate_vjp_(torch.zeros((B, nq + 1), dtype=torch.float64, device="cuda"), vb, s, DT)
    with pytest.raises(ValueError):
        rbd.simulate_vjp_(qb, vb, s, DT, -1)
    # loop joints: RBD_ERR_HAS_LOOPS
    fbar = models["four_bar"]
    s4 = make_state(rbd, fbar, *rand_inputs(rbd, fbar, 2, 42)[:2])
    with pytest.raises(RuntimeError, match="tree Mechanisms"):
        rbd.simulate_vjp_(torch.zeros_like(s4.q), torch.zeros_like(s4.v), s4, DT)
    # contact points with an environment: RBD_ERR_UNSUPPORTED
    rng = np.random.default_rng(43)
    mech = rbd.rand_tree_mechanism(rng, ["QuaternionFloating", "Revolute"])
    cm = rbd.SoftContactModel(rbd.hunt_crossley_hertz(), rbd.ViscoelasticCoulombModel(0.5, 1e3, 1e3))
    rbd.add_contact_point_(mech.bodies[-1], rbd.ContactPoint(np.zeros(3), cm))
    rbd.add_environment_primitive_(mech, rbd.HalfSpace3D([0, 0, 0], [0, 0, 1.0]))
    fc = rbd.flatten(mech)
    sc = make_state(rbd, fc, *rand_inputs(rbd, fc, 2, 44)[:2])
    with pytest.raises(rbd._capi.RBDError) as e:
        rbd.simulate_vjp_(torch.zeros_like(sc.q), torch.zeros_like(sc.v), sc, DT)
    assert e.value.status == 3


def test_second_call_allocates_nothing(rbd, models):
    flat = models["atlas_floating"]
    B = 256
    q, v, tau, fext = rand_inputs(rbd, flat, B, 45, fext=True)
    s = make_state(rbd, flat, q, v)
    t, f = dev(tau, "aos"), dev(fext, "aos")  # (every tensor of the test made before the measurement)
    qb, vb, tb, fb = (torch.ones((B, n), dtype=torch.float64, device="cuda") for n in (flat.nq, flat.nv, flat.nv, 6 * flat.n_bodies))
    rbd.simulate_vjp_(qb, vb, s, DT, 4, torques=t, externalwrenches=f, tau_bar=tb, fext_bar=fb)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    rbd.simulate_vjp_(qb, vb, s, DT, 4, torques=t, externalwrenches=f, tau_bar=tb, fext_bar=fb)
    rbd.simulate_vjp_(qb, vb, s, DT, 2, torques=t)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0


def test_gradcheck(rbd, models):
    """torch.autograd.gradcheck in fp64, reverse and forward mode, through autograd.simulate (with and without the optional inputs)."""
    flat = models["double_pendulum"]
    B = 2
    q, v, tau, fext = rand_inputs(rbd, flat, B, 46, fext=True)
    s = rbd.MechanismState(flat, B)
    g = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=True)
    f = lambda *a: rbd.autograd.simulate(s, *a, dt=1e-2, nsteps=3)
    assert torch.autograd.gradcheck(f, (g(q), g(v), g(tau), g(fext)), check_forward_ad=True)
    assert torch.autograd.gradcheck(lambda qq, vv: rbd.autograd.simulate(s, qq, vv, dt=1e-2, nsteps=2), (g(q), g(v)), check_forward_ad=True)


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_loss_backward_through_a_loop_of_steps(rbd, models, layout):
    """loss.backward() through 10 one-step calls with a torque per step (backpropagation through time) equals the chained products of the step Jacobians:
    x̄_k = A_kᵀ x̄_{k+1}, τ̄_k = B_kᵀ x̄_{k+1}."""
    flat = models["atlas_floating"]
    B, N = 32, 10
    rng = np.random.default_rng(47)
    q, v, _ = rand_inputs(rbd, flat, B, 48)
    taus = [rng.standard_normal((B, flat.nv)) for _ in range(N)]
    wq, wv = rng.standard_normal((B, flat.nq)), rng.standard_normal((B, flat.nv))
    s = rbd.MechanismState(flat, B, layout=layout)
    Q, V = dev(q, layout).requires_grad_(True), dev(v, layout).requires_grad_(True)
    T = [dev(t, layout).requires_grad_(True) for t in taus]
    x = (Q, V)
    for k in range(N):
        x = rbd.autograd.simulate(s, x[0], x[1], T[k], dt=DT)
    ((dev(wq, layout) * x[0]).sum() + (dev(wv, layout) * x[1]).sum()).backward()
    # the reference: the step Jacobians along the trajectory, chained backwards
    qs, vs, As, Bs = [q], [v], [], []
    for k in range(N):
        q1, v1, A, Bt = step_jacobians(rbd, flat, qs[-1], vs[-1], taus[k], layout=layout)
        qs.append(q1); vs.append(v1); As.append(A); Bs.append(Bt)
    xb = np.concatenate([wq, wv], axis=1)
    tref = [None] * N
    for k in reversed(range(N)):
        tref[k] = np.einsum("bij,bi->bj", Bs[k], xb)
        xb = np.einsum("bij,bi->bj", As[k], xb)
    got = np.concatenate([host(Q.grad, layout), host(V.grad, layout)], axis=1)
    assert np.abs(got - xb).max() <= 1e-8 * (1 + np.abs(xb).max())
    for k in range(N):
        g = host(T[k].grad, layout)
        assert np.abs(g - tref[k]).max() <= 1e-8 * (1 + np.abs(tref[k]).max()), k
