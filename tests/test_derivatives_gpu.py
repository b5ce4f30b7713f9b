"""Forward-mode derivatives of inverse_dynamics! and dynamics! on the GPU (header 700: rbd_inverse_dynamics_jvp, rbd_dynamics_jvp,
rbd_inverse_dynamics_derivatives, rbd_dynamics_derivatives): tangents and full Jacobians against the quad-precision oracle (oracle.jvp, oracle.jacobians: exact
to double rounding, in raw coordinates; the bounds: tests/derivative_parity.py), the reference's own autodiff identities (test/test_mechanism_algorithms.jl:600-652), Jacobian columns against JVPs, fp32 against fp64, and the edge cases."""
import numpy as np
import pytest
import torch

from conftest import LIMBS, rand_inputs
from derivative_parity import assert_no_solve, assert_solve_forward, cond_M, jvp_directions

pytestmark = pytest.mark.gpu

FD_MODELS = ["atlas_floating", "atlas_fixed", "valkyrie_floating", "double_pendulum", "randmech1", "randmech2", "randmech3", "inner_floating", "mixed20", "chain70"]

# trees of at most 64 bodies with more than 64 velocity coordinates: the lane-per-body kernels take them, the dense solve does not hold a row per lane
NV_OVER_64 = ["nv66_spherical", "nv65_mixed"]
NV_OVER_64_TYPES = {"nv66_spherical": ["QuaternionSpherical"] * 22,
                    "nv65_mixed": ["QuaternionFloating"] + ["QuaternionSpherical"] * 12 + ["Planar"] * 5 + ["Revolute"] * 6 + ["Prismatic"] * 2}


def at_most_3_children(m, r):
    return m.bodies[max(1, len(m.bodies) - 1 - int(r.integers(0, 3)))]


def model(rbd, models, name):
    if name in NV_OVER_64_TYPES:
        return rbd.flatten(rbd.rand_tree_mechanism(np.random.default_rng(5), NV_OVER_64_TYPES[name], at_most_3_children))
    if name == "chain70":  # a tree of more than 64 bodies: the any-size tables
        return rbd.flatten(rbd.rand_tree_mechanism(np.random.default_rng(70), ["QuaternionFloating"] + ["Revolute", "Prismatic", "SinCosRevolute", "Revolute"] * 17 + ["Revolute"]))
    if name == "tree20":  # test/test_mechanism_algorithms.jl:618: rand_tree_mechanism with 10 revolute and 10 prismatic joints
        return rbd.flatten(rbd.rand_tree_mechanism(np.random.default_rng(20), ["Revolute"] * 10 + ["Prismatic"] * 10))
    return models[name]


def dev(a, state):
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=state.dtype)
    return (t if state.layout == "aos" else t.t().contiguous()).cuda()


def host(t, state):
    t = t.detach().double().cpu()
    return (t if state.layout == "aos" else t.t()).numpy().copy()


def make_state(rbd, flat, q, v, dtype=torch.float64, layout="aos"):
    s = rbd.MechanismState(flat, q.shape[0], dtype=dtype, layout=layout)
    rbd.set_configuration_(s, q)
    rbd.set_velocity_(s, v)
    return s


def close(got, ref, tol, what=""):
    err = np.abs(got - ref).max()
    assert err <= tol * (1 + np.abs(ref).max()), (what, err, np.abs(ref).max())


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", FD_MODELS)
def test_jvp_against_central_difference(rbd, oracle, models, name, layout):
    """Against the central difference of the oracle evaluated in QUAD precision (exact to double rounding; it was an fp64 difference, good to 1e-7): inverse
    dynamics at the fp64 parity number 1e-10, dynamics state by state at C · cond₂(M_b) · eps64 with the model's measured C (profiles/derivative_parity.txt)."""
    flat = model(rbd, models, name)
    B, ntan = (4096, 1) if name == "atlas_floating" else (16, 2)
    q, v, tau, fext = rand_inputs(rbd, flat, B, 11, fext=True)
    vd = np.random.default_rng(13).standard_normal((B, flat.nv))
    d = jvp_directions(flat, B, ntan)  # (dq not projected on any quaternion's unit sphere: raw-coordinate derivatives)
    s = make_state(rbd, flat, q, v, layout=layout)
    flat2 = lambda a: dev(a.reshape(B, -1), s)
    out = torch.full_like(flat2(d["v"]), float("nan"))
    rbd.inverse_dynamics_jvp_(out, s, dev(vd, s), ntan, dq=flat2(d["q"]), dv=flat2(d["v"]), dvd=flat2(d["vd"]), externalwrenches=dev(fext, s), dexternalwrenches=flat2(d["f"]))
    got = host(out, s).reshape(B, ntan, flat.nv)
    ref = oracle.jvp(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext, d["q"], d["v"], d["vd"], d["f"])
    for k in range(ntan):
        assert_no_solve(got[:, k], ref[:, k], name, "jvp inverse_dynamics %s %d" % (layout, k))
    out = torch.full_like(flat2(d["v"]), float("nan"))
    rbd.dynamics_jvp_(out, s, ntan, torques=dev(tau, s), dq=flat2(d["q"]), dv=flat2(d["v"]), dtorques=flat2(d["tau"]), externalwrenches=dev(fext, s), dexternalwrenches=flat2(d["f"]))
    got = host(out, s).reshape(B, ntan, flat.nv)
    ref = oracle.jvp(flat, oracle.WHAT_DYNAMICS, q, v, tau, fext, d["q"], d["v"], d["tau"], d["f"])
    kappa = cond_M(oracle, flat, q)
    for k in range(ntan):
        assert_solve_forward(got[:, k], ref[:, k], kappa, name, "jvp dynamics %s %d" % (layout, k))
    assert "tangent" in rbd.last_kernel(s)


def jacobians(rbd, s, flat, vd, tau, fext=None):
    B, nq, nv = s.batch, flat.nq, flat.nv
    z = lambda n: torch.full_like(s.q[:, :1].expand(B, n).contiguous() if s.layout == "aos" else s.q[:1, :].expand(n, B).contiguous(), float("nan"))
    Tq, Tv, M, tau_out = z(nv * nq), z(nv * nv), z(nv * nv), z(nv)
    rbd.inverse_dynamics_derivatives_(s, vd, Tq, Tv, M, externalwrenches=fext, torquesout=tau_out)
    Aq, Av, Ainv, vd_out = z(nv * nq), z(nv * nv), z(nv * nv), z(nv)
    rbd.dynamics_derivatives_(s, tau, Aq, Av, Ainv, externalwrenches=fext, vdout=vd_out)
    v3 = lambda t, cols: rbd.jacobian_view(t, s, nv, cols).double().cpu().numpy()
    return dict(tq=v3(Tq, nq), tv=v3(Tv, nv), M=v3(M, nv), tau=host(tau_out, s), aq=v3(Aq, nq), av=v3(Av, nv), Minv=v3(Ainv, nv), vd=host(vd_out, s))


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", FD_MODELS + LIMBS + NV_OVER_64)
def test_jacobians_against_the_quad_oracle(rbd, oracle, models, name, layout):
    """The full Jacobians of both entry points, external wrenches present, against unit-direction derivatives of the quad-precision oracle in raw coordinates:
    ∂τ/∂(q, v, v̇) at 1e-10, ∂v̇/∂(q, v, τ) state by state at the model's C · cond₂(M_b) · eps64.  8 states: a full Jacobian costs ~2 (nq + 2 nv) quad evaluations."""
    flat = model(rbd, models, name)
    B = 8
    q, v, tau, fext = rand_inputs(rbd, flat, B, 11, fext=True)
    vd = np.random.default_rng(13).standard_normal((B, flat.nv))
    s = make_state(rbd, flat, q, v, layout=layout)
    J = jacobians(rbd, s, flat, dev(vd, s), dev(tau, s), fext=dev(fext, s))
    T = oracle.jacobians(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext)
    A = oracle.jacobians(flat, oracle.WHAT_DYNAMICS, q, v, tau, fext)
    for key, ref in (("tq", T["q"]), ("tv", T["v"]), ("M", T["x"]), ("tau", T["val"])):
        assert_no_solve(J[key], ref, name, "jacobian %s %s" % (key, layout))
    kappa = cond_M(oracle, flat, q)
    for key, ref in (("aq", A["q"]), ("av", A["v"]), ("Minv", A["x"])):
        assert_solve_forward(J[key], ref, kappa, name, "jacobian %s %s" % (key, layout))
    close(J["vd"], A["val"], 1e-10, "vdot")


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", ["atlas_floating", "mixed20", "tree20", "chain70"])
def test_reference_identities(rbd, oracle, models, name, layout):
    flat = model(rbd, models, name)
    B = 8
    q, v, tau = rand_inputs(rbd, flat, B, 21)
    rng = np.random.default_rng(4)
    vd = rng.standard_normal((B, flat.nv))
    s = make_state(rbd, flat, q, v, layout=layout)
    J = jacobians(rbd, s, flat, dev(vd, s), dev(tau, s))
    Mo = oracle.mass_matrix(flat, q)
    Ms = np.tril(Mo) + np.transpose(np.tril(Mo, -1), (0, 2, 1))
    scale = lambda X: 1e-10 * max(1.0, np.abs(X).max())
    # ∂τ/∂v̇ = M (:600-614)
    assert np.abs(J["M"] - Ms).max() <= scale(Ms)
    # ∂v̇/∂τ = M⁻¹
    assert np.abs(np.einsum("bij,bjk->bik", Ms, J["Minv"]) - np.eye(flat.nv)).max() <= 1e-10 * max(1.0, np.linalg.cond(Ms).max() * 1e-3)
    # M ∂v̇/∂q = −∂τ/∂q at the computed v̇
    Tq_at = jacobians(rbd, s, flat, dev(J["vd"], s), dev(tau, s))["tq"]
    assert np.abs(np.einsum("bij,bjk->bik", Ms, J["aq"]) + Tq_at).max() <= scale(Tq_at)
    # values: τ = rbd_inverse_dynamics, v̇ = the CRBA route of rbd_dynamics
    t_ref = torch.zeros_like(s.v)
    rbd.inverse_dynamics_(t_ref, s, dev(vd, s))
    close(J["tau"], host(t_ref, s), 1e-12, "tau")
    r = rbd.DynamicsResult(flat, B, layout=layout)
    rbd.dynamics_(r, s, dev(tau, s), algorithm="crba")
    close(J["vd"], host(r.vd, s), 1e-12, "vdot")


@pytest.mark.parametrize("name", ["tree20"])
def test_mdot_minus_2c_skew_symmetric(rbd, oracle, models, name):
    """test/test_mechanism_algorithms.jl:616-652: Ṁ from JVPs along dq = q̇ (= v for these joints) at v̇ = e_j minus v̇ = 0, C = ½ ∂τ/∂v."""
    flat = model(rbd, models, name)
    assert flat.nq == flat.nv  # (q̇ = v: revolute and prismatic joints only)
    B, nv = 4, flat.nv
    q, v, _ = rand_inputs(rbd, flat, B, 31)
    s = make_state(rbd, flat, q, v)
    Md = np.zeros((B, nv, nv))
    jvp = lambda vd: rbd.inverse_dynamics_jvp_(torch.zeros((B, nv), dtype=torch.float64, device="cuda"), s, dev(vd, s), 1, dq=dev(v, s)).cpu().numpy()
    base = jvp(np.zeros((B, nv)))
    for j in range(nv):
        e = np.zeros((B, nv)); e[:, j] = 1
        Md[:, :, j] = jvp(e) - base
    Tv = torch.zeros((B, nv * nv), dtype=torch.float64, device="cuda")
    rbd.inverse_dynamics_derivatives_(s, torch.zeros_like(s.v), dtau_dv=Tv)
    C = 0.5 * rbd.jacobian_view(Tv, s, nv, nv).cpu().numpy()
    S = Md - 2 * C
    assert np.abs(S + np.transpose(S, (0, 2, 1))).max() <= 1e-10 * max(1.0, np.abs(S).max())


@pytest.mark.parametrize("name", ["atlas_floating", "inner_floating", "chain70"])
def test_jacobian_columns_are_jvps(rbd, models, name):
    flat = model(rbd, models, name)
    B, nq, nv = 6, flat.nq, flat.nv
    q, v, tau = rand_inputs(rbd, flat, B, 41)
    vd = np.random.default_rng(5).standard_normal((B, nv))
    s = make_state(rbd, flat, q, v)
    J = jacobians(rbd, s, flat, dev(vd, s), dev(tau, s))
    E = np.eye(nq + nv)
    nt = nq + nv
    dq = dev(np.tile(E[:, :nq].reshape(1, -1), (B, 1)), s)
    dv = dev(np.tile(E[:, nq:].reshape(1, -1), (B, 1)), s)
    out = torch.zeros((B, nv * nt), dtype=torch.float64, device="cuda")
    rbd.inverse_dynamics_jvp_(out, s, dev(vd, s), nt, dq=dq, dv=dv)
    ref = np.concatenate([J["tq"], J["tv"]], axis=2)
    close(out.cpu().numpy().reshape(B, nt, nv).transpose(0, 2, 1), ref, 1e-13, "inverse_dynamics")
    rbd.dynamics_jvp_(out, s, nt, torques=dev(tau, s), dq=dq, dv=dv)
    ref = np.concatenate([J["aq"], J["av"]], axis=2)
    close(out.cpu().numpy().reshape(B, nt, nv).transpose(0, 2, 1), ref, 1e-13, "dynamics")


@pytest.mark.parametrize("name", ["atlas_floating", "valkyrie_floating", "mixed20"])
def test_fp32_against_fp64(rbd, oracle, models, name):
    flat = model(rbd, models, name)
    B, ntan = 64, 2
    q, v, tau = rand_inputs(rbd, flat, B, 51)
    rng = np.random.default_rng(6)
    vd = rng.standard_normal((B, flat.nv))
    dq, dv, dt = (rng.standard_normal((B, ntan * n)) for n in (flat.nq, flat.nv, flat.nv))
    # the fp64 side is the quad-precision oracle, not the library's fp64 kernels: an error shared by both GPU precisions does not cancel
    D = lambda a, n: a.reshape(B, ntan, n)
    a64 = oracle.jvp(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, None, D(dq, flat.nq), D(dv, flat.nv))
    b64 = oracle.jvp(flat, oracle.WHAT_DYNAMICS, q, v, tau, None, D(dq, flat.nq), D(dv, flat.nv), D(dt, flat.nv))
    s = make_state(rbd, flat, q, v, dtype=torch.float32)
    a = torch.zeros((B, flat.nv * ntan), dtype=torch.float32, device="cuda")
    b = torch.zeros_like(a)
    rbd.inverse_dynamics_jvp_(a, s, dev(vd, s), ntan, dq=dev(dq, s), dv=dev(dv, s))
    rbd.dynamics_jvp_(b, s, ntan, torques=dev(tau, s), dq=dev(dq, s), dv=dev(dv, s), dtorques=dev(dt, s))
    a32, b32 = a.double().cpu().numpy().reshape(B, ntan, -1), b.double().cpu().numpy().reshape(B, ntan, -1)
    for d in range(ntan):
        assert np.abs(a32[:, d] - a64[:, d]).max() <= 1e-4 * np.abs(a64[:, d]).max()
    # the dynamics! tangents: the cond-scaled forward-error criterion of tests/test_gpu_parity.py:26-35 (a solve with M), state by state
    M = oracle.mass_matrix(flat, q)
    kappa = np.linalg.cond(np.tril(M) + np.transpose(np.tril(M, -1), (0, 2, 1)))
    for d in range(ntan):
        err = np.linalg.norm(b32[:, d] - b64[:, d], axis=1) / np.maximum(np.linalg.norm(b64[:, d], axis=1), 1e-30)
        assert (err <= 8.0 * kappa * np.finfo(np.float32).eps * 10).all(), float((err / kappa).max())


def test_null_tangents_and_errors(rbd, models):
    flat = models["randmech1"]
    B = 8
    q, v, tau = rand_inputs(rbd, flat, B, 61)
    s = make_state(rbd, flat, q, v)
    out = torch.full((B, 2 * flat.nv), float("nan"), dtype=torch.float64, device="cuda")
    rbd.inverse_dynamics_jvp_(out, s, torch.zeros_like(s.v), 2)
    assert (out == 0).all()
    out.fill_(float("nan"))
    rbd.dynamics_jvp_(out, s, 2, torques=dev(tau, s))
    assert (out == 0).all()
    p = lambda t: rbd.state._ptr(t)
    L, opts = rbd._capi.lib(), s._opts()
    import ctypes
    assert L.rbd_inverse_dynamics_jvp(s.ws.handle, B, 0, p(s.q), p(s.v), p(s.v), None, None, None, None, None, None, p(out), ctypes.byref(opts)) == 1
    assert L.rbd_dynamics_jvp(s.ws.handle, B, -1, p(s.q), p(s.v), None, None, None, None, None, None, None, p(out), ctypes.byref(opts)) == 1
    with pytest.raises(ValueError):
        rbd.inverse_dynamics_jvp_(out, s, torch.zeros_like(s.v), 0)
    with pytest.raises(rbd.DimensionMismatch):  # shapes are checked before any launch
        rbd.dynamics_jvp_(out, s, 3)
    # loop joints: RBD_ERR_HAS_LOOPS (src/mechanism_algorithms.jl:549)
    fb = models["four_bar"]
    s4 = make_state(rbd, fb, *rand_inputs(rbd, fb, 2, 62)[:2])
    J = torch.zeros((2, fb.nv * fb.nq), dtype=torch.float64, device="cuda")
    for call in (lambda: rbd.inverse_dynamics_derivatives_(s4, torch.zeros_like(s4.v), J), lambda: rbd.dynamics_derivatives_(s4, None, J)):
        with pytest.raises(RuntimeError, match="tree Mechanisms"):
            call()
    # contact points with an environment: RBD_ERR_UNSUPPORTED, as rbd_dynamics
    rng = np.random.default_rng(63)
    mech = rbd.rand_tree_mechanism(rng, ["QuaternionFloating", "Revolute"])
    cm = rbd.SoftContactModel(rbd.hunt_crossley_hertz(), rbd.ViscoelasticCoulombModel(0.5, 1e3, 1e3))
    rbd.add_contact_point_(mech.bodies[-1], rbd.ContactPoint(np.zeros(3), cm))
    rbd.add_environment_primitive_(mech, rbd.HalfSpace3D([0, 0, 0], [0, 0, 1.0]))
    fc = rbd.flatten(mech)
    sc = make_state(rbd, fc, *rand_inputs(rbd, fc, 2, 64)[:2])
    with pytest.raises(rbd._capi.RBDError) as e:
        rbd.dynamics_derivatives_(sc, None, torch.zeros((2, fc.nv * fc.nq), dtype=torch.float64, device="cuda"))
    assert e.value.status == 3


def test_second_call_allocates_nothing(rbd, models):
    """The first derivative call of a workspace allocates its buffers; the next one (Jacobians and a JVP) does not."""
    flat = models["atlas_floating"]
    B = 256
    q, v, tau = rand_inputs(rbd, flat, B, 71)
    s = make_state(rbd, flat, q, v)
    nq, nv = flat.nq, flat.nv
    Aq = torch.zeros((B, nv * nq), dtype=torch.float64, device="cuda")
    Av, Ai = torch.zeros((B, nv * nv), dtype=torch.float64, device="cuda"), torch.zeros((B, nv * nv), dtype=torch.float64, device="cuda")
    t, dt, zv = dev(tau, s), dev(np.ones((B, 3 * nv)), s), torch.zeros_like(s.v)  # (every tensor of the test made before the measurement)
    out = torch.zeros((B, nv * 3), dtype=torch.float64, device="cuda")
    rbd.dynamics_derivatives_(s, t, Aq, Av, Ai)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    rbd.dynamics_derivatives_(s, t, Aq, Av, Ai)
    rbd.dynamics_jvp_(out, s, 3, torques=t, dtorques=dt)
    rbd.inverse_dynamics_derivatives_(s, zv, Aq)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
