"""Reverse-mode derivatives of inverse_dynamics! and dynamics! on the GPU (header 700 additions: rbd_inverse_dynamics_vjp, rbd_dynamics_vjp, and the
torch.autograd functions of rigidbodydynamics.jl_amd/autograd.py): VJPs and backward() against Jᵀλ from the Jacobians of the quad-precision oracle (exact to
double rounding; the bounds: tests/derivative_parity.py), VJPs against Jᵀλ from the library's full Jacobians, the external-wrench pullback against JVPs,
values against the library's own calls, fp32 against fp64, the edge cases, allocation, gradcheck (reverse and forward mode) and loss.backward()."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rand_inputs
from derivative_parity import assert_no_solve, assert_solve_forward, cond_M
from test_derivatives_gpu import NV_OVER_64, close, dev, host, jacobians, make_state, model

pytestmark = pytest.mark.gpu

MODELS = ["atlas_floating", "valkyrie_floating", "mixed20", "inner_floating", "tree20", "chain70"]


def empty(s, n):
    shape = (s.batch, n) if s.layout == "aos" else (n, s.batch)
    return torch.full(shape, float("nan"), dtype=s.dtype, device="cuda")


def vjps(rbd, s, flat, vd, tau, lam, w, fext=None):
    """Both VJPs of one state batch: (q̄, v̄, v̇̄, f̄ext, τ) of inverse dynamics with cotangent lam, (q̄, v̄, τ̄, f̄ext, v̇) of dynamics with cotangent w."""
    nq, nv, nf = flat.nq, flat.nv, 6 * flat.n_bodies
    a = [empty(s, n) for n in (nq, nv, nv, nf, nv)]
    rbd.inverse_dynamics_vjp_(s, vd, dev(lam, s), a[0], a[1], a[2], externalwrenches=fext, fext_bar=a[3], torquesout=a[4])
    b = [empty(s, n) for n in (nq, nv, nv, nf, nv)]
    rbd.dynamics_vjp_(s, dev(w, s), tau, b[0], b[1], b[2], externalwrenches=fext, fext_bar=b[3], vdout=b[4])
    return [host(x, s) for x in a], [host(x, s) for x in b]


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", MODELS)
def test_vjp_equals_transposed_jacobians(rbd, models, name, layout):
    flat = model(rbd, models, name)
    B = 4096 if name == "atlas_floating" else 16
    q, v, tau = rand_inputs(rbd, flat, B, 81)
    rng = np.random.default_rng(8)
    vd = rng.standard_normal((B, flat.nv))
    lam, w = rng.standard_normal((B, flat.nv)), rng.standard_normal((B, flat.nv))
    s = make_state(rbd, flat, q, v, layout=layout)
    J = jacobians(rbd, s, flat, dev(vd, s), dev(tau, s))
    (qa, va, vda, _, ta), (qb, vb, tb, _, vdb) = vjps(rbd, s, flat, dev(vd, s), dev(tau, s), lam, w)
    assert "adjoint" in rbd.last_kernel(s)
    Tq = lambda X, y: np.einsum("bij,bi->bj", X, y)  # Xᵀ y per state
    close(qa, Tq(J["tq"], lam), 1e-10, "id q̄")
    close(va, Tq(J["tv"], lam), 1e-10, "id v̄")
    close(vda, Tq(J["M"], lam), 1e-10, "id v̇̄")
    close(qb, Tq(J["aq"], w), 1e-10, "dyn q̄")
    close(vb, Tq(J["av"], w), 1e-10, "dyn v̄")
    close(tb, Tq(J["Minv"], w), 1e-10, "dyn τ̄")
    # the values: τ = rbd_inverse_dynamics, v̇ = the CRBA route of rbd_dynamics
    t_ref = torch.zeros_like(s.v)
    rbd.inverse_dynamics_(t_ref, s, dev(vd, s))
    close(ta, host(t_ref, s), 1e-12, "tau")
    r = rbd.DynamicsResult(flat, B, layout=layout)
    rbd.dynamics_(r, s, dev(tau, s), algorithm="crba")
    close(vdb, host(r.vd, s), 1e-12, "vdot")


Tr = lambda X, y: np.einsum("bij,bi->bj", X, y)  # Xᵀ y per state


def quad_transposed(oracle, flat, q, v, vd, tau, fext, lam, w, wrench=False):
    """Jᵀλ of inverse dynamics and Jᵀw of dynamics formed in numpy from the quad-precision oracle's Jacobians: (q̄, v̄, v̇̄[, f̄ext]), (q̄, v̄, τ̄[, f̄ext]); the
    wrench part from its directional derivative along every wrench coordinate."""
    T = oracle.jacobians(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext)
    A = oracle.jacobians(flat, oracle.WHAT_DYNAMICS, q, v, tau, fext)
    a, b = [Tr(T[k], lam) for k in "qvx"], [Tr(A[k], w) for k in "qvx"]
    if wrench:
        E = np.tile(np.eye(6 * flat.n_bodies)[None], (q.shape[0], 1, 1))  # [b, wrench coordinate, :]
        a.append(np.einsum("bji,bi->bj", oracle.jvp(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext, dfext=E), lam))
        b.append(np.einsum("bji,bi->bj", oracle.jvp(flat, oracle.WHAT_DYNAMICS, q, v, tau, fext, dfext=E), w))
    return a, b


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", MODELS + NV_OVER_64)
def test_vjp_against_the_quad_oracle(rbd, oracle, models, name, layout):
    """(q̄, v̄, v̇̄ / τ̄, f̄ext) against Jᵀλ from the QUAD Jacobians, external wrenches present: inverse dynamics at 1e-10, dynamics state by state at the model's
    C · cond₂(M_b) · eps64 (profiles/derivative_parity.txt).  f̄ext on the small models (6 n_bodies more directions)."""
    flat = model(rbd, models, name)
    B = 8
    q, v, tau, fext = rand_inputs(rbd, flat, B, 11, fext=True)
    rng = np.random.default_rng(8)
    vd = rng.standard_normal((B, flat.nv))
    lam, w = rng.standard_normal((B, flat.nv)), rng.standard_normal((B, flat.nv))
    wrench = name in ("mixed20", "inner_floating")
    s = make_state(rbd, flat, q, v, layout=layout)
    (qa, va, vda, fa, _), (qb, vb, tb, fb, _) = vjps(rbd, s, flat, dev(vd, s), dev(tau, s), lam, w, fext=dev(fext, s))
    ra, rb = quad_transposed(oracle, flat, q, v, vd, tau, fext, lam, w, wrench)
    kappa = cond_M(oracle, flat, q)
    for key, got, ref in zip(("q̄", "v̄", "v̇̄", "f̄ext"), (qa, va, vda, fa), ra):
        assert_no_solve(got, ref, name, "vjp inverse_dynamics %s %s" % (key, layout))
    for key, got, ref in zip(("q̄", "v̄", "τ̄", "f̄ext"), (qb, vb, tb, fb), rb):
        assert_solve_forward(got, ref, kappa, name, "vjp dynamics %s %s" % (key, layout))


def test_loss_backward_against_the_quad_oracle(rbd, oracle, models):
    """loss.backward() through both autograd functions, external wrenches among the leaves, against Jᵀw from the quad Jacobians."""
    name = "mixed20"
    flat = models[name]
    B = 8
    q, v, tau, fext = rand_inputs(rbd, flat, B, 11, fext=True)
    rng = np.random.default_rng(14)
    vd, w = rng.standard_normal((B, flat.nv)), rng.standard_normal((B, flat.nv))
    s = make_state(rbd, flat, q, v)
    ra, rb = quad_transposed(oracle, flat, q, v, vd, tau, fext, w, w, True)
    leaf = lambda a: dev(a, s).requires_grad_(True)
    Q, V, A, F, W = leaf(q), leaf(v), leaf(vd), leaf(fext), dev(w, s)
    (W * rbd.autograd.inverse_dynamics(s, Q, V, A, F)).sum().backward()
    for key, t, ref in zip(("q", "v", "v̇", "f_ext"), (Q, V, A, F), ra):
        assert_no_solve(host(t.grad, s), ref, name, "backward inverse_dynamics " + key)
    Q, V, T, F = leaf(q), leaf(v), leaf(tau), leaf(fext)
    (W * rbd.autograd.dynamics(s, Q, V, T, F, algorithm="crba")).sum().backward()
    kappa = cond_M(oracle, flat, q)
    for key, t, ref in zip(("q", "v", "τ", "f_ext"), (Q, V, T, F), rb):
        assert_solve_forward(host(t.grad, s), ref, kappa, name, "backward dynamics " + key)


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", ["atlas_floating", "mixed20", "chain70"])
def test_wrench_pullback_against_jvp(rbd, models, name, layout):
    """f̄ext (and everything else at once) by the dot-product identity ⟨λ, J d⟩ = ⟨Jᵀλ, d⟩ with the JVPs, external wrenches present."""
    flat = model(rbd, models, name)
    B = 64
    q, v, tau, fext = rand_inputs(rbd, flat, B, 91, fext=True)
    rng = np.random.default_rng(9)
    vd = rng.standard_normal((B, flat.nv))
    lam, w = rng.standard_normal((B, flat.nv)), rng.standard_normal((B, flat.nv))
    d = {k: rng.standard_normal((B, n)) for k, n in (("q", flat.nq), ("v", flat.nv), ("a", flat.nv), ("f", 6 * flat.n_bodies))}
    s = make_state(rbd, flat, q, v, layout=layout)
    F = dev(fext, s)
    (qa, va, vda, fa, _), (qb, vb, tb, fb, _) = vjps(rbd, s, flat, dev(vd, s), dev(tau, s), lam, w, fext=F)
    jv = empty(s, flat.nv)
    rbd.inverse_dynamics_jvp_(jv, s, dev(vd, s), 1, dq=dev(d["q"], s), dv=dev(d["v"], s), dvd=dev(d["a"], s), externalwrenches=F, dexternalwrenches=dev(d["f"], s))
    lhs = np.sum(lam * host(jv, s), axis=1)
    terms = [qa * d["q"], va * d["v"], vda * d["a"], fa * d["f"]]
    mag = sum(np.abs(t).sum(axis=1) for t in terms)
    assert (np.abs(lhs - sum(t.sum(axis=1) for t in terms)) <= 1e-10 * mag).all()
    rbd.dynamics_jvp_(jv, s, 1, torques=dev(tau, s), dq=dev(d["q"], s), dv=dev(d["v"], s), dtorques=dev(d["a"], s), externalwrenches=F,
                      dexternalwrenches=dev(d["f"], s))
    lhs = np.sum(w * host(jv, s), axis=1)
    terms = [qb * d["q"], vb * d["v"], tb * d["a"], fb * d["f"]]
    mag = sum(np.abs(t).sum(axis=1) for t in terms)
    assert (np.abs(lhs - sum(t.sum(axis=1) for t in terms)) <= 1e-10 * mag).all()


@pytest.mark.parametrize("name", ["atlas_floating", "valkyrie_floating", "mixed20"])
def test_fp32_against_fp64(rbd, oracle, models, name):
    flat = model(rbd, models, name)
    B = 64
    q, v, tau = rand_inputs(rbd, flat, B, 101)
    rng = np.random.default_rng(10)
    vd = rng.standard_normal((B, flat.nv))
    lam, w = rng.standard_normal((B, flat.nv)), rng.standard_normal((B, flat.nv))
    # the fp64 side is Jᵀλ from the quad-precision oracle's Jacobians, not the library's fp64 kernels: an error shared by both GPU precisions does not cancel
    a64, b64 = quad_transposed(oracle, flat, q, v, vd, tau, None, lam, w)
    s = make_state(rbd, flat, q, v, dtype=torch.float32)
    a32, b32 = vjps(rbd, s, flat, dev(vd, s), dev(tau, s), lam, w)
    for k in range(3):  # q̄, v̄, v̇̄ of inverse dynamics
        assert np.abs(a32[k] - a64[k]).max() <= 1e-4 * np.abs(a64[k]).max(), k
    # dynamics: a solve with M — the cond-scaled forward-error criterion of tests/test_gpu_parity.py:26-35, state by state
    M = oracle.mass_matrix(flat, q)
    kappa = np.linalg.cond(np.tril(M) + np.transpose(np.tril(M, -1), (0, 2, 1)))
    for k in range(3):  # q̄, v̄, τ̄
        err = np.linalg.norm(b32[k] - b64[k], axis=1) / np.maximum(np.linalg.norm(b64[k], axis=1), 1e-30)
        assert (err <= 8.0 * kappa * np.finfo(np.float32).eps * 10).all(), (k, float((err / kappa).max()))


def test_null_outputs_errors_and_empty_batch(rbd, models):
    flat = models["randmech1"]
    B = 8
    q, v, tau = rand_inputs(rbd, flat, B, 111)
    s = make_state(rbd, flat, q, v)
    lam = torch.ones_like(s.v)
    # every output nullable: only the value
    t = empty(s, flat.nv)
    rbd.inverse_dynamics_vjp_(s, torch.zeros_like(s.v), lam, torquesout=t)
    t_ref = torch.zeros_like(s.v)
    rbd.inverse_dynamics_(t_ref, s, torch.zeros_like(s.v))
    assert torch.allclose(t, t_ref, rtol=1e-12, atol=1e-12)
    vd = empty(s, flat.nv)
    rbd.dynamics_vjp_(s, lam, torques=dev(tau, s), vdout=vd)
    assert torch.isfinite(vd).all()
    tb = empty(s, flat.nv)  # τ̄ alone (no adjoint pass)
    rbd.dynamics_vjp_(s, lam, torques=dev(tau, s), tau_bar=tb)
    assert torch.isfinite(tb).all()
    p = lambda x: rbd.state._ptr(x)
    L, opts = rbd._capi.lib(), s._opts()
    out = empty(s, flat.nq)
    # NULL q, v, cotangent, or v̇ (inverse dynamics): RBD_ERR_INVALID_ARGUMENT
    assert L.rbd_inverse_dynamics_vjp(s.ws.handle, B, None, p(s.v), p(s.v), None, p(lam), None, p(out), None, None, None, ctypes.byref(opts)) == 1
    assert L.rbd_inverse_dynamics_vjp(s.ws.handle, B, p(s.q), p(s.v), None, None, p(lam), None, p(out), None, None, None, ctypes.byref(opts)) == 1
    assert L.rbd_inverse_dynamics_vjp(s.ws.handle, B, p(s.q), p(s.v), p(s.v), None, None, None, p(out), None, None, None, ctypes.byref(opts)) == 1
    assert L.rbd_dynamics_vjp(s.ws.handle, B, p(s.q), None, None, None, p(lam), None, p(out), None, None, None, ctypes.byref(opts)) == 1
    assert L.rbd_dynamics_vjp(s.ws.handle, B, p(s.q), p(s.v), None, None, None, None, p(out), None, None, None, ctypes.byref(opts)) == 1
    # B == 0: a successful no-op
    out.fill_(float("nan"))
    assert L.rbd_inverse_dynamics_vjp(s.ws.handle, 0, p(s.q), p(s.v), p(s.v), None, p(lam), None, p(out), None, None, None, ctypes.byref(opts)) == 0
    assert L.rbd_dynamics_vjp(s.ws.handle, 0, p(s.q), p(s.v), None, None, p(lam), None, p(out), None, None, None, ctypes.byref(opts)) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    # RBD_MEM_HOST: RBD_ERR_UNSUPPORTED
    hopts = rbd._capi.Opts(rbd._capi.LAYOUT_AOS, rbd._capi.MEM_HOST, 0, 1)
    assert L.rbd_inverse_dynamics_vjp(s.ws.handle, B, p(s.q), p(s.v), p(s.v), None, p(lam), None, p(out), None, None, None, ctypes.byref(hopts)) == 3
    with pytest.raises(rbd.DimensionMismatch):  # shapes are checked before any launch
        rbd.dynamics_vjp_(s, lam, q_bar=torch.zeros((B, flat.nq + 1), dtype=torch.float64, device="cuda"))
    # loop joints: RBD_ERR_HAS_LOOPS
    fb = models["four_bar"]
    s4 = make_state(rbd, fb, *rand_inputs(rbd, fb, 2, 112)[:2])
    for call in (lambda: rbd.inverse_dynamics_vjp_(s4, torch.zeros_like(s4.v), torch.ones_like(s4.v), torch.zeros_like(s4.q)),
                 lambda: rbd.dynamics_vjp_(s4, torch.ones_like(s4.v), None, torch.zeros_like(s4.q))):
        with pytest.raises(RuntimeError, match="tree Mechanisms"):
            call()
    # contact points with an environment: RBD_ERR_UNSUPPORTED
    rng = np.random.default_rng(113)
    mech = rbd.rand_tree_mechanism(rng, ["QuaternionFloating", "Revolute"])
    cm = rbd.SoftContactModel(rbd.hunt_crossley_hertz(), rbd.ViscoelasticCoulombModel(0.5, 1e3, 1e3))
    rbd.add_contact_point_(mech.bodies[-1], rbd.ContactPoint(np.zeros(3), cm))
    rbd.add_environment_primitive_(mech, rbd.HalfSpace3D([0, 0, 0], [0, 0, 1.0]))
    fc = rbd.flatten(mech)
    sc = make_state(rbd, fc, *rand_inputs(rbd, fc, 2, 114)[:2])
    with pytest.raises(rbd._capi.RBDError) as e:
        rbd.dynamics_vjp_(sc, torch.ones_like(sc.v), None, torch.zeros_like(sc.q))
    assert e.value.status == 3


def test_second_call_allocates_nothing(rbd, models):
    flat = models["atlas_floating"]
    B = 256
    q, v, tau = rand_inputs(rbd, flat, B, 121)
    s = make_state(rbd, flat, q, v)
    nq, nv, nf = flat.nq, flat.nv, 6 * flat.n_bodies
    t, lam, zv = dev(tau, s), torch.ones_like(s.v), torch.zeros_like(s.v)  # (every tensor of the test made before the measurement)
    qb, vb, ab, fb = (torch.zeros((B, n), dtype=torch.float64, device="cuda") for n in (nq, nv, nv, nf))
    rbd.dynamics_vjp_(s, lam, t, qb, vb, ab, fext_bar=fb)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    rbd.dynamics_vjp_(s, lam, t, qb, vb, ab, fext_bar=fb)
    rbd.inverse_dynamics_vjp_(s, zv, lam, qb, vb, ab, fext_bar=fb)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0


def on_manifold(rbd, flat, q):
    """q with every quaternion (and SinCosRevolute (s, c)) normalised, differentiably in torch."""
    parts, k = [], 0
    for jt, off, n in zip(flat.joint_type, flat.q_offset, np.diff(np.append(flat.q_offset, flat.nq))):
        if off > k:
            parts.append(q[:, k:off])
        m = 4 if jt in (rbd.mechanism.JOINT_QUAT_FLOATING, rbd.mechanism.JOINT_QUAT_SPHERICAL) else 2 if jt == rbd.mechanism.JOINT_SINCOS_REVOLUTE else 0
        if m:
            parts.append(q[:, off:off + m] / q[:, off:off + m].norm(dim=1, keepdim=True))
            k = off + m
        else:
            k = off
    parts.append(q[:, k:])
    return torch.cat(parts, dim=1)


@pytest.mark.parametrize("name", ["double_pendulum", "mixed20", "inner_floating"])
def test_gradcheck(rbd, models, name):
    """torch.autograd.gradcheck in fp64, reverse and forward mode, through both functions: raw q, so finite differences apply as they stand — to
    inverse_dynamics and to the CRBA route of dynamics, the function whose derivatives the library takes.  The articulated-body route is a different
    function of q off the unit sphere of a quaternion: its check runs with the quaternions normalised in torch (derivatives along the sphere)."""
    flat = models[name]
    B = 3
    q, v, tau, fext = rand_inputs(rbd, flat, B, 131, fext=True)
    vd = np.random.default_rng(13).standard_normal((B, flat.nv))
    s = rbd.MechanismState(flat, B)
    g = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda *a: rbd.autograd.inverse_dynamics(s, *a), (g(q), g(v), g(vd), g(fext)), check_forward_ad=True)
    args = (g(q), g(v), g(tau), g(fext))
    assert torch.autograd.gradcheck(lambda *a: rbd.autograd.dynamics(s, *a, algorithm="crba"), args, check_forward_ad=True)
    assert torch.autograd.gradcheck(lambda qq, *a: rbd.autograd.dynamics(s, on_manifold(rbd, flat, qq), *a), args, check_forward_ad=True)
    # (without the optional inputs)
    assert torch.autograd.gradcheck(lambda qq, vv: rbd.autograd.dynamics(s, qq, vv, algorithm="crba"), (g(q), g(v)), check_forward_ad=True)


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_loss_backward_on_atlas(rbd, models, layout):
    """loss.backward() through both functions at 4096 Atlas states against Jᵀw from the full Jacobians."""
    flat = models["atlas_floating"]
    B = 4096
    q, v, tau = rand_inputs(rbd, flat, B, 141)
    rng = np.random.default_rng(14)
    vd = rng.standard_normal((B, flat.nv))
    w = rng.standard_normal((B, flat.nv))
    s = make_state(rbd, flat, q, v, layout=layout)
    J = jacobians(rbd, s, flat, dev(vd, s), dev(tau, s))
    leaf = lambda a: dev(a, s).requires_grad_(True)
    Q, V, A, T, W = leaf(q), leaf(v), leaf(vd), leaf(tau), dev(w, s)
    (W * rbd.autograd.inverse_dynamics(s, Q, V, A)).sum().backward()
    Tq = lambda X, y: np.einsum("bij,bi->bj", X, y)
    close(host(Q.grad, s), Tq(J["tq"], w), 1e-10, "id q")
    close(host(V.grad, s), Tq(J["tv"], w), 1e-10, "id v")
    close(host(A.grad, s), Tq(J["M"], w), 1e-10, "id v̇")
    Q.grad = V.grad = None
    out = rbd.autograd.dynamics(s, Q, V, T)
    close(host(out.detach(), s), J["vd"], 1e-9, "dynamics value (ABA against CRBA)")
    (W * out).sum().backward()
    close(host(Q.grad, s), Tq(J["aq"], w), 1e-10, "dyn q")
    close(host(V.grad, s), Tq(J["av"], w), 1e-10, "dyn v")
    close(host(T.grad, s), Tq(J["Minv"], w), 1e-10, "dyn τ")
