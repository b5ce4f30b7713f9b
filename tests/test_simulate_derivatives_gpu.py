"""Derivatives of simulate steps on the GPU (rbd_simulate_jvp, rbd_simulate_step_derivatives): one-step tangents against a Richardson central difference of
oracle/simulate_np.py step (and of rbd_simulate for wrench directions and whole batches), the singular starting points of quaternion joints, Jacobian
columns against JVPs, several steps against chained steps and products of step Jacobians, fp32 against fp64, the edge cases and the allocation policy."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rand_inputs

pytestmark = pytest.mark.gpu

FD_MODELS = ["atlas_floating", "atlas_fixed", "double_pendulum", "randmech1", "randmech2", "randmech3", "inner_floating", "mixed20", "chain70"]
H = 1e-3
DT = 5e-3


def central_difference(f):
    """f'(0): 4th-order central differences at h = 1e-3 and h / 2, Richardson-combined."""
    d = lambda h: (8 * (f(h) - f(-h)) - (f(2 * h) - f(-2 * h))) / (12 * h)
    return (16 * d(H / 2) - d(H)) / 15


def model(rbd, models, name):
    if name == "chain70":  # a tree of more than 64 bodies: the any-size tables
        return rbd.flatten(rbd.rand_tree_mechanism(np.random.default_rng(70), ["QuaternionFloating"] + ["Revolute", "Prismatic", "SinCosRevolute", "Revolute"] * 17 + ["Revolute"]))
    return models[name]


@pytest.fixture(scope="module")
def sim(oracle):
    import simulate_np
    return simulate_np


def dev(a, layout, dtype=torch.float64):
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)
    return (t if layout == "aos" else t.t().contiguous()).cuda()


def host(t, layout):
    t = t.detach().double().cpu()
    return (t if layout == "aos" else t.t()).numpy().copy()


def make_state(rbd, flat, q, v, dtype=torch.float64, layout="aos"):
    s = rbd.MechanismState(flat, q.shape[0], dtype=dtype, layout=layout)
    rbd.set_configuration_(s, q)
    rbd.set_velocity_(s, v)
    return s


def close(got, ref, tol, what=""):
    err = np.abs(got - ref).max()
    assert np.isfinite(got).all(), what
    assert err <= tol * (1 + np.abs(ref).max()), (what, err, np.abs(ref).max())


def jvp(rbd, flat, q, v, tau, dq, dv, dtau=None, fext=None, dfext=None, nsteps=1, dt=DT, layout="aos", dtype=torch.float64):
    """(q, v after the steps, dq, dv after the steps) with (B, ntan, n) directions."""
    B, ntan = dq.shape[:2]
    s = make_state(rbd, flat, q, v, dtype=dtype, layout=layout)
    f = lambda a: None if a is None else dev(a.reshape(B, -1), layout, dtype)
    tq, tv = f(dq), f(dv)
    rbd.simulate_jvp_(tq, tv, s, ntan, dt, nsteps, torques=f(tau), dtorques=f(dtau), externalwrenches=f(fext), dexternalwrenches=f(dfext))
    assert "tangent_mk_stage_kernel" in rbd.last_kernel(s)
    return host(s.q, layout), host(s.v, layout), host(tq, layout).reshape(B, ntan, -1), host(tv, layout).reshape(B, ntan, -1)


def gpu_simulate(rbd, flat, q, v, tau, fext=None, nsteps=1, dt=DT, layout="aos", dtype=torch.float64):
    s = make_state(rbd, flat, q, v, dtype=dtype, layout=layout)
    rbd.simulate_(s, (nsteps - 0.5) * dt, dt=dt, torques=dev(tau, layout, dtype), externalwrenches=None if fext is None else dev(fext, layout, dtype))
    return host(s.q, layout), host(s.v, layout)


def oracle_step(sim, flat, q, v, tau, dt=DT):
    out = [sim.step(flat, q[b], v[b], dt, tau[b]) for b in range(q.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", FD_MODELS)
def test_jvp_against_central_difference(rbd, sim, models, name, layout):
    flat = model(rbd, models, name)
    B, ntan = 3, 3
    rng = np.random.default_rng(3)
    q, v, tau = rand_inputs(rbd, flat, B, 11)
    dq = rng.standard_normal((B, ntan, flat.nq))  # (not projected on any quaternion's unit sphere: raw-coordinate derivatives)
    dv = rng.standard_normal((B, ntan, flat.nv))
    dtau = rng.standard_normal((B, ntan, flat.nv))
    dq[:, 1] = 0  # (direction 1: v and τ only; direction 2: q alone)
    dv[:, 2] = 0
    dtau[:, 2] = 0
    q1, v1, gq, gv = jvp(rbd, flat, q, v, tau, dq, dv, dtau, layout=layout)
    rq, rv = oracle_step(sim, flat, q, v, tau)
    close(q1, rq, 1e-10, "q")
    close(v1, rv, 1e-10, "v")
    for d in range(ntan):
        ref = central_difference(lambda h: np.concatenate(oracle_step(sim, flat, q + h * dq[:, d], v + h * dv[:, d], tau + h * dtau[:, d]), axis=1))
        close(np.concatenate([gq[:, d], gv[:, d]], axis=1), ref, 1e-6, (name, d))


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", ["atlas_floating", "mixed20"])
def test_wrench_directions(rbd, models, name, layout):
    """dfext (held over the step, as fext is) against a central difference of rbd_simulate itself."""
    flat = model(rbd, models, name)
    B, ntan = 8, 2
    rng = np.random.default_rng(13)
    q, v, tau, fext = rand_inputs(rbd, flat, B, 12, fext=True)
    dfe = rng.standard_normal((B, ntan, 6 * flat.n_bodies))
    dq = np.zeros((B, ntan, flat.nq))
    dv = np.zeros((B, ntan, flat.nv))
    dv[:, 1] = rng.standard_normal((B, flat.nv))
    _, _, gq, gv = jvp(rbd, flat, q, v, tau, dq, dv, fext=fext, dfext=dfe, layout=layout)
    for d in range(ntan):
        ref = central_difference(lambda h: np.concatenate(gpu_simulate(rbd, flat, q, v + h * dv[:, d], tau, fext + h * dfe[:, d], layout=layout), axis=1))
        close(np.concatenate([gq[:, d], gv[:, d]], axis=1), ref, 1e-6, (name, d))


@pytest.mark.parametrize("case", ["rest", "no_rotation"])
@pytest.mark.parametrize("name", ["atlas_floating", "inner_floating"])
def test_singular_starting_points(rbd, sim, models, name, case):
    """From rest (v = 0), and with every floating joint at ω = 0 and a nonzero linear velocity: the later stages have a rotation of exactly zero with a
    nonzero derivative, where the reference's small-angle branches would drop first-order terms.  Every direction moves the angular velocities (dθ ≠ 0): along
    a curve on which a stage's relative rotation stays exactly zero, the reference's log takes its branch for every h and drops ½ q_v × ω from the value
    (rbd_simulate's value too, O(dt²) here), so a difference quotient there would measure the branch, not the step.  The state keeps that value (it is
    rbd_simulate's), and the tangents of the smooth map are carried along it: an O(dt³) departure from the smooth map's own trajectory, far below the
    tolerance at the step of the other checks."""
    flat = model(rbd, models, name)
    B, ntan = 3, 3
    rng = np.random.default_rng(17)
    q, v, tau = rand_inputs(rbd, flat, B, 18)
    if case == "rest":
        v[:] = 0
    else:
        for i in range(flat.n_bodies):
            if int(flat.joint_type[i]) == sim.FLOATING:
                vo = int(flat.v_offset[i])
                v[:, vo:vo + 3] = 0
    dq = rng.standard_normal((B, ntan, flat.nq))
    dv = rng.standard_normal((B, ntan, flat.nv))
    dtau = rng.standard_normal((B, ntan, flat.nv))
    dq[:, 1] = 0
    dtau[:, 2] = 0
    q1, v1, gq, gv = jvp(rbd, flat, q, v, tau, dq, dv, dtau)
    assert np.isfinite(gq).all() and np.isfinite(gv).all()
    rq, rv = oracle_step(sim, flat, q, v, tau)
    close(q1, rq, 1e-10, "q")
    close(v1, rv, 1e-10, "v")
    for d in range(ntan):
        ref = central_difference(lambda h: np.concatenate(oracle_step(sim, flat, q + h * dq[:, d], v + h * dv[:, d], tau + h * dtau[:, d]), axis=1))
        close(np.concatenate([gq[:, d], gv[:, d]], axis=1), ref, 1e-6, (name, case, d))


def step_jacobians(rbd, flat, q, v, tau, layout="aos", dt=DT, dtype=torch.float64, which=(True, True)):
    B, nx, nv = q.shape[0], flat.nq + flat.nv, flat.nv
    s = make_state(rbd, flat, q, v, dtype=dtype, layout=layout)
    z = lambda n: dev(np.full((B, n), np.nan), layout, dtype)
    A, Bt = z(nx * nx) if which[0] else None, z(nx * nv) if which[1] else None
    rbd.simulate_step_derivatives_(s, dt, torques=dev(tau, layout, dtype), dx_dx=A, dx_dtau=Bt)
    assert "tangent_mk_stage_kernel" in rbd.last_kernel(s)
    J = lambda t, cols: None if t is None else rbd.jacobian_view(t, s, nx, cols).double().cpu().numpy()
    return host(s.q, layout), host(s.v, layout), J(A, nx), J(Bt, nv)


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", ["atlas_floating", "inner_floating", "mixed20", "chain70"])
def test_jacobian_columns_are_jvps(rbd, models, name, layout):
    flat = model(rbd, models, name)
    B, nq, nv = 4, flat.nq, flat.nv
    nx = nq + nv
    q, v, tau = rand_inputs(rbd, flat, B, 41)
    q1, v1, A, Bt = step_jacobians(rbd, flat, q, v, tau, layout)
    E = np.eye(nx + nv)
    nt = nx + nv
    dq = np.tile(E[:nq].T[None], (B, 1, 1))
    dv = np.tile(E[nq:nx].T[None], (B, 1, 1))
    dtau = np.tile(E[nx:].T[None], (B, 1, 1))
    jq, jv, gq, gv = jvp(rbd, flat, q, v, tau, dq, dv, dtau, layout=layout)
    assert gq.shape == (B, nt, nq)
    ref = np.concatenate([gq, gv], axis=2).transpose(0, 2, 1)  # (B, nx, nt)
    close(A, ref[:, :, :nx], 1e-12, "dx_dx")
    close(Bt, ref[:, :, nx:], 1e-12, "dx_dtau")
    np.testing.assert_array_equal(q1, jq)
    np.testing.assert_array_equal(v1, jv)
    # one output alone: the same columns
    _, _, A2, none = step_jacobians(rbd, flat, q, v, tau, layout, which=(True, False))
    assert none is None
    np.testing.assert_array_equal(A2, A)
    _, _, none, B2 = step_jacobians(rbd, flat, q, v, tau, layout, which=(False, True))
    np.testing.assert_array_equal(B2, Bt)


@pytest.mark.parametrize("name", ["atlas_floating", "mixed20"])
def test_several_steps(rbd, sim, models, name):
    flat = model(rbd, models, name)
    B, ntan = 4, 2
    nx = flat.nq + flat.nv
    rng = np.random.default_rng(23)
    q, v, tau = rand_inputs(rbd, flat, B, 24)
    dq = rng.standard_normal((B, ntan, flat.nq))
    dv = rng.standard_normal((B, ntan, flat.nv))
    dtau = rng.standard_normal((B, ntan, flat.nv))
    q3, v3, gq3, gv3 = jvp(rbd, flat, q, v, tau, dq, dv, dtau, nsteps=3)
    # three chained one-step JVPs (τ and its direction held)
    qc, vc, cq, cv = q, v, dq, dv
    prod = np.tile(np.eye(nx)[None], (B, 1, 1))
    Bsum = np.zeros((B, nx, flat.nv))
    for _ in range(3):
        qn, vn, A, Bt = step_jacobians(rbd, flat, qc, vc, tau)
        prod = np.einsum("bij,bjk->bik", A, prod)
        Bsum = np.einsum("bij,bjk->bik", A, Bsum) + Bt
        qc, vc, cq, cv = jvp(rbd, flat, qc, vc, tau, cq, cv, dtau)
        close(qn, qc, 1e-13, "q of the Jacobian call")
    close(np.concatenate([gq3, gv3], axis=2), np.concatenate([cq, cv], axis=2), 1e-10, "chained")
    x0 = np.concatenate([dq, dv], axis=2)
    ref = np.einsum("bij,bdj->bdi", prod, x0) + np.einsum("bij,bdj->bdi", Bsum, dtau)
    close(np.concatenate([gq3, gv3], axis=2), ref, 1e-10, "product of step Jacobians")
    # the state: rbd_simulate to rounding, and the oracle
    sq, sv = gpu_simulate(rbd, flat, q, v, tau, nsteps=3)
    close(q3, sq, 1e-11, "q vs rbd_simulate")
    close(v3, sv, 1e-11, "v vs rbd_simulate")
    oq, ov = q, v
    for _ in range(3):
        oq, ov = oracle_step(sim, flat, oq, ov, tau)
    close(q3, oq, 1e-10, "q vs oracle")
    close(v3, ov, 1e-10, "v vs oracle")


def test_whole_batch(rbd, models):
    """Atlas floating, 4096 fp64 states, one random direction each, against a central difference built from rbd_simulate on the same GPU."""
    flat = models["atlas_floating"]
    B = 4096
    rng = np.random.default_rng(29)
    q, v, tau = rand_inputs(rbd, flat, B, 30)
    dq = rng.standard_normal((B, 1, flat.nq))
    dv = rng.standard_normal((B, 1, flat.nv))
    dtau = rng.standard_normal((B, 1, flat.nv))
    # (the base quaternion's direction tangent to its unit sphere: the difference quotient of rbd_simulate then stays on unit quaternions, where its
    #  kernels are held to the oracle)
    qr, dr = q[:, 0:4], dq[:, 0, 0:4]
    dq[:, 0, 0:4] = dr - np.sum(qr * dr, axis=1, keepdims=True) * qr
    q1, v1, gq, gv = jvp(rbd, flat, q, v, tau, dq, dv, dtau, layout="soa")
    sq, sv = gpu_simulate(rbd, flat, q, v, tau, layout="soa")
    close(q1, sq, 1e-11, "q")
    close(v1, sv, 1e-11, "v")
    ref = central_difference(lambda h: np.concatenate(gpu_simulate(rbd, flat, q + h * dq[:, 0], v + h * dv[:, 0], tau + h * dtau[:, 0], layout="soa"), axis=1))
    close(np.concatenate([gq[:, 0], gv[:, 0]], axis=1), ref, 1e-6, "whole batch")


@pytest.mark.parametrize("name", ["atlas_floating", "mixed20"])
def test_fp32_against_fp64(rbd, oracle, models, name):
    flat = model(rbd, models, name)
    B, ntan = 64, 2
    rng = np.random.default_rng(31)
    q, v, tau = rand_inputs(rbd, flat, B, 32)
    dq, dv, dtau = (rng.standard_normal((B, ntan, n)) for n in (flat.nq, flat.nv, flat.nv))
    r64 = jvp(rbd, flat, q, v, tau, dq, dv, dtau)
    r32 = jvp(rbd, flat, q, v, tau, dq, dv, dtau, dtype=torch.float32)
    M = oracle.mass_matrix(flat, q)
    kappa = np.linalg.cond(np.tril(M) + np.transpose(np.tril(M, -1), (0, 2, 1)))
    bound = 8.0 * kappa * np.finfo(np.float32).eps * 10  # (the criterion of tests/test_derivatives_gpu.py test_fp32_against_fp64, state by state)
    for d in range(ntan):
        x64 = np.concatenate([r64[2][:, d], r64[3][:, d]], axis=1)
        x32 = np.concatenate([r32[2][:, d], r32[3][:, d]], axis=1)
        assert np.isfinite(x32).all()
        err = np.linalg.norm(x32 - x64, axis=1) / np.maximum(np.linalg.norm(x64, axis=1), 1e-30)
        assert (err <= bound).all(), float((err / kappa).max())
    A64 = step_jacobians(rbd, flat, q, v, tau)[2]
    A32 = step_jacobians(rbd, flat, q, v, tau, dtype=torch.float32)[2]
    err = np.linalg.norm(A32 - A64, axis=(1, 2)) / np.linalg.norm(A64, axis=(1, 2))
    assert (err <= bound).all(), float((err / kappa).max())


def test_errors_and_no_ops(rbd, models):
    flat = models["randmech1"]
    B = 8
    q, v, tau = rand_inputs(rbd, flat, B, 61)
    s = make_state(rbd, flat, q, v)
    L, opts = rbd._capi.lib(), s._opts()
    p = lambda t: rbd.state._ptr(t)
    dq = torch.randn((B, 2 * flat.nq), dtype=torch.float64, device="cuda")
    dv = torch.randn((B, 2 * flat.nv), dtype=torch.float64, device="cuda")
    h = s.ws.handle
    INV = 1
    call = lambda ntan, dt, nsteps, a=dq, b=dv: L.rbd_simulate_jvp(h, B, ntan, p(s.q), p(s.v), None, None, ctypes.c_double(dt), nsteps, p(a), p(b), None, None,
                                                                 ctypes.byref(opts))
    assert call(0, DT, 1) == INV and call(-1, DT, 1) == INV
    assert call(2, 0.0, 1) == INV and call(2, -1e-3, 1) == INV
    assert call(2, DT, -1) == INV
    assert L.rbd_simulate_jvp(h, B, 2, p(s.q), p(s.v), None, None, ctypes.c_double(DT), 1, None, p(dv), None, None, ctypes.byref(opts)) == INV
    assert L.rbd_simulate_jvp(h, B, 2, p(s.q), p(s.v), None, None, ctypes.c_double(DT), 1, p(dq), None, None, None, ctypes.byref(opts)) == INV
    assert L.rbd_simulate_jvp(h, B, 2, None, p(s.v), None, None, ctypes.c_double(DT), 1, p(dq), p(dv), None, None, ctypes.byref(opts)) == INV
    assert L.rbd_simulate_step_derivatives(h, B, p(s.q), p(s.v), None, None, ctypes.c_double(0.0), None, None, ctypes.byref(opts)) == INV
    with pytest.raises(ValueError):
        rbd.simulate_jvp_(dq, dv, s, 0, DT)
    with pytest.raises(rbd.DimensionMismatch):  # shapes are checked before any launch
        rbd.simulate_jvp_(dq, dv, s, 3, DT)
    # nsteps = 0 and B = 0: nothing changes
    before = [t.clone() for t in (s.q, s.v, dq, dv)]
    assert call(2, DT, 0) == 0
    assert L.rbd_simulate_jvp(h, 0, 2, p(s.q), p(s.v), None, None, ctypes.c_double(DT), 1, p(dq), p(dv), None, None, ctypes.byref(opts)) == 0
    torch.cuda.synchronize()
    for a, b in zip(before, (s.q, s.v, dq, dv)):
        assert torch.equal(a, b)
    # NULL Jacobian outputs: the step alone
    q1, v1, _, _ = step_jacobians(rbd, flat, q, v, tau, which=(False, False))
    rq, rv, _, _ = step_jacobians(rbd, flat, q, v, tau)
    np.testing.assert_array_equal(q1, rq)
    np.testing.assert_array_equal(v1, rv)
    # host memory: RBD_ERR_UNSUPPORTED (device pointers only)
    qh, vh = np.ascontiguousarray(q), np.ascontiguousarray(v)
    dqh, dvh = np.zeros((B, 2 * flat.nq)), np.zeros((B, 2 * flat.nv))
    hopts = s._opts()
    hopts.memory = rbd._capi.MEM_HOST
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.rbd_simulate_jvp(h, B, 2, hp(qh), hp(vh), None, None, ctypes.c_double(DT), 1, hp(dqh), hp(dvh), None, None, ctypes.byref(hopts)) == 3
    assert L.rbd_simulate_step_derivatives(h, B, hp(qh), hp(vh), None, None, ctypes.c_double(DT), None, None, ctypes.byref(hopts)) == 3
    # loop joints: RBD_ERR_HAS_LOOPS
    fb = models["four_bar"]
    s4 = make_state(rbd, fb, *rand_inputs(rbd, fb, 2, 62)[:2])
    with pytest.raises(RuntimeError, match="tree Mechanisms"):
        rbd.simulate_step_derivatives_(s4, DT, dx_dx=torch.zeros((2, (fb.nq + fb.nv) ** 2), dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError, match="tree Mechanisms"):
        rbd.simulate_jvp_(torch.zeros((2, fb.nq), dtype=torch.float64, device="cuda"), torch.zeros((2, fb.nv), dtype=torch.float64, device="cuda"), s4, 1, DT)
    # contact points with an environment: RBD_ERR_UNSUPPORTED
    rng = np.random.default_rng(63)
    mech = rbd.rand_tree_mechanism(rng, ["QuaternionFloating", "Revolute"])
    cm = rbd.SoftContactModel(rbd.hunt_crossley_hertz(), rbd.ViscoelasticCoulombModel(0.5, 1e3, 1e3))
    rbd.add_contact_point_(mech.bodies[-1], rbd.ContactPoint(np.zeros(3), cm))
    rbd.add_environment_primitive_(mech, rbd.HalfSpace3D([0, 0, 0], [0, 0, 1.0]))
    fc = rbd.flatten(mech)
    sc = make_state(rbd, fc, *rand_inputs(rbd, fc, 2, 64)[:2])
    with pytest.raises(rbd._capi.RBDError) as e:
        rbd.simulate_step_derivatives_(sc, DT)
    assert e.value.status == 3
    with pytest.raises(rbd._capi.RBDError) as e:
        rbd.simulate_jvp_(torch.zeros((2, fc.nq), dtype=torch.float64, device="cuda"), torch.zeros((2, fc.nv), dtype=torch.float64, device="cuda"), sc, 1, DT)
    assert e.value.status == 3


def test_second_call_allocates_nothing(rbd, models):
    """The first call of a workspace allocates; the next ones (Jacobians, a JVP with fewer directions, several steps) do not."""
    flat = models["atlas_floating"]
    B = 256
    nx, nv = flat.nq + flat.nv, flat.nv
    q, v, tau = rand_inputs(rbd, flat, B, 71)
    s = make_state(rbd, flat, q, v)
    t = dev(tau, "aos")
    A = torch.zeros((B, nx * nx), dtype=torch.float64, device="cuda")
    Bt = torch.zeros((B, nx * nv), dtype=torch.float64, device="cuda")
    dq = torch.zeros((B, 3 * flat.nq), dtype=torch.float64, device="cuda")
    dv = torch.ones((B, 3 * nv), dtype=torch.float64, device="cuda")
    rbd.simulate_step_derivatives_(s, DT, torques=t, dx_dx=A, dx_dtau=Bt)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    rbd.simulate_step_derivatives_(s, DT, torques=t, dx_dx=A, dx_dtau=Bt)
    rbd.simulate_jvp_(dq, dv, s, 3, DT, 2, torques=t)
    rbd.simulate_step_derivatives_(s, DT, torques=t, dx_dtau=Bt)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
