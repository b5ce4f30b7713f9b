"""Pins of the quad-precision oracle (oracle/rbd_oracle_q.c), the reference of the derivative tests — no GPU.  It is the fp64 oracle's program text instantiated
in IEEE binary128, so its values must round to the fp64 oracle's; its difference quotients must not depend on the step (exactness) and must equal the closed-form
derivative of the reference's closed-form double pendulum (test/test_double_pendulum.jl:41-65, the known answers of tests/test_oracle_pins.py); ∂τ/∂v̇ must be
the mass matrix; and the two dynamics routes must have one derivative along the unit spheres."""
import numpy as np
import pytest

from conftest import rand_inputs

TREES = ["atlas_floating", "atlas_fixed", "acrobot_urdf", "valkyrie_floating", "double_pendulum", "quickstart_pendulum", "randmech1", "randmech2", "randmech3",
         "inner_floating", "mixed20", "limbs_humanoid", "limbs_only_children", "limbs_quadruped", "limbs_three"]
ALL = TREES + ["four_bar"]  # (its tree part: the batch drivers do not see loop joints)


def test_every_model_is_covered(models):
    assert sorted(ALL) == sorted(models)


def rel(a, ref):
    return np.abs(a - ref).max() / (1 + np.abs(ref).max())


@pytest.mark.parametrize("name", ALL)
def test_quad_values_round_to_the_fp64_oracle(oracle, models, rbd, name):
    """Within 1e-12 of 1 + max|ref| (the fp64 oracle's own rounding through the solve; the largest measured is 2.2e-13, dynamics of Atlas)."""
    flat = models[name]
    B = 8
    q, v, tau, fext = rand_inputs(rbd, flat, B, 11, fext=True)
    vd = np.random.default_rng(3).standard_normal((B, flat.nv))
    for what, x in ((oracle.WHAT_INVERSE_DYNAMICS, vd), (oracle.WHAT_DYNAMICS, tau), (oracle.WHAT_ABA, tau), (oracle.WHAT_DYNAMICS_BIAS, None)):
        ref = oracle.quad_values(flat, what, q, v, x, fext)
        assert rel(oracle.batch(flat, what, q, v, x, fext), ref) <= 1e-12, what
    assert rel(oracle.mass_matrix(flat, q), oracle.quad_values(flat, oracle.WHAT_MASS_MATRIX, q)) <= 1e-12
    # the value that the derivative drivers return beside the derivative is the same one
    val, _ = oracle.jvp(flat, oracle.WHAT_DYNAMICS, q, v, tau, fext, dv=np.ones_like(v), want_value=True)
    assert np.array_equal(val, oracle.quad_values(flat, oracle.WHAT_DYNAMICS, q, v, tau, fext))


@pytest.mark.parametrize("name", TREES)
def test_quotient_does_not_depend_on_the_step(oracle, models, rbd, name):
    """Exactness of both schemes: the result at h and at 3h agree to 1e-14 of the scale, and the 2-point quotient at 1e-11 agrees with the 4-point one at 1e-7."""
    flat = models[name]
    B = 2
    rng = np.random.default_rng(3)
    q, v, tau, fext = rand_inputs(rbd, flat, B, 11, fext=True)
    vd = rng.standard_normal((B, flat.nv))
    d = [rng.standard_normal((B, n)) for n in (flat.nq, flat.nv, flat.nv, 6 * flat.n_bodies)]  # (dq off every quaternion's unit sphere)
    for what, x in ((oracle.WHAT_INVERSE_DYNAMICS, vd), (oracle.WHAT_DYNAMICS, tau), (oracle.WHAT_ABA, tau)):
        at = lambda h, points: oracle.jvp(flat, what, q, v, x, fext, *d, h=h, points=points)
        a = at(oracle.QUAD_H, 2)
        assert rel(at(3 * oracle.QUAD_H, 2), a) <= 1e-14, (what, "2-point")
        b = at(1e-7, 4)
        assert rel(at(3e-7, 4), b) <= 1e-14, (what, "4-point")
        assert rel(b, a) <= 1e-14, (what, "2-point against 4-point")


def closed_form_derivatives(q, v, vd, lc1=-0.5, l1=-1.0, m1=1.0, I1=0.333, lc2=-1.0, m2=1.0, I2=1.33, g=-9.81):
    """∂τ/∂q, ∂τ/∂v, ∂τ/∂v̇ of τ = M(q) v̇ + C(q, v) v + G(q) with M, C, G of test/test_double_pendulum.jl:41-65 (test_oracle_pins.closed_form), by hand."""
    (q1, q2), (v1, v2), (a1, a2) = q, v, vd
    k = m2 * l1 * lc2
    c1, c2, s2, c12 = np.cos(q1), np.cos(q2), np.sin(q2), np.cos(q1 + q2)
    M = np.array([[I1 + I2 + m2 * l1 ** 2 + 2 * k * c2, I2 + k * c2], [I2 + k * c2, I2]])
    Tq = np.array([[m1 * g * lc1 * c1 + m2 * g * (l1 * c1 + lc2 * c12), -2 * k * s2 * a1 - k * s2 * a2 - 2 * k * c2 * v1 * v2 - k * c2 * v2 ** 2 + m2 * g * lc2 * c12],
                   [m2 * g * lc2 * c12, -k * s2 * a1 + k * c2 * v1 ** 2 + m2 * g * lc2 * c12]])
    Tv = np.array([[-2 * k * s2 * v2, -2 * k * s2 * (v1 + v2)], [2 * k * s2 * v1, 0.0]])
    return Tq, Tv, M


@pytest.mark.parametrize("name", ["double_pendulum", "acrobot_urdf"])
def test_double_pendulum_closed_form_derivatives(oracle, models, name):
    """1e-12 absolute, the atol of the reference's closed-form test: the closed form is evaluated in fp64 here (sums of terms of size ~20)."""
    flat = models[name]
    rng = np.random.default_rng(6)
    B = 16
    q, v, vd, tau = rng.standard_normal((B, 2)), rng.random((B, 2)), rng.random((B, 2)), rng.random((B, 2))
    J = oracle.jacobians(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd)
    A = oracle.jacobians(flat, oracle.WHAT_DYNAMICS, q, v, tau)
    for b in range(B):
        Tq, Tv, M = closed_form_derivatives(q[b], v[b], vd[b])
        for got, ref in ((J["q"][b], Tq), (J["v"][b], Tv), (J["x"][b], M)):
            assert np.abs(got - ref).max() <= 1e-12
        # v̇ = M⁻¹ (τ − C v − G): ∂v̇/∂· = −M⁻¹ ∂τ/∂· at that v̇, ∂v̇/∂τ = M⁻¹ (2 × 2, cond(M) < 20)
        Tq, Tv, M = closed_form_derivatives(q[b], v[b], A["val"][b])
        for got, ref in ((A["q"][b], -np.linalg.solve(M, Tq)), (A["v"][b], -np.linalg.solve(M, Tv)), (A["x"][b], np.linalg.inv(M))):
            assert np.abs(got - ref).max() <= 1e-12 * (1 + np.abs(ref).max())


@pytest.mark.parametrize("name", ["atlas_floating", "randmech2", "inner_floating", "mixed20", "limbs_humanoid"])
def test_jacobian_in_vdot_is_the_mass_matrix(oracle, models, rbd, name):
    """test/test_mechanism_algorithms.jl:600-614 on the quad Jacobian driver, and its columns against the directional driver."""
    flat = models[name]
    B = 2
    q, v, tau, fext = rand_inputs(rbd, flat, B, 21, fext=True)
    vd = np.random.default_rng(4).standard_normal((B, flat.nv))
    J = oracle.jacobians(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext)
    Mo = oracle.mass_matrix(flat, q)
    Ms = np.tril(Mo) + np.transpose(np.tril(Mo, -1), (0, 2, 1))
    assert rel(J["x"], Ms) <= 1e-12
    assert np.array_equal(J["val"], oracle.quad_values(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext))
    for key, n, arg in (("q", flat.nq, "dq"), ("v", flat.nv, "dv"), ("x", flat.nv, "dx")):
        E = np.tile(np.eye(n)[None], (B, 1, 1))  # [b, direction, coordinate]
        cols = oracle.jvp(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext, **{arg: E})
        assert np.array_equal(np.transpose(cols, (0, 2, 1)), J[key]), key
    # ∂τ/∂f_ext along the wrench of body b: −(the joint's share of it); a linear map, so the directional driver must be additive in the wrench
    rng = np.random.default_rng(5)
    f1, f2 = rng.standard_normal((2, B, 6 * flat.n_bodies))
    parts = oracle.jvp(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext, dfext=f1) + oracle.jvp(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext, dfext=f2)
    assert rel(oracle.jvp(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext, dfext=f1 + f2), parts) <= 1e-14


def tangent_to_the_spheres(rbd, flat, q, dq):
    """dq with its radial part removed on every quaternion and every SinCosRevolute (s, c) pair."""
    dq = dq.copy()
    J = rbd.mechanism
    for jt, off in zip(flat.joint_type, flat.q_offset):
        n = 4 if jt in (J.JOINT_QUAT_FLOATING, J.JOINT_QUAT_SPHERICAL) else 2 if jt == J.JOINT_SINCOS_REVOLUTE else 0
        if n:
            u = q[:, off:off + n] / np.linalg.norm(q[:, off:off + n], axis=1, keepdims=True)
            dq[:, off:off + n] -= u * np.sum(u * dq[:, off:off + n], axis=1, keepdims=True)
    return dq


@pytest.mark.parametrize("name", ["atlas_floating", "randmech1", "randmech2", "randmech3", "inner_floating", "mixed20"])
def test_aba_and_dynamics_have_one_derivative_on_the_unit_spheres(oracle, models, rbd, name):
    """The articulated-body route and the reference's route are one function of unit quaternions (another one off the sphere), so along directions tangent to
    the spheres their quad derivatives agree.  q is on the sphere only to fp64 rounding (‖q‖ = 1 ± 1e-16), which the two routes answer differently in the
    radial direction: 1e-12 of the scale leaves room for that offset times the second derivative; both quotients themselves are exact."""
    flat = models[name]
    B = 4
    rng = np.random.default_rng(7)
    q, v, tau, fext = rand_inputs(rbd, flat, B, 31, fext=True)
    dq = tangent_to_the_spheres(rbd, flat, q, rng.standard_normal((B, flat.nq)))
    d = [dq] + [rng.standard_normal((B, n)) for n in (flat.nv, flat.nv, 6 * flat.n_bodies)]
    a = oracle.jvp(flat, oracle.WHAT_DYNAMICS, q, v, tau, fext, *d)
    b = oracle.jvp(flat, oracle.WHAT_ABA, q, v, tau, fext, *d)
    assert rel(b, a) <= 1e-12
