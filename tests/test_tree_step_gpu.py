"""The three routes that share the per-state tree step (csrc/rbd_tree_step.hpp) compute the same τ: rbd_inverse_dynamics, tau_out of rbd_inverse_dynamics_jvp
(the tangent RNEA, one direction) and tau_out of rbd_inverse_dynamics_vjp (the adjoint RNEA), for the same states, external wrenches present, both layouts.
chain70 has more than 64 bodies, so its first route is big_rnea_kernel; mixed20 has every tree joint type.  B = 65: a full wavefront plus one lane (the
`slot >= nt` guards, the leading dimension of the scratch).  fp64: each against the oracle at the project's 1e-10 (1 + max|ref|) (derivative_parity.assert_no_solve);
fp32: each at the bound test_gpu_parity.test_rnea_crba_f32 holds inverse dynamics to, 2e-5 max|ref|."""
import numpy as np
import pytest
import torch

from conftest import rand_inputs
from derivative_parity import assert_no_solve, jvp_directions
from test_derivatives_gpu import dev, host, make_state, model

pytestmark = pytest.mark.gpu

MODELS = ["chain70", "mixed20"]
B = 65


@pytest.fixture(scope="module")
def case(rbd, oracle, models):
    """name -> (flat, q, v, v̇, f_ext, direction, λ, the oracle's τ), computed once per model."""
    cache = {}

    def get(name):
        if name not in cache:
            flat = model(rbd, models, name)
            q, v, _, fext = rand_inputs(rbd, flat, B, 31, fext=True)
            rng = np.random.default_rng(32)
            vd, lam = rng.standard_normal((B, flat.nv)), rng.standard_normal((B, flat.nv))
            cache[name] = (flat, q, v, vd, fext, jvp_directions(flat, B, 1), lam, oracle.inverse_dynamics(flat, q, v, vd, fext))
        return cache[name]
    return get


def three_routes(rbd, s, flat, vd, fext, d, lam, name):
    """τ by rbd_inverse_dynamics, by the tangent RNEA and by the adjoint RNEA, as host arrays [B, nv]."""
    nan = lambda: torch.full_like(s.v, float("nan"))
    vd_d, fe_d = dev(vd, s), dev(fext, s)
    t0, t1, t2 = nan(), nan(), nan()
    rbd.inverse_dynamics_(t0, s, vd_d, fe_d)
    assert ("big_" in rbd.last_kernel(s)) == (name == "chain70"), rbd.last_kernel(s)
    flat1 = lambda a: dev(a.reshape(B, -1), s)
    rbd.inverse_dynamics_jvp_(nan(), s, vd_d, 1, dq=flat1(d["q"]), dv=flat1(d["v"]), dvd=flat1(d["vd"]), externalwrenches=fe_d, dexternalwrenches=flat1(d["f"]),
                              torquesout=t1)
    assert "tangent" in rbd.last_kernel(s)
    rbd.inverse_dynamics_vjp_(s, vd_d, dev(lam, s), externalwrenches=fe_d, torquesout=t2)
    assert "adjoint" in rbd.last_kernel(s)
    return [("inverse_dynamics", host(t0, s)), ("jvp tau_out", host(t1, s)), ("vjp tau_out", host(t2, s))]


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", MODELS)
def test_three_routes_f64(rbd, case, name, layout):
    flat, q, v, vd, fext, d, lam, ref = case(name)
    s = make_state(rbd, flat, q, v, layout=layout)
    for what, got in three_routes(rbd, s, flat, vd, fext, d, lam, name):
        assert_no_solve(got, ref, name, "%s %s" % (what, layout))


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", MODELS)
def test_three_routes_f32(rbd, case, name, layout):
    flat, q, v, vd, fext, d, lam, ref = case(name)
    s = make_state(rbd, flat, q, v, dtype=torch.float32, layout=layout)
    for what, got in three_routes(rbd, s, flat, vd, fext, d, lam, name):
        err = np.abs(got - ref).max()
        print("observed %-10s %-28s err %.3e   bound %.3e" % (name, "%s %s f32" % (what, layout), err, 2e-5 * np.abs(ref).max()))
        assert err <= 2e-5 * np.abs(ref).max(), (name, what, layout, err, np.abs(ref).max())
