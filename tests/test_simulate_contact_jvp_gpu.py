"""Forward mode through simulate steps with soft contact on the GPU (rbd_simulate_contact_jvp, rbd_simulate_contact_step_derivatives).  The reference is exact
and independent of the code under test: the merged reverse mode through the same steps (rbd_simulate_contact_vjp — itself held at 1e-10 to torch autograd of
the composition of merged parts by test_simulate_contact_vjp_gpu.py).  The step Jacobians assembled from its rows (unit cotangents of (q⁺; v⁺; s⁺)) must equal
the Jacobians assembled from forward-mode columns, and ⟨cotangent, J·d⟩ = ⟨Jᵀ·cotangent, d⟩ state by state over several steps.  No difference quotients.
Tolerances: 1e-10·(1 + max|ref|) between the forward and the reverse route in fp64, 1e-12·(1 + max|ref|) between two runs of the forward route."""
import ctypes

import numpy as np
import pytest
import torch

import contact_model_ref as cm
from conftest import tune
from test_contact_vjp_gpu import close, cond_bound, dev, host, interpreting_kernels, walker_inputs, walker_pair, with_contact  # noqa: F401 (the fixture is autouse)
from test_contact_jvp_gpu import adjoint_identity, nan
from test_simulate_contact_vjp_gpu import Reference, all_margins, atlas_with_feet, big_tree, branches, cotangents, gpu_positions, stages

pytestmark = pytest.mark.gpu
DT = 1e-3
STAGE_KERNEL = "tangent_contact_stage_kernel"


def dims(flat):
    return flat.nq, flat.nv, flat.ns, flat.nq + flat.nv + flat.ns


def jacobians(rbd, flat, B, q, v, s, tau, fext, dt=DT, layout="aos", dtype=torch.float64, state=None, want=(True, True)):
    """One rbd_simulate_contact_step_derivatives call on NaN-prefilled outputs: A = ∂x⁺/∂x (B, nx, nx), B = ∂x⁺/∂τ (B, nx, nv) (None where not asked for) and
    the state after the step, fp64 numpy."""
    nq, nv, ns, nx = dims(flat)
    st = state or rbd.MechanismState(flat, B, dtype=dtype, layout=layout)
    D = lambda x: None if x is None else dev(x, layout, dtype)
    A = nan(B, nx * nx, layout, dtype) if want[0] else None
    Bt = nan(B, nx * nv, layout, dtype) if want[1] else None
    qd, vd, sd = D(q), D(v), D(s)
    rbd.simulate_contact_step_derivatives_(st, dt, D(tau), A, Bt, D(fext), q=qd, v=vd, s=sd)
    assert rbd.sync(st) == 0 and STAGE_KERNEL in rbd.last_kernel(st)
    M = lambda t, cols: None if t is None else host(t, layout).reshape(B, cols, nx).transpose(0, 2, 1)  # (column-major per state)
    return M(A, nx), M(Bt, nv), (host(qd, layout), host(vd, layout), host(sd, layout))


def jvp(rbd, flat, B, ntan, q, v, s, tau, fext, dq, dv, ds, dtau, dfext, nsteps=1, dt=DT, layout="aos", dtype=torch.float64, state=None):
    """One rbd_simulate_contact_jvp call; tangents (B, ntan, n) numpy in and out (dtau, dfext may be None), and the final state."""
    st = state or rbd.MechanismState(flat, B, dtype=dtype, layout=layout)
    D = lambda x: None if x is None else dev(x, layout, dtype)
    T = lambda x: None if x is None else D(x[:, :ntan].reshape(B, -1))
    tq, tv, ts = T(dq), T(dv), T(ds)
    qd, vd, sd = D(q), D(v), D(s)
    rbd.simulate_contact_jvp_(tq, tv, ts, st, ntan, dt, nsteps, torques=D(tau), dtorques=T(dtau), externalwrenches=D(fext), dexternalwrenches=T(dfext),
                              q=qd, v=vd, s=sd)
    assert rbd.sync(st) == 0
    if nsteps > 0:
        assert STAGE_KERNEL in rbd.last_kernel(st)
    return [host(t, layout).reshape(B, ntan, -1) for t in (tq, tv, ts)], (host(qd, layout), host(vd, layout), host(sd, layout))


def vjp_rows(rbd, flat, B, q, v, s, tau, fext, dt=DT, dtype=torch.float64):
    """[A B] by rows: nx one-step rbd_simulate_contact_vjp calls with unit cotangents of (q⁺; v⁺; s⁺) — q̄, v̄, s̄ give the row of A, τ̄ that of B — and the state
    after the step."""
    nq, nv, ns, nx = dims(flat)
    st = rbd.MechanismState(flat, B, dtype=dtype)
    D = lambda x: dev(x, dtype=dtype)
    q0, v0, s0, td, fd = D(q), D(v), D(s), D(tau), D(fext)
    A, Bt = np.full((B, nx, nx), np.nan), np.full((B, nx, nv), np.nan)
    for i in range(nx):
        cot = [torch.zeros(B, n, dtype=dtype, device="cuda") for n in (nq, nv, ns)]
        blk, k = (0, i) if i < nq else ((1, i - nq) if i < nq + nv else (2, i - nq - nv))
        cot[blk][:, k] = 1
        tb = nan(B, nv, dtype=dtype)
        qd, vd, sd = q0.clone(), v0.clone(), s0.clone()
        rbd.simulate_contact_vjp_(*cot, st, dt, 1, torques=td, externalwrenches=fd, tau_bar=tb, q=qd, v=vd, s=sd)
        A[:, i, :] = np.concatenate([host(c) for c in cot], axis=1)
        Bt[:, i, :] = host(tb)
    assert rbd.sync(st) == 0
    return A, Bt, (host(qd), host(vd), host(sd))


def directions(flat, B, ntan, rng):
    return [rng.standard_normal((B, ntan, n)) for n in (flat.nq, flat.nv, flat.ns, flat.nv, 6 * flat.n_bodies)]


def apply(A, Bt, dx, dtau):
    """[A B]·(dx; dτ) per state and direction; dx (B, ntan, nx)"""
    return np.einsum("brc,bdc->bdr", A, dx) + np.einsum("brc,bdc->bdr", Bt, dtau)


def split(flat, dx):
    nq, nv, ns, _ = dims(flat)
    return dx[..., :nq], dx[..., nq:nq + nv], dx[..., nq + nv:]


def one_vjp(rbd, flat, B, q, v, s, tau, fext, cot, nsteps, dt=DT):
    """One nsteps-step rbd_simulate_contact_vjp call: (q̄, v̄, s̄, τ̄, f̄ext) and the final state."""
    st = rbd.MechanismState(flat, B)
    qb, vb, sb = (dev(x) for x in cot)
    tb, fb = nan(B, flat.nv), nan(B, 6 * flat.n_bodies)
    qd, vd, sd = dev(q), dev(v), dev(s)
    rbd.simulate_contact_vjp_(qb, vb, sb, st, dt, nsteps, torques=dev(tau), externalwrenches=dev(fext), tau_bar=tb, fext_bar=fb, q=qd, v=vd, s=sd)
    assert rbd.sync(st) == 0
    return [host(x) for x in (qb, vb, sb, tb, fb)], (host(qd), host(vd), host(sd))


@pytest.fixture(scope="module")
def walker130(rbd, oracle, interpreting_kernels):
    """The walker, B = 130, the states of test_simulate_contact_vjp_gpu.py (seed 5): the pair info of a 3-step reference rollout, [A B] of the first step by
    rows of rbd_simulate_contact_vjp (45 calls) and by one forward call, five random directions (computed once, shared, left unchanged)."""
    flat, bare = walker_pair(rbd)
    B = 130
    rng, q, v, s, tau, fext = walker_inputs(rbd, flat, B, seed=5)
    cot = cotangents(flat, B, rng)
    _, _, infos = Reference(rbd, flat, bare, B).run(q, v, s, tau, fext, cot, 3)
    A, Bt, final = vjp_rows(rbd, flat, B, q, v, s, tau, fext)
    Af, Bf, ffinal = jacobians(rbd, flat, B, q, v, s, tau, fext)
    return dict(flat=flat, bare=bare, B=B, inputs=(q, v, s, tau, fext), cot=cot, infos=infos, A=A, Bt=Bt, final=final, Af=Af, Bf=Bf, ffinal=ffinal,
                d=directions(flat, B, 5, rng), rng=rng)


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_walker_step_jacobians_against_vjp_rows(rbd, walker130, layout):
    """dx_dx and dx_dtau of one call at 1e-10·(1 + max|ref|) of the 45 rows of rbd_simulate_contact_vjp, on states whose pairs are clear of the branch
    boundaries at every stage of the step (asserted from the reference rollout) and cover every branch; q⁺, v⁺, s⁺ at 1e-12 of the VJP's advanced state."""
    w = walker130
    assert dims(w["flat"]) == (11, 10, 24, 45)
    assert bool(all_margins(w["infos"][:1], 1e-6).all())
    assert min(cm.coverage(w["infos"][0][0])) >= 0.05
    A, Bt, final = jacobians(rbd, w["flat"], w["B"], *w["inputs"], layout=layout)
    close(A, w["A"], 1e-10, "dx_dx")
    close(Bt, w["Bt"], 1e-10, "dx_dtau")
    for name, g, r in zip("qvs", final, w["final"]):
        close(g, r, 1e-12, name + "+")


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("ntan", [5, 1])
def test_jacobian_columns_are_jvps(rbd, walker130, ntan, layout):
    """A one-step rbd_simulate_contact_jvp with random (dq, dv, ds, dτ), dfext NULL, equals [A B]·directions of the forward call at 1e-12; ntan = 5 and 1 leave
    the last chunk partly filled (fp64 chunks hold 2 directions; the 55 columns of the fp32 Jacobians in test_fp32_against_fp64 end in a chunk of 3 of 4)."""
    w = walker130
    dq, dv, ds, dtau, _ = [x[:, :ntan] for x in w["d"]]
    got, final = jvp(rbd, w["flat"], w["B"], ntan, *w["inputs"], dq, dv, ds, dtau, None, layout=layout)
    ref = split(w["flat"], apply(w["Af"], w["Bf"], np.concatenate([dq, dv, ds], axis=2), dtau))
    for name, g, r in zip(("dq+", "dv+", "ds+"), got, ref):
        close(g, r, 1e-12, name)
    for name, g, r in zip("qvs", final, w["ffinal"]):
        close(g, r, 1e-12, name + "+")


def adjoint_case(rbd, flat, B, q, v, s, tau, fext, nsteps, ntan, rng, tol, what):
    """⟨a, dq⁺⟩ + ⟨b, dv⁺⟩ + ⟨c, ds⁺⟩ = ⟨q̄, dq⟩ + ⟨v̄, dv⟩ + ⟨s̄, ds⟩ + ⟨τ̄, dτ⟩ + ⟨f̄ext, dfext⟩ per state, all five inputs live, the bars from ONE
    rbd_simulate_contact_vjp call over the same steps; the two routes' final states at the same tolerance."""
    cot = cotangents(flat, B, rng)
    d = directions(flat, B, ntan, rng)
    bars, vfinal = one_vjp(rbd, flat, B, q, v, s, tau, fext, cot, nsteps)
    got, final = jvp(rbd, flat, B, ntan, q, v, s, tau, fext, *d, nsteps=nsteps)
    adjoint_identity(got, cot, bars, d, tol, what)
    assert all(np.abs(g).max() > 0 for g in got)
    for name, g, r in zip("qvs", final, vfinal):
        close(g, r, 1e-12, name + "+")


def test_adjoint_identity_walker(rbd, walker130):
    """The walker, B = 130, 3 steps (the steps whose margins test_simulate_contact_vjp_gpu.py::test_walker_conditions_hold asserts; re-asserted), ntan = 5."""
    w = walker130
    assert bool(all_margins(w["infos"], 1e-6).all())
    adjoint_case(rbd, w["flat"], w["B"], *w["inputs"], 3, 5, np.random.default_rng(77), 1e-10, "walker, 3 steps")


def test_adjoint_identity_atlas_floating(rbd, oracle, models):
    """Atlas on a floating base with test_atlas_floating's feet and floor, B = 67, 2 steps, at cond_bound."""
    bare = models["atlas_floating"]
    B = 67
    rng = np.random.default_rng(23)
    flat, q, v = atlas_with_feet(rbd, bare, B, rng, gpu_positions(rbd, bare, B))
    s = 1e-3 * rng.standard_normal((B, flat.ns))
    tau, fext = rng.random((B, flat.nv)), rng.random((B, 6 * flat.n_bodies))
    adjoint_case(rbd, flat, B, q, v, s, tau, fext, 2, 3, rng, cond_bound(oracle, bare, q), "atlas, 2 steps")


def test_adjoint_identity_tree_of_more_than_64_bodies(rbd, oracle):
    """The 70-body tree, B = 8, 2 steps, at cond_bound: the any-size route of the value path."""
    (flat, rng), (bare, _) = big_tree(rbd, False), big_tree(rbd, True)
    assert flat.n_bodies == 70 and flat.ns == 9
    B = 8
    q, v = rbd.rand_configuration(flat, B, rng), rbd.rand_velocity(flat, B, rng)
    s = 1e-3 * rng.standard_normal((B, flat.ns))
    tau, fext = rng.random((B, flat.nv)), rng.random((B, 6 * flat.n_bodies))
    adjoint_case(rbd, flat, B, q, v, s, tau, fext, 2, 3, rng, cond_bound(oracle, bare, q), "70 bodies, 2 steps")


def test_chaining(rbd, walker130):
    """One 3-step JVP call equals three 1-step calls chained (state and tangents, dτ and dfext held) at 1e-12, and the product of the three step Jacobians
    taken along the trajectory applied to the directions with dτ held (dfext NULL) at 1e-10."""
    w = walker130
    flat, B = w["flat"], 32
    q, v, s, tau, fext = (x[:B].copy() for x in w["inputs"])
    d = [x[:B].copy() for x in w["d"]]
    st = rbd.MechanismState(flat, B)
    one, final = jvp(rbd, flat, B, 5, q, v, s, tau, fext, *d, nsteps=3, state=st)
    x, t = (q, v, s), d[:3]
    for _ in range(3):
        t, x = jvp(rbd, flat, B, 5, *x, tau, fext, *t, d[3], d[4], state=st)
    for name, g, r in zip(("dq+", "dv+", "ds+", "q+", "v+", "s+"), list(t) + list(x), one + list(final)):
        close(g, r, 1e-12, name)
    one, _ = jvp(rbd, flat, B, 5, q, v, s, tau, fext, d[0], d[1], d[2], d[3], None, nsteps=3, state=st)
    x, dx = (q, v, s), np.concatenate(d[:3], axis=2)
    for _ in range(3):
        A, Bt, x = jacobians(rbd, flat, B, *x, tau, fext, state=st)
        dx = apply(A, Bt, dx, d[3])
    for name, g, r in zip(("dq+", "dv+", "ds+"), one, split(flat, dx)):
        close(g, r, 1e-10, name + " (product)")


def test_no_contact_anywhere_is_rbd_simulate_jvp(rbd, walker130):
    """The walker 5 m clear of both half-spaces, B = 16, 2 steps: dq⁺, dv⁺ and the (q; v) blocks of A, B equal rbd_simulate_jvp / rbd_simulate_step_derivatives
    on the bare model at 1e-12; ∂s⁺/∂s = I; ∂s⁺/∂(q, v, τ) and ∂(q⁺, v⁺)/∂s are exact zeros."""
    w = walker130
    flat, bare, B = w["flat"], w["bare"], 16
    nq, nv, ns, nx = dims(flat)
    q, v, s, tau, fext = (x[:B].copy() for x in w["inputs"])
    d = [x[:B].copy() for x in w["d"]]
    nrm = np.array([h["outward_normal"] / np.linalg.norm(h["outward_normal"]) for h in flat.halfspaces])
    assert nrm[0] @ nrm[1] > 0  # (moving along the sum of the normals leaves both half-spaces)
    q[:, 4:7] += flat.pred_rot[0].T @ (5.0 * nrm.sum(axis=0))
    _, _, infos = Reference(rbd, flat, bare, B).run(q, v, s, tau, fext, cotangents(flat, B, np.random.default_rng(3)), 2)
    assert not any(bool(i["inside"].any()) for i in stages(infos)) and min(float(i["sep"].min()) for i in stages(infos)) > 1.0
    got, final = jvp(rbd, flat, B, 5, q, v, s, tau, fext, *d, nsteps=2)
    st = rbd.MechanismState(bare, B)
    T = lambda x: dev(x.reshape(B, -1))
    tq, tv = T(d[0]), T(d[1])
    rbd.set_configuration_(st, q)
    rbd.set_velocity_(st, v)
    rbd.simulate_jvp_(tq, tv, st, 5, DT, 2, torques=dev(tau), dtorques=T(d[3]), externalwrenches=dev(fext), dexternalwrenches=T(d[4]))
    close(got[0], host(tq).reshape(B, 5, nq), 1e-12, "dq+")
    close(got[1], host(tv).reshape(B, 5, nv), 1e-12, "dv+")
    close(final[0], host(st.q), 1e-12, "q+")
    close(final[1], host(st.v), 1e-12, "v+")
    assert np.array_equal(got[2], d[2]) and np.array_equal(final[2], s)  # (every pair outside at every stage: ṡ = 0 and dṡ = 0 exactly)
    A, Bt, _ = jacobians(rbd, flat, B, q, v, s, tau, fext)
    rbd.set_configuration_(st, q)
    rbd.set_velocity_(st, v)
    n2 = nq + nv
    Ab, Bb = nan(B, n2 * n2), nan(B, n2 * nv)
    rbd.simulate_step_derivatives_(st, DT, dev(tau), Ab, Bb, dev(fext))
    close(A[:, :n2, :n2], host(Ab).reshape(B, n2, n2).transpose(0, 2, 1), 1e-12, "A (q; v)")
    close(Bt[:, :n2], host(Bb).reshape(B, nv, n2).transpose(0, 2, 1), 1e-12, "B (q; v)")
    assert np.array_equal(A[:, n2:, n2:], np.broadcast_to(np.eye(ns), (B, ns, ns)))
    assert (A[:, n2:, :n2] == 0).all() and (Bt[:, n2:] == 0).all() and (A[:, :n2, n2:] == 0).all()


def pass_bytes(flat, B, width, es=8):
    """RBD_TUNE sim_tan_bytes for passes of `width` directions: 2·nq + 6·nv + 4·ns tangent values per direction and state"""
    nq, nv, ns, _ = dims(flat)
    return es * (2 * nq + 6 * nv + 4 * ns) * B * width


def test_several_passes(rbd, walker130, monkeypatch):
    """RBD_TUNE sim_tan_bytes for passes of 20 directions (workspaces made under that setting): the 55 unit directions take 3 passes at B = 130, the last of 15;
    A, B and the final state equal the single-pass call bit for bit.  The same with passes of 4 for a JVP with ntan = 7 (two passes, the second of 3)."""
    w = walker130
    flat, B = w["flat"], w["B"]
    d7 = directions(flat, B, 7, np.random.default_rng(9))
    ref7, rfinal7 = jvp(rbd, flat, B, 7, *w["inputs"], *d7)
    tune(monkeypatch, sim_tan_bytes=pass_bytes(flat, B, 20))
    assert -(-(45 + 10) // 20) >= 3
    A, Bt, final = jacobians(rbd, flat, B, *w["inputs"])
    assert np.array_equal(A, w["Af"]) and np.array_equal(Bt, w["Bf"])
    for g, r in zip(final, w["ffinal"]):
        assert np.array_equal(g, r)
    tune(monkeypatch, sim_tan_bytes=pass_bytes(flat, B, 4))
    got7, final7 = jvp(rbd, flat, B, 7, *w["inputs"], *d7)
    for g, r in zip(got7 + list(final7), ref7 + list(rfinal7)):
        assert np.isfinite(g).all() and np.array_equal(g, r)


def test_partial_outputs_and_null_inputs(rbd, walker130):
    """Only dx_dx, only dx_dtau; τ / fext NULL against explicit zeros; dτ / dfext NULL against explicit zero directions — each at 1e-12 of the full call."""
    w = walker130
    flat, B, (q, v, s, tau, fext) = w["flat"], w["B"], w["inputs"]
    st = rbd.MechanismState(flat, B)
    A, Bt, final = jacobians(rbd, flat, B, q, v, s, tau, fext, state=st, want=(True, False))
    assert Bt is None
    close(A, w["Af"], 1e-12, "dx_dx alone")
    A, Bt, final2 = jacobians(rbd, flat, B, q, v, s, tau, fext, state=st, want=(False, True))
    assert A is None
    close(Bt, w["Bf"], 1e-12, "dx_dtau alone")
    _, _, final3 = jacobians(rbd, flat, B, q, v, s, tau, fext, state=st, want=(False, False))  # (neither: the state is still advanced)
    for name, a, b, c, r in zip("qvs", final, final2, final3, w["ffinal"]):
        close(a, r, 1e-12, name + "+"); close(b, r, 1e-12, name + "+"); close(c, r, 1e-12, name + "+")
    for tn, fn in ((None, fext), (tau, None), (None, None)):
        z = lambda x, like: np.zeros_like(like) if x is None else x
        ref = jacobians(rbd, flat, B, q, v, s, z(tn, tau), z(fn, fext), state=st)
        got = jacobians(rbd, flat, B, q, v, s, tn, fn, state=st)
        for name, g, r in zip(("dx_dx", "dx_dtau"), got[:2], ref[:2]):
            close(g, r, 1e-12, name + " (NULL tau / fext)")
    d = w["d"]
    full, _ = jvp(rbd, flat, B, 5, q, v, s, tau, fext, *d, state=st)
    for k in (3, 4):
        dz = [np.zeros_like(x) if i == k else x for i, x in enumerate(d)]
        dn = [None if i == k else x for i, x in enumerate(d)]
        zero, _ = jvp(rbd, flat, B, 5, q, v, s, tau, fext, *dz, state=st)
        null, _ = jvp(rbd, flat, B, 5, q, v, s, tau, fext, *dn, state=st)
        for name, a, b in zip(("dq+", "dv+", "ds+"), zero, null):
            close(b, a, 1e-12, name + " (NULL tangent %d)" % k)
        assert any(np.abs(a - f).max() > 0 for a, f in zip(zero, full))  # (the direction dropped was live)


def test_fp32_against_fp64(rbd):
    """fp32, walker, B = 64, one step, dt = 5e-4 (test_simulate_contact_vjp_gpu.py::test_fp32_against_fp64 found dt = 1e-3 within 8.2e-4 of a stick / slip
    boundary), on states 1e-3 clear of the branch boundaries at every stage whose fp32 and fp64 reference rollouts take the same branches: per block of A and B,
    the error of the fp32 call against the fp64 call is at most 4 × the error of the fp32 VJP-row Jacobian against its fp64 self, plus 1e-6 (errors relative to
    1 + max|fp64 value|)."""
    flat, bare = walker_pair(rbd)
    B, dt = 64, 5e-4
    nq, nv, ns, nx = dims(flat)
    rng, q, v, s, tau, fext = walker_inputs(rbd, flat, B, seed=6, vscales=(1.0,))
    cot = cotangents(flat, B, rng)
    _, _, infos = Reference(rbd, flat, bare, B).run(q, v, s, tau, fext, cot, 1, dt=dt)
    ok = all_margins(infos, rel=1e-3)
    print("margins %d / %d" % (int(ok.sum()), B))
    assert bool(ok.all())
    _, _, infos32 = Reference(rbd, flat, bare, B, dtype=torch.float32).run(q, v, s, tau, fext, cot, 1, dt=dt)
    assert torch.equal(branches(infos), branches(infos32))
    ref64, ref32 = (vjp_rows(rbd, flat, B, q, v, s, tau, fext, dt=dt, dtype=t)[:2] for t in (torch.float64, torch.float32))
    got64, got32 = (jacobians(rbd, flat, B, q, v, s, tau, fext, dt=dt, dtype=t)[:2] for t in (torch.float64, torch.float32))
    e = lambda x, r: np.abs(x - r).max() / (1 + np.abs(r).max())
    rows = (("q", 0, nq), ("v", nq, nq + nv), ("s", nq + nv, nx))
    bad = []
    for m, mname, cols in ((0, "A", rows), (1, "B", (("tau", 0, nv),))):
        for rn, r0, r1 in rows:
            for cn, c0, c1 in cols:
                blk = lambda x: x[m][:, r0:r1, c0:c1]
                ours, theirs = e(blk(got32), blk(got64)), e(blk(ref32), blk(ref64))
                print("%s d%s+/d%-3s fp32 call %.3e  fp32 VJP rows %.3e  ratio %.2f" % (mname, rn, cn, ours, theirs, ours / max(theirs, 1e-300)))
                assert np.isfinite(blk(got32)).all()
                if not ours <= 4 * theirs + 1e-6:
                    bad.append((mname, rn, cn, ours, theirs))
    assert not bad, bad


def test_errors_and_no_ops(rbd, models, walker130):
    L, p = rbd._capi.lib(), (lambda t: None if t is None else ctypes.c_void_p(t.data_ptr()))
    w = walker130
    flat, B = w["flat"], w["B"]
    nq, nv, ns, nx = dims(flat)
    st = rbd.MechanismState(flat, B)
    q, v, s, tau, fext = (dev(x) for x in w["inputs"])
    dq, dv, ds = (dev(x[:, :1].reshape(B, -1)) for x in w["d"][:3])
    A, Bt = nan(B, nx * nx), nan(B, nx * nv)
    opts = st._opts()

    def run(state=st, batch=B, ntan=1, q=q, v=v, s=s, dt=DT, n=1, dq=dq, dv=dv, ds=ds, o=opts):
        return L.rbd_simulate_contact_jvp(state.ws.handle, batch, ntan, p(q), p(v), p(s), p(tau), p(fext), ctypes.c_double(dt), n, p(dq), p(dv), p(ds), None, None,
                                          ctypes.byref(o))

    def jac(state=st, batch=B, q=q, v=v, s=s, dt=DT, A=A, Bt=Bt, o=opts):
        return L.rbd_simulate_contact_step_derivatives(state.ws.handle, batch, p(q), p(v), p(s), p(tau), p(fext), ctypes.c_double(dt), p(A), p(Bt), ctypes.byref(o))
    keep = [x.clone() for x in (q, v, s, dq, dv, ds)]
    same = lambda: all(torch.equal(a, b) for a, b in zip(keep, (q, v, s, dq, dv, ds))) and bool(torch.isnan(A).all()) and bool(torch.isnan(Bt).all())
    # ntan <= 0, dt <= 0, nsteps < 0, a NULL q, v, s, dq, dv or ds: RBD_ERR_INVALID_ARGUMENT
    for kw in (dict(ntan=0), dict(ntan=-3), dict(dt=0.0), dict(dt=-DT), dict(dt=float("nan")), dict(n=-1), dict(q=None), dict(v=None), dict(s=None), dict(dq=None),
               dict(dv=None), dict(ds=None)):
        assert run(**kw) == 1, kw
    for kw in (dict(dt=0.0), dict(dt=-DT), dict(q=None), dict(v=None), dict(s=None)):
        assert jac(**kw) == 1, kw
    # host memory: RBD_ERR_UNSUPPORTED; a batch beyond the workspace's: RBD_ERR_DIMENSION_MISMATCH
    hopts = rbd._capi.Opts(opts.layout, rbd._capi.MEM_HOST, opts.algorithm, opts.stabilization)
    assert run(o=hopts) == 3 and jac(o=hopts) == 3
    assert run(batch=B + 1) == 2 and jac(batch=B + 1) == 2
    # no contact points (a model that never had any, the bare walker), contact points without an environment: RBD_ERR_INVALID_ARGUMENT; loop joints: HAS_LOOPS
    z4 = torch.zeros(4, 64 * 64, dtype=torch.float64, device="cuda")
    noenv = with_contact(w["bare"], [dict(c) for c in flat.contact_points], [])
    for model, code in ((models["double_pendulum"], 1), (w["bare"], 1), (noenv, 1), (models["four_bar"], 7)):
        m = rbd.MechanismState(model, 4)
        assert run(state=m, batch=4, q=m.q, v=m.v, s=z4, dq=z4, dv=z4, ds=z4, o=m._opts()) == code
        assert jac(state=m, batch=4, q=m.q, v=m.v, s=z4, A=z4, Bt=z4, o=m._opts()) == code
    assert rbd.sync(st) == 0 and same()
    # B == 0 or nsteps == 0: a successful no-op that writes nothing
    assert run(batch=0, n=3) == 0 and jac(batch=0) == 0 and run(n=0) == 0
    assert rbd.sync(st) == 0 and same()
    with pytest.raises(ValueError):
        rbd.simulate_contact_jvp_(dq, dv, ds, st, 0, DT)
    with pytest.raises(ValueError):
        rbd.simulate_contact_jvp_(dq, dv, ds, st, 1, DT, -1)
    with pytest.raises(ValueError):
        rbd.simulate_contact_jvp_(dq, dv, None, st, 1, DT)
    with pytest.raises(ValueError):
        rbd.simulate_contact_step_derivatives_(st, 0.0)
    with pytest.raises(rbd.DimensionMismatch):
        rbd.simulate_contact_jvp_(dq, dv, torch.zeros((B, ns + 1), dtype=torch.float64, device="cuda"), st, 1, DT)
    with pytest.raises(rbd.DimensionMismatch):
        rbd.simulate_contact_step_derivatives_(st, DT, dx_dx=torch.zeros((B, (nq + nv) ** 2), dtype=torch.float64, device="cuda"))
    # the entry points without contact in their name keep refusing the model
    assert L.rbd_simulate_jvp(st.ws.handle, B, 1, p(q), p(v), None, None, ctypes.c_double(DT), 1, p(dq), p(dv), None, None, ctypes.byref(opts)) == 3
    assert L.rbd_simulate_step_derivatives(st.ws.handle, B, p(q), p(v), None, None, ctypes.c_double(DT), None, None, ctypes.byref(opts)) == 3
    assert rbd.sync(st) == 0 and same()
    # and proper calls work afterwards
    assert run(n=2) == 0 and jac() == 0 and rbd.sync(st) == 0
    assert not torch.equal(keep[0], q) and all(bool(torch.isfinite(x).all()) for x in (q, v, s, dq, dv, ds, A, Bt))


def test_second_call_allocates_nothing(rbd, walker130):
    """The first calls allocate; the same calls again, and calls with fewer directions or outputs, do not.  A JVP with more directions than any pass before
    (80 > the Jacobians' 55) does, and the call after it does not."""
    w = walker130
    flat, B = w["flat"], w["B"]
    nq, nv, ns, nx = dims(flat)
    st = rbd.MechanismState(flat, B)
    q, v, s, tau, fext = (dev(x) for x in w["inputs"])  # (every tensor of the test made before the measurement)
    d = [dev(x.reshape(B, -1)) for x in w["d"]]
    A, Bt = torch.empty(B, nx * nx, dtype=torch.float64, device="cuda"), torch.empty(B, nx * nv, dtype=torch.float64, device="cuda")
    d3 = [dev(x[:, :3].reshape(B, -1)) for x in w["d"][:3]]
    wide = [torch.zeros(B, 80 * n, dtype=torch.float64, device="cuda") for n in (nq, nv, ns)]

    def calls():
        rbd.simulate_contact_jvp_(d[0], d[1], d[2], st, 5, DT, 2, torques=tau, dtorques=d[3], externalwrenches=fext, dexternalwrenches=d[4], q=q, v=v, s=s)
        rbd.simulate_contact_step_derivatives_(st, DT, tau, A, Bt, fext, q=q, v=v, s=s)
    calls()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    calls()
    rbd.simulate_contact_jvp_(*d3, st, 3, DT, 1, q=q, v=v, s=s)
    rbd.simulate_contact_step_derivatives_(st, DT, tau, dx_dtau=Bt, q=q, v=v, s=s)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    rbd.simulate_contact_jvp_(*wide, st, 80, DT, 1, torques=tau, q=q, v=v, s=s)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free1 < free0
    rbd.simulate_contact_jvp_(*wide, st, 80, DT, 1, torques=tau, q=q, v=v, s=s)
    calls()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free1
    assert rbd.sync(st) == 0


def test_last_kernel_names_the_stage_kernel(rbd, walker130):
    w = walker130
    flat, B = w["flat"], 4
    st = rbd.MechanismState(flat, B)
    q, v, s = (dev(x[:B]) for x in w["inputs"][:3])
    d = [dev(x[:B, :1].reshape(B, -1)) for x in w["d"][:3]]
    rbd.simulate_contact_jvp_(*d, st, 1, DT, 1, q=q, v=v, s=s)
    assert rbd.sync(st) == 0 and STAGE_KERNEL in rbd.last_kernel(st)
