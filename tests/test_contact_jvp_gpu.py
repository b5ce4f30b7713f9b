"""Forward mode through soft contact on the GPU (rbd_contact_dynamics_jvp, rbd_dynamics_contact_jvp, rbd_dynamics_contact_derivatives).  The reference is exact
and independent of the code under test: the merged reverse mode (rbd_dynamics_contact_vjp, rbd_contact_dynamics_vjp — itself held at 1e-10 to torch autograd of
the composition of merged parts by test_contact_vjp_gpu.py).  A Jacobian assembled from its rows (unit cotangents) must equal the Jacobian assembled from
forward-mode columns, and ⟨cotangent, J·d⟩ = ⟨Jᵀ·cotangent, d⟩ state by state.  No difference quotients."""
import ctypes
import os

import numpy as np
import pytest
import torch

import contact_model_ref as cm
from test_contact_vjp_gpu import cond_bound, dev, host, interpreting_kernels, walker_inputs, walker_pair, with_contact  # noqa: F401 (the RBD_JIT=0 fixture)

pytestmark = pytest.mark.gpu
JAC = ("vd_q", "vd_v", "vd_s", "vd_tau", "sd_q", "sd_v", "sd_s")


def close(got, ref, tol, what):
    err = np.abs(got - ref).max()
    print("%-12s max|err| %.3e  max|ref| %.3e  bound %.3e" % (what, err, np.abs(ref).max(), tol * (1 + np.abs(ref).max())))
    assert np.isfinite(got).all(), what
    assert err <= tol * (1 + np.abs(ref).max()), (what, err, np.abs(ref).max())


def nan(B, n, layout="aos", dtype=torch.float64):
    return torch.full((B, n) if layout == "aos" else (n, B), float("nan"), dtype=dtype, device="cuda")


def jac_shapes(flat):
    nq, nv, ns = flat.nq, flat.nv, flat.ns
    return dict(vd_q=(nv, nq), vd_v=(nv, nv), vd_s=(nv, ns), vd_tau=(nv, nv), sd_q=(ns, nq), sd_v=(ns, nv), sd_s=(ns, ns))


def vjp_rows(rbd, flat, B, q, v, s, tau, fext, dtype=torch.float64):
    """The seven Jacobians (B, rows, cols) by rows: nv + ns calls of rbd_dynamics_contact_vjp with unit cotangents."""
    st = rbd.MechanismState(flat, B, dtype=dtype)
    D = lambda x: dev(x, dtype=dtype)
    qd, vd_, sd_, td, fd = D(q), D(v), D(s), D(tau), D(fext)
    J = {k: np.full((B,) + shp, np.nan) for k, shp in jac_shapes(flat).items()}
    out = [nan(B, n, dtype=dtype) for n in (flat.nq, flat.nv, flat.ns, flat.nv)]
    for i in range(flat.nv + flat.ns):
        e = torch.zeros(B, flat.nv if i < flat.nv else flat.ns, dtype=dtype, device="cuda")
        e[:, i if i < flat.nv else i - flat.nv] = 1
        for o in out:
            o.fill_(float("nan"))
        if i < flat.nv:
            rbd.dynamics_contact_vjp_(st, e, None, None, td, fd, *out, q=qd, v=vd_, s=sd_)
            for k, o in zip(("vd_q", "vd_v", "vd_s", "vd_tau"), out):
                J[k][:, i, :] = host(o)
        else:
            rbd.dynamics_contact_vjp_(st, None, e, None, td, fd, *out[:3], q=qd, v=vd_, s=sd_)
            for k, o in zip(("sd_q", "sd_v", "sd_s"), out[:3]):
                J[k][:, i - flat.nv, :] = host(o)
    assert rbd.sync(st) == 0
    return J


def derivatives(rbd, flat, B, q, v, s, tau, fext, layout="aos", dtype=torch.float64, state=None):
    """One rbd_dynamics_contact_derivatives call on NaN-prefilled outputs: the seven Jacobians (B, rows, cols), v̇ and ṡ (fp64 numpy)."""
    st = state or rbd.MechanismState(flat, B, dtype=dtype, layout=layout)
    D = lambda x: dev(x, layout, dtype)
    shp = jac_shapes(flat)
    outs = {k: nan(B, r * c, layout, dtype) for k, (r, c) in shp.items()}
    vdo, sdo, sd_ = nan(B, flat.nv, layout, dtype), nan(B, flat.ns, layout, dtype), D(s)
    rbd.dynamics_contact_derivatives_(st, D(tau), D(fext), outs["vd_q"], outs["vd_v"], outs["vd_s"], outs["vd_tau"], outs["sd_q"], outs["sd_v"], outs["sd_s"],
                                      vdout=vdo, sdout=sdo, q=D(q), v=D(v), s=sd_)
    assert rbd.sync(st) == 0
    assert torch.equal(sd_, D(s))  # s is const: not reset
    assert "tangent_contact" in rbd.last_kernel(st)
    J = {k: host(outs[k], layout).reshape(B, shp[k][1], shp[k][0]).transpose(0, 2, 1) for k in JAC}  # (column-major per state)
    return J, host(vdo, layout), host(sdo, layout)


def jvp(rbd, flat, B, ntan, q, v, s, tau, fext, dq, dv, ds, dtau, dfext, layout="aos", dtype=torch.float64, state=None, want=(True, True, True)):
    """One rbd_dynamics_contact_jvp call on NaN-prefilled outputs; tangents (B, ntan, n) numpy in and out (None: not passed / not asked for)."""
    st = state or rbd.MechanismState(flat, B, dtype=dtype, layout=layout)
    D = lambda x: dev(x, layout, dtype)
    T = lambda x: None if x is None else D(x[:, :ntan].reshape(B, -1))
    outs = [nan(B, ntan * n, layout, dtype) if w else None for n, w in zip((flat.nv, flat.ns, flat.ns), want)]
    sd_ = D(s)
    rbd.dynamics_contact_jvp_(st, ntan, D(tau), D(fext), T(dq), T(dv), T(ds), T(dtau), T(dfext), *outs, q=D(q), v=D(v), s=sd_)
    assert rbd.sync(st) == 0
    assert torch.equal(sd_, D(s)) and "tangent_contact" in rbd.last_kernel(st)
    return [None if o is None else host(o, layout).reshape(B, ntan, -1) for o in outs]


def directions(flat, B, ntan, rng):
    return [rng.standard_normal((B, ntan, n)) for n in (flat.nq, flat.nv, flat.ns, flat.nv, 6 * flat.n_bodies)]


def adjoint_identity(tans_out, cots, bars, tans_in, tol, what):
    """⟨a, dv̇⟩ + ⟨b, dṡ⟩ + ⟨c, ds_out⟩ = ⟨q̄, dq⟩ + … per state and direction, to tol·(1 + Σ|terms|)."""
    left = [np.einsum("bn,bdn->bd", c, t) for c, t in zip(cots, tans_out)]
    right = [np.einsum("bn,bdn->bd", b, t) for b, t in zip(bars, tans_in)]
    mag = sum(np.einsum("bn,bdn->bd", np.abs(c), np.abs(t)) for c, t in zip(list(cots) + list(bars), list(tans_out) + list(tans_in)))
    gap = np.abs(sum(left) - sum(right))
    print("%-22s max gap %.3e  max gap / bound %.3e" % (what, gap.max(), (gap / (tol * (1 + mag))).max()))
    assert all(np.isfinite(t).all() for t in tans_out)
    assert (gap <= tol * (1 + mag)).all(), (what, (gap / (tol * (1 + mag))).max())


def one_vjp(rbd, flat, B, q, v, s, tau, fext, a, b, c, dtype=torch.float64):
    st = rbd.MechanismState(flat, B, dtype=dtype)
    D = lambda x: dev(x, dtype=dtype)
    out = [nan(B, n, dtype=dtype) for n in (flat.nq, flat.nv, flat.ns, flat.nv, 6 * flat.n_bodies)]
    rbd.dynamics_contact_vjp_(st, D(a), D(b), D(c), D(tau), D(fext), *out, q=D(q), v=D(v), s=D(s))
    assert rbd.sync(st) == 0
    return [host(o) for o in out]


@pytest.fixture(scope="module")
def walker130(rbd, oracle, interpreting_kernels):
    """The walker, B = 130, the states of test_contact_vjp_gpu.py (seed 5): the pair information, the Jacobians by rows of rbd_dynamics_contact_vjp (34 calls,
    computed once, shared, left unchanged), the oracle's values, five random directions and one VJP for the adjoint identity."""
    flat, bare = walker_pair(rbd)
    B = 130
    rng, q, v, s, tau, fext = walker_inputs(rbd, flat, B)
    info = cm.oracle_pair_info(oracle, flat, q, v, s)
    J = vjp_rows(rbd, flat, B, q, v, s, tau, fext)
    vd_ref, _, sd_ref, _, _ = oracle.dynamics_contact(flat, q, v, s, tau, fext)
    d = directions(flat, B, 5, rng)
    cots = [rng.standard_normal((B, n)) for n in (flat.nv, flat.ns, flat.ns)]
    bars = one_vjp(rbd, flat, B, q, v, s, tau, fext, *cots)
    return dict(flat=flat, bare=bare, B=B, inputs=(q, v, s, tau, fext), info=info, J=J, vd=vd_ref, sd=sd_ref, d=d, cots=cots, bars=bars, rng=rng)


def expected_tangents(w, d, ntan):
    """J·d from the Jacobians by rows, for the (q, v, s, τ) part; ds_out = ds on inside pairs, 0 outside."""
    J, (dq, dv, ds, dtau, _) = w["J"], [x[:, :ntan] for x in d]
    mm = lambda Jk, x: np.einsum("brc,bdc->bdr", Jk, x)
    inside = np.repeat(w["info"]["inside"].numpy().reshape(w["B"], -1), 3, axis=1)
    return (mm(J["vd_q"], dq) + mm(J["vd_v"], dv) + mm(J["vd_s"], ds) + mm(J["vd_tau"], dtau), mm(J["sd_q"], dq) + mm(J["sd_v"], dv) + mm(J["sd_s"], ds),
            ds * inside[:, None, :])


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_walker_jacobians_against_vjp_rows(rbd, walker130, layout):
    """All seven matrices of one rbd_dynamics_contact_derivatives call at 1e-10·(1 + max|ref|) of the rows of rbd_dynamics_contact_vjp (dvdot_dtau against the
    τ̄ rows); v̇ and ṡ at 1e-10 of oracle.dynamics_contact; every branch holds at least 5 % of the pairs, clear of the boundaries."""
    w = walker130
    cov = cm.coverage(w["info"])
    assert min(cov) >= 0.05, dict(zip(cm.BRANCHES, cov))
    assert bool(cm.margins_ok(w["info"]).all())
    J, vd, sd = derivatives(rbd, w["flat"], w["B"], *w["inputs"], layout=layout)
    for k in JAC:
        close(J[k], w["J"][k], 1e-10, k)
    rel = lambda x, y: np.abs(x - y).max() / max(1.0, np.abs(y).max())
    assert rel(vd, w["vd"]) <= 1e-10 and rel(sd, w["sd"]) <= 1e-10


def test_walker_partial_jacobians(rbd, walker130):
    """Calls that ask for some outputs only (no solve without dvdot_*; no tangent pass for values alone) write the same matrices."""
    w = walker130
    flat, B, (q, v, s, tau, fext) = w["flat"], w["B"], w["inputs"]
    st = rbd.MechanismState(flat, B)
    shp = jac_shapes(flat)
    arg = dict(vd_q="dvd_dq", vd_v="dvd_dv", vd_s="dvd_ds", vd_tau="dvd_dtau", sd_q="dsd_dq", sd_v="dsd_dv", sd_s="dsd_ds")
    for ask in (("sd_q", "sd_s"), ("vd_v",), ("vd_s", "sd_v"), ("vd_tau",)):
        outs = {k: nan(B, shp[k][0] * shp[k][1]) for k in ask}
        rbd.dynamics_contact_derivatives_(st, dev(tau), dev(fext), q=dev(q), v=dev(v), s=dev(s), **{arg[k]: o for k, o in outs.items()})
        for k, o in outs.items():
            close(host(o).reshape(B, shp[k][1], shp[k][0]).transpose(0, 2, 1), w["J"][k], 1e-10, "+".join(ask) + ": " + k)
    vdo, sdo = nan(B, flat.nv), nan(B, flat.ns)
    rbd.dynamics_contact_derivatives_(st, dev(tau), dev(fext), vdout=vdo, sdout=sdo, q=dev(q), v=dev(v), s=dev(s))
    rel = lambda x, y: np.abs(x - y).max() / max(1.0, np.abs(y).max())
    assert rel(host(vdo), w["vd"]) <= 1e-10 and rel(host(sdo), w["sd"]) <= 1e-10


@pytest.fixture(scope="module")
def walker_jvp5(rbd, walker130):
    """The JVP of ntan = 5 with all five tangent inputs live, un-slabbed (computed once; the slab test compares bit for bit)."""
    w = walker130
    return jvp(rbd, w["flat"], w["B"], 5, *w["inputs"], *w["d"])


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("ntan", [5, 1])
def test_walker_jvp_equals_jacobians_times_directions(rbd, walker130, ntan, layout):
    """dv̇, dṡ, ds_out of rbd_dynamics_contact_jvp (dfext NULL) against the Jacobians by rows times the directions; ntan = 5 leaves the last fp64 chunk half full."""
    w = walker130
    dq, dv, ds, dtau, _ = w["d"]
    got = jvp(rbd, w["flat"], w["B"], ntan, *w["inputs"], dq, dv, ds, dtau, None, layout=layout)
    for name, g, r in zip(("dvdot", "dsdot", "ds_out"), got, expected_tangents(w, w["d"], ntan)):
        close(g, r, 1e-10, name)


def test_walker_jvp_adjoint_identity(rbd, walker130, walker_jvp5):
    """⟨a, dv̇⟩ + ⟨b, dṡ⟩ + ⟨c, ds_out⟩ = ⟨q̄, dq⟩ + ⟨v̄, dv⟩ + ⟨s̄, ds⟩ + ⟨τ̄, dτ⟩ + ⟨f̄ext, dfext⟩ state by state with all five tangent inputs live, the barred
    quantities from ONE rbd_dynamics_contact_vjp call, at 1e-10·(1 + Σ|terms|); ntan = 5 and ntan = 1."""
    w = walker130
    adjoint_identity(walker_jvp5, w["cots"], w["bars"], w["d"], 1e-10, "ntan 5")
    one = jvp(rbd, w["flat"], w["B"], 1, *w["inputs"], *w["d"])
    adjoint_identity(one, w["cots"], w["bars"], [x[:, :1] for x in w["d"]], 1e-10, "ntan 1")


def test_walker_jvp_null_inputs_and_partial_outputs(rbd, walker130, walker_jvp5):
    """Each tangent input NULL in turn gives what an explicit zero direction gives; a call that asks for dṡ alone (forward-only pass) returns the same dṡ."""
    w = walker130
    flat, B = w["flat"], w["B"]
    st = rbd.MechanismState(flat, B)
    for k in range(5):
        dz = [np.zeros_like(x) if i == k else x for i, x in enumerate(w["d"])]
        dn = [None if i == k else x for i, x in enumerate(w["d"])]
        zero, null = jvp(rbd, flat, B, 5, *w["inputs"], *dz, state=st), jvp(rbd, flat, B, 5, *w["inputs"], *dn, state=st)
        for name, a, b in zip(("dvdot", "dsdot", "ds_out"), zero, null):
            assert np.isfinite(b).all() and np.array_equal(a, b), (k, name, np.abs(a - b).max())
    _, only, _ = jvp(rbd, flat, B, 5, *w["inputs"], *w["d"], state=st, want=(False, True, False))
    assert np.array_equal(only, walker_jvp5[1])
    close(only, expected_tangents(w, w["d"], 5)[1], 1e-10, "dsdot alone")


def test_walker_jvp_in_slabs(rbd, walker130, walker_jvp5):
    """RBD_TUNE tan_scratch_threads=128: the 3 chunks × 130 states = 390 threads of the ntan = 5 call run in 4 slabs of a workspace made under that setting;
    the result equals the un-slabbed one bit for bit."""
    w = walker130
    old = os.environ.get("RBD_TUNE")
    os.environ["RBD_TUNE"] = "tan_scratch_threads=128"
    try:
        st = rbd.MechanismState(w["flat"], w["B"])
        got = jvp(rbd, w["flat"], w["B"], 5, *w["inputs"], *w["d"], state=st)
    finally:
        if old is None:
            del os.environ["RBD_TUNE"]
        else:
            os.environ["RBD_TUNE"] = old
    assert -(-5 // 2) * w["B"] >= 3 * 128
    for name, g, r in zip(("dvdot", "dsdot", "ds_out"), got, walker_jvp5):
        assert np.isfinite(g).all() and np.array_equal(g, r), (name, np.abs(g - r).max())


def contact_jvp(rbd, st, flat, B, ntan, q, v, s, dq, dv, ds):
    outs = [nan(B, ntan * n) for n in (6 * flat.n_bodies, flat.ns, flat.ns)]
    T = lambda x: dev(x[:, :ntan].reshape(B, -1))
    rbd.contact_dynamics_jvp_(st, ntan, T(dq), T(dv), T(ds), *outs, q=dev(q), v=dev(v), s=dev(s))
    assert rbd.sync(st) == 0 and "tangent_contact" in rbd.last_kernel(st)
    return [host(o).reshape(B, ntan, -1) for o in outs]


def test_contact_dynamics_jvp_alone(rbd, walker130):
    """rbd_contact_dynamics_jvp: the adjoint identity against rbd_contact_dynamics_vjp with random cw_bar, sdot_bar, s_out_bar; a state with every pair outside
    gives all-zero outputs."""
    w = walker130
    flat, B, (q, v, s, tau, fext), rng = w["flat"], w["B"], w["inputs"], w["rng"]
    dq, dv, ds = w["d"][:3]
    cots = [rng.standard_normal((B, n)) for n in (6 * flat.n_bodies, flat.ns, flat.ns)]
    st = rbd.MechanismState(flat, B)
    bars = [nan(B, n) for n in (flat.nq, flat.nv, flat.ns)]
    rbd.contact_dynamics_vjp_(st, *[dev(c) for c in cots], *bars, q=dev(q), v=dev(v), s=dev(s))
    got = contact_jvp(rbd, st, flat, B, 5, q, v, s, dq, dv, ds)
    adjoint_identity(got, cots, [host(b) for b in bars], [dq, dv, ds], 1e-10, "contact_dynamics_jvp")
    assert all(np.abs(g).max() > 0 for g in got)
    # far on the outer side of both half-spaces (the state of test_contact_dynamics_vjp_alone)
    nrm = np.array([h["outward_normal"] / np.linalg.norm(h["outward_normal"]) for h in flat.halfspaces])
    qo = q.copy()
    qo[:, 4:7] = flat.pred_rot[0].T @ (20.0 * nrm.sum(axis=0))
    assert not bool(cm.oracle_pair_info(__import__("oracle"), flat, qo, v, s)["inside"].any())
    assert all((g == 0).all() for g in contact_jvp(rbd, st, flat, B, 5, qo, v, s, dq, dv, ds))


def other_mechanism(rbd, oracle, flat, bare, B, q, v, s, rng):
    """The adjoint identity with ntan = 3 at cond_bound, and v̇, ṡ against the oracle as the VJP tests do."""
    tau, fext = rng.random((B, flat.nv)), rng.random((B, 6 * flat.n_bodies))
    cots = [rng.standard_normal((B, n)) for n in (flat.nv, flat.ns, flat.ns)]
    info = cm.oracle_pair_info(oracle, flat, q, v, s)
    assert bool(info["inside"].any()) and not bool(info["inside"].all()) and bool(cm.margins_ok(info).all())
    d = directions(flat, B, 3, rng)
    st = rbd.MechanismState(flat, B)
    vdo, sdo = nan(B, flat.nv), nan(B, flat.ns)
    outs = [nan(B, 3 * n) for n in (flat.nv, flat.ns, flat.ns)]
    rbd.dynamics_contact_jvp_(st, 3, dev(tau), dev(fext), *[dev(x.reshape(B, -1)) for x in d], *outs, vdout=vdo, sdout=sdo, q=dev(q), v=dev(v), s=dev(s))
    assert rbd.sync(st) == 0 and "tangent_contact" in rbd.last_kernel(st)
    tol = cond_bound(oracle, bare, q)
    bars = one_vjp(rbd, flat, B, q, v, s, tau, fext, *cots)
    adjoint_identity([host(o).reshape(B, 3, -1) for o in outs], cots, bars, d, tol, "ntan 3")
    vd_ref, _, sd_ref, _, _ = oracle.dynamics_contact(flat, q, v, s, tau, fext)
    close(host(vdo), vd_ref, tol, "vdot")
    close(host(sdo), sd_ref, 1e-10, "sdot")


def test_atlas_floating(rbd, oracle, models):
    """Atlas on a floating base, B = 67, the construction of test_contact_vjp_gpu.py::test_atlas_floating (seed 23): some feet touch, not all."""
    bare = models["atlas_floating"]
    feet = [bare.body_names.index(n) for n in ("l_foot", "r_foot")]
    hc = rbd.hunt_crossley_hertz()
    par = dict(hc_k=hc.k, hc_lambda=hc.lam, hc_n=hc.n, mu=0.8, k=20e3, b=100.0)
    pts = [dict(par, body=f, location=np.array([x, 0.0, -0.08])) for f in feet for x in (0.15, -0.08)]
    flat = with_contact(bare, pts, [dict(point=np.zeros(3), outward_normal=np.array([0.0, 0.0, 1.0]))])
    B = 67
    rng = np.random.default_rng(23)
    q, v = rbd.rand_configuration(bare, B, rng), rbd.rand_velocity(bare, B, rng)
    up = bare.pred_rot[0].T @ np.array([0.0, 0.0, 1.0])
    q[:, 4:7] = 0
    ref = rbd.MechanismState(bare, B)
    rbd.set_points_(ref, [c["body"] for c in pts], [c["location"] for c in pts])
    pos = torch.empty(B, 12, dtype=torch.float64, device="cuda")
    rbd.point_kinematics_(ref, pos, q=dev(q), v=dev(v))
    low = host(pos).reshape(B, 4, 3)[:, :, 2].min(axis=1)
    q[:, 4:7] = (rng.uniform(-0.03, 0.01, B) - low)[:, None] * up
    s = 1e-3 * rng.standard_normal((B, flat.ns))
    other_mechanism(rbd, oracle, flat, bare, B, q, v, s, rng)


def test_tree_of_more_than_64_bodies(rbd, oracle):
    """The 70-body tree of test_contact_vjp_gpu.py::test_tree_of_more_than_64_bodies, B = 8: the any-size route of the value path."""
    def build(bare):
        rng = np.random.default_rng(15)
        mech = rbd.rand_tree_mechanism(rng, ["QuaternionFloating"] + ["Revolute"] * 69)
        for k in (3, 35, 69):
            model = rbd.SoftContactModel(rbd.hunt_crossley_hertz(k=2e3 * (1 + rng.random()), alpha=0.3 * rng.random()),
                                         rbd.ViscoelasticCoulombModel(0.3 + rng.random(), 1e3 * (1 + rng.random()), 1e2 * (1 + rng.random())))
            rbd.add_contact_point_(mech.bodies[1:][k], rbd.ContactPoint(0.3 * rng.standard_normal(3), model))
        rbd.add_environment_primitive_(mech, rbd.HalfSpace3D([0, 0, 0.2], [0.1, -0.2, 1.0]))
        return rbd.flatten(cm.strip_contact(mech) if bare else mech), rng
    (flat, rng), (bare, _) = build(False), build(True)
    assert flat.n_bodies == 70 and flat.ns == 9
    B = 8
    q, v = rbd.rand_configuration(flat, B, rng), rbd.rand_velocity(flat, B, rng)
    s = 1e-3 * rng.standard_normal((B, flat.ns))
    other_mechanism(rbd, oracle, flat, bare, B, q, v, s, rng)


def gpu_pair_info(rbd, flat, bare, B, q, v, s, dtype):
    """The pair information at the contact points' positions and velocities the library computes in `dtype` (merged point kinematics on the bare model)."""
    ref = rbd.MechanismState(bare, B, dtype=dtype)
    rbd.set_points_(ref, [c["body"] for c in flat.contact_points], [c["location"] for c in flat.contact_points])
    n = 3 * len(flat.contact_points)
    pos, vel = torch.empty(B, n, dtype=dtype, device="cuda"), torch.empty(B, n, dtype=dtype, device="cuda")
    rbd.point_kinematics_(ref, pos, vel, q=dev(q, dtype=dtype), v=dev(v, dtype=dtype))
    info = cm.contact_model(flat, pos, vel, dev(s, dtype=dtype), cm.tables(flat, dtype, "cuda"))[3]
    return {k: x.cpu() for k, x in info.items()}


def test_fp32_against_fp64(rbd):
    """fp32, walker, B = 64, on states a factor 1e-3 clear of the branch boundaries: per Jacobian, the error of the fp32 call against the fp64 call is at most
    4 × the error of the fp32 VJP-row Jacobian against its fp64 self, plus 1e-6 (errors relative to 1 + max|fp64 value|): the rule of
    test_contact_vjp_gpu.py::test_fp32_against_fp64."""
    flat, bare = walker_pair(rbd)
    B = 64
    rng, q, v, s, tau, fext = walker_inputs(rbd, flat, B, seed=6, vscales=(1.0,))
    info = gpu_pair_info(rbd, flat, bare, B, q, v, s, torch.float64)
    assert bool(cm.margins_ok(info, rel=1e-3).all())
    assert torch.equal(cm.branch_of(info), cm.branch_of(gpu_pair_info(rbd, flat, bare, B, q, v, s, torch.float32)))
    ref64, ref32 = (vjp_rows(rbd, flat, B, q, v, s, tau, fext, dtype=dt) for dt in (torch.float64, torch.float32))
    got64, got32 = (derivatives(rbd, flat, B, q, v, s, tau, fext, dtype=dt)[0] for dt in (torch.float64, torch.float32))
    e = lambda x, r: np.abs(x - r).max() / (1 + np.abs(r).max())
    bad = []
    for k in JAC:
        ours, theirs = e(got32[k], got64[k]), e(ref32[k], ref64[k])
        print("%-7s fp32 call %.3e  fp32 VJP rows %.3e  ratio %.2f" % (k, ours, theirs, ours / max(theirs, 1e-300)))
        if not ours <= 4 * theirs + 1e-6:
            bad.append((k, ours, theirs))
    assert not bad, bad


def test_errors_and_no_ops(rbd, models, walker130):
    from rigidbodydynamics_jl_amd import _capi
    L, p = _capi.lib(), (lambda t: ctypes.c_void_p(t.data_ptr()))
    w = walker130
    flat, B = w["flat"], w["B"]
    st = rbd.MechanismState(flat, B)
    z = lambda n, b=B: torch.zeros(b, n, dtype=torch.float64, device="cuda")
    s, dv, out = z(flat.ns), z(flat.nv), z(flat.ns)
    opts = st._opts()

    def three(state, batch, ntan, q, v, s, dv, out, o):
        h = state.ws.handle
        return (L.rbd_contact_dynamics_jvp(h, batch, ntan, q, v, s, None, dv, None, None, out, None, ctypes.byref(o)),
                L.rbd_dynamics_contact_jvp(h, batch, ntan, q, v, s, None, None, None, dv, None, None, None, None, None, None, out, None, ctypes.byref(o)),
                L.rbd_dynamics_contact_derivatives(h, batch, q, v, s, None, None, None, out, None, None, None, None, None, None, None, ctypes.byref(o)))
    # a model without contact points: RBD_ERR_INVALID_ARGUMENT
    dp = rbd.MechanismState(models["double_pendulum"], 4)
    z4 = torch.zeros(4, 8, dtype=torch.float64, device="cuda")
    assert three(dp, 4, 1, p(dp.q), p(dp.v), p(z4), p(z4), p(z4), dp._opts()) == (1, 1, 1)
    # contact points without an environment
    noenv = with_contact(w["bare"], [dict(c) for c in flat.contact_points], [])
    ne = rbd.MechanismState(noenv, 4)
    z4w = torch.zeros(4, 64, dtype=torch.float64, device="cuda")
    assert three(ne, 4, 1, p(ne.q), p(ne.v), p(z4w), p(z4w), p(z4w), ne._opts()) == (1, 1, 1)
    # loop joints: RBD_ERR_HAS_LOOPS
    fb = rbd.MechanismState(models["four_bar"], 4)
    assert three(fb, 4, 1, p(fb.q), p(fb.v), p(z4), p(z4), p(z4), fb._opts()) == (7, 7, 7)
    # host memory: RBD_ERR_UNSUPPORTED
    hopts = _capi.Opts(opts.layout, _capi.MEM_HOST, opts.algorithm, opts.stabilization)
    assert three(st, B, 1, p(st.q), p(st.v), p(s), p(dv), p(out), hopts) == (3, 3, 3)
    # ntan <= 0, or a NULL q / v / s: RBD_ERR_INVALID_ARGUMENT
    assert three(st, B, 0, p(st.q), p(st.v), p(s), p(dv), p(out), opts)[:2] == (1, 1)
    assert three(st, B, -2, p(st.q), p(st.v), p(s), p(dv), p(out), opts)[:2] == (1, 1)
    assert three(st, B, 1, None, p(st.v), p(s), p(dv), p(out), opts) == (1, 1, 1)
    assert three(st, B, 1, p(st.q), None, p(s), p(dv), p(out), opts) == (1, 1, 1)
    assert three(st, B, 1, p(st.q), p(st.v), None, p(dv), p(out), opts) == (1, 1, 1)
    # B == 0: a successful no-op; a batch beyond the workspace's: RBD_ERR_DIMENSION_MISMATCH
    out.fill_(float("nan"))
    assert three(st, 0, 1, p(st.q), p(st.v), p(s), p(dv), p(out), opts) == (0, 0, 0)
    assert rbd.sync(st) == 0 and bool(torch.isnan(out).all())
    assert three(st, B + 1, 1, p(st.q), p(st.v), p(s), p(dv), p(out), opts) == (2, 2, 2)
    # the entry points without contact keep refusing the model
    assert L.rbd_dynamics_jvp(st.ws.handle, B, 1, p(st.q), p(st.v), None, None, None, p(dv), None, None, None, p(dv), ctypes.byref(opts)) == 3
    assert L.rbd_dynamics_derivatives(st.ws.handle, B, p(st.q), p(st.v), None, None, p(dv), None, None, None, ctypes.byref(opts)) == 3
    # and a proper call still works afterwards
    assert three(st, B, 1, p(st.q), p(st.v), p(s), p(dv), p(out), opts) == (0, 0, 0)
    assert rbd.sync(st) == 0 and bool(torch.isfinite(out).all())


def test_second_call_allocates_nothing(rbd, walker130):
    w = walker130
    flat, B, (q, v, s, tau, fext) = w["flat"], w["B"], w["inputs"]
    st = rbd.MechanismState(flat, B)
    qd, vd_, sd_, td, fd = (dev(x) for x in (q, v, s, tau, fext))  # (every tensor of the test made before the measurement)
    d = [dev(x.reshape(B, -1)) for x in w["d"]]
    shp = jac_shapes(flat)
    jac = [torch.empty(B, r * c, dtype=torch.float64, device="cuda") for r, c in (shp[k] for k in JAC)]
    tan = [torch.empty(B, 5 * n, dtype=torch.float64, device="cuda") for n in (flat.nv, flat.ns, flat.ns, 6 * flat.n_bodies)]

    def calls():
        rbd.dynamics_contact_jvp_(st, 5, td, fd, *d, *tan[:3], q=qd, v=vd_, s=sd_)
        rbd.dynamics_contact_derivatives_(st, td, fd, *jac, q=qd, v=vd_, s=sd_)
        rbd.contact_dynamics_jvp_(st, 5, d[0], d[1], d[2], tan[3], tan[1], tan[2], q=qd, v=vd_, s=sd_)
    calls()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    calls()
    rbd.dynamics_contact_jvp_(st, 5, td, fd, d[0], None, None, None, None, None, tan[1], None, q=qd, v=vd_, s=sd_)
    rbd.dynamics_contact_derivatives_(st, td, fd, dsd_ds=jac[6], q=qd, v=vd_, s=sd_)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    assert rbd.sync(st) == 0
