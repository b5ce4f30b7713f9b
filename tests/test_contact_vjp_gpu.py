"""Reverse mode through soft contact on the GPU (rbd_contact_dynamics_vjp, rbd_dynamics_contact_vjp, autograd.dynamics_contact).  The reference is exact, a
composition of merged parts evaluated on the GPU: autograd.point_kinematics on the BARE model (the same mechanism without contact points and environment) with
the contact points set as points, the torch pair model (tests/contact_model_ref.py, pinned to the oracle by test_contact_vjp_cpu.py), autograd.dynamics of the
bare model at fext + contactwrenches, and backward() of Σ v̇·a + Σ ṡ·b + Σ s_out·c.  No difference quotients (gradcheck apart, which is torch's own)."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import contact_model_ref as cm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("q_bar", "v_bar", "s_bar", "tau_bar", "fext_bar")


@pytest.fixture(scope="module", autouse=True)
def interpreting_kernels():
    """Nothing under test here is compiled per mechanism at run time: the workspaces of this module run the kernels built with the library (RBD_JIT is read
    when a workspace first asks), so no test waits for hiprtc on a mechanism met for the first time."""
    old = os.environ.get("RBD_JIT")
    os.environ["RBD_JIT"] = "0"
    yield
    if old is None:
        del os.environ["RBD_JIT"]
    else:
        os.environ["RBD_JIT"] = old


def dev(a, layout="aos", dtype=torch.float64):
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)
    return (t if layout == "aos" else t.t().contiguous()).cuda()


def host(t, layout="aos"):
    t = t.detach().double().cpu()
    return (t if layout == "aos" else t.t()).numpy().copy()


class Case:
    """A mechanism with contact (flat), the same without (bare), the bare model's state with the contact points set as points, and the contact tables."""

    def __init__(self, rbd, flat, bare, B, dtype=torch.float64):
        self.rbd, self.flat, self.bare, self.B, self.dtype = rbd, flat, bare, B, dtype
        self.ref = rbd.MechanismState(bare, B, dtype=dtype)
        rbd.set_points_(self.ref, [c["body"] for c in flat.contact_points], [c["location"] for c in flat.contact_points])
        self.tab = cm.tables(flat, dtype, "cuda")

    def composition(self, q, v, s, tau, fext, a, b, c, cw_bar=None):
        """backward() through the merged parts; (B, n) numpy in, the five gradients (fp64 numpy), the pair info and the values (v̇, ṡ, s_out) out.  With
        `cw_bar` the loss is Σ cw·cw_bar + Σ ṡ·b + Σ s_out·c (contact_dynamics! alone)."""
        rbd, D = self.rbd, (lambda x: dev(x, dtype=self.dtype))
        qq, vv, ss, tt, ff = (D(x).requires_grad_(True) for x in (q, v, s, tau, fext))
        pos, vel = rbd.autograd.point_kinematics(self.ref, qq, vv)
        cw, sd, s_out, info = cm.contact_model(self.flat, pos, vel, ss, self.tab)
        if cw_bar is None:
            vd = rbd.autograd.dynamics(self.ref, qq, vv, tt, ff + cw)
            loss = (vd * D(a)).sum() + (sd * D(b)).sum() + (s_out * D(c)).sum()
        else:
            vd = None
            loss = (cw * D(cw_bar)).sum() + (sd * D(b)).sum() + (s_out * D(c)).sum()
        loss.backward()
        grads = [host(x.grad) if x.grad is not None else np.zeros(x.shape) for x in (qq, vv, ss, tt, ff)]
        return grads, {k: x.cpu() for k, x in info.items()}, (vd, sd, s_out)


def fused(rbd, flat, B, q, v, s, tau, fext, a, b, c, layout="aos", dtype=torch.float64, state=None):
    """One rbd_dynamics_contact_vjp call on NaN-prefilled outputs: the five gradients and (v̇, ṡ), fp64 numpy (B, n)."""
    st = state or rbd.MechanismState(flat, B, dtype=dtype, layout=layout)
    D = lambda x: None if x is None else dev(x, layout, dtype)
    nan = lambda n: torch.full((B, n) if layout == "aos" else (n, B), float("nan"), dtype=dtype, device="cuda")
    out = [nan(n) for n in (flat.nq, flat.nv, flat.ns, flat.nv, 6 * flat.n_bodies)]
    vdo, sdo = nan(flat.nv), nan(flat.ns)
    sd_ = D(s)
    rbd.dynamics_contact_vjp_(st, D(a), D(b), D(c), D(tau), D(fext), *out, vdout=vdo, sdout=sdo, q=D(q), v=D(v), s=sd_)
    assert rbd.sync(st) == 0
    assert torch.equal(sd_, D(s))  # s is const: not reset
    assert "contact_adjoint_kernel" in rbd.last_kernel(st)
    return [host(x, layout) for x in out], host(vdo, layout), host(sdo, layout)


def close(got, ref, tol, what):
    err = np.abs(got - ref).max()
    print("%-10s max|err| %.3e  max|ref| %.3e  bound %.3e" % (what, err, np.abs(ref).max(), tol * (1 + np.abs(ref).max())))
    assert np.isfinite(got).all(), what
    assert err <= tol * (1 + np.abs(ref).max()), (what, err, np.abs(ref).max())


def cotangents(flat, B, rng):
    return rng.standard_normal((B, flat.nv)), rng.standard_normal((B, flat.ns)), rng.standard_normal((B, flat.ns))


def walker_pair(rbd, seed=5):
    return rbd.flatten(cm.walker(rbd, np.random.default_rng(seed))), rbd.flatten(cm.walker(rbd, np.random.default_rng(seed), bare=True))


def walker_inputs(rbd, flat, B, seed=5, **kw):
    rng = np.random.default_rng(seed)
    cm.walker(rbd, rng)  # (the draws of the mechanism itself, as test_contact.py makes them)
    q, v, s = cm.walker_states(rbd, flat, B, rng, **kw)
    return rng, q, v, s, rng.random((B, flat.nv)), rng.random((B, 6 * flat.n_bodies))


@pytest.fixture(scope="module")
def walker130(rbd, oracle, interpreting_kernels):
    """The walker, B = 130: inputs, cotangents, the composition's gradients (computed once, shared, left unchanged) and the oracle's values."""
    flat, bare = walker_pair(rbd)
    B = 130
    rng, q, v, s, tau, fext = walker_inputs(rbd, flat, B)
    a, b, c = cotangents(flat, B, rng)
    case = Case(rbd, flat, bare, B)
    ref, info, _ = case.composition(q, v, s, tau, fext, a, b, c)
    vd_ref, s_ref, sd_ref, _, _ = oracle.dynamics_contact(flat, q, v, s, tau, fext)
    return dict(flat=flat, case=case, B=B, inputs=(q, v, s, tau, fext), cot=(a, b, c), ref=ref, info=info, vd=vd_ref, sd=sd_ref, rng=rng)


def test_walker_states_cover_every_branch_with_margins(walker130):
    cov = cm.coverage(walker130["info"])
    print(dict(zip(cm.BRANCHES, cov)))
    assert min(cov) >= 0.05, dict(zip(cm.BRANCHES, cov))
    assert bool(cm.margins_ok(walker130["info"]).all())


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_walker_against_the_composition(rbd, walker130, layout):
    """q̄, v̄, s̄, τ̄, f̄ext of one rbd_dynamics_contact_vjp call at 1e-10·(1 + max|ref|) of the composition; v̇ and ṡ at 1e-10 of oracle.dynamics_contact."""
    w = walker130
    got, vd, sd = fused(rbd, w["flat"], w["B"], *w["inputs"], *w["cot"], layout=layout)
    for name, g, r in zip(NAMES, got, w["ref"]):
        close(g, r, 1e-10, name)
    rel = lambda x, y: np.abs(x - y).max() / max(1.0, np.abs(y).max())
    assert rel(vd, w["vd"]) <= 1e-10 and rel(sd, w["sd"]) <= 1e-10


def test_walker_partial_cotangents_and_outputs(rbd, walker130):
    """v̇̄ alone, and ṡ̄ / s̄_out without v̇̄ (τ̄ and f̄ext are then zero), against the composition; a call that asks for s̄ alone returns the same s̄."""
    w = walker130
    flat, B, (q, v, s, tau, fext), (a, b, c) = w["flat"], w["B"], w["inputs"], w["cot"]
    zs, zv = np.zeros((B, flat.ns)), np.zeros((B, flat.nv))
    for cot, ref_cot in (((a, None, None), (a, zs, zs)), ((None, b, c), (zv, b, c))):
        ref, _, _ = w["case"].composition(q, v, s, tau, fext, *ref_cot)
        got, _, _ = fused(rbd, flat, B, q, v, s, tau, fext, *cot)
        for name, g, r in zip(NAMES, got, ref):
            close(g, r, 1e-10, name)
    st = rbd.MechanismState(flat, B)
    sb = torch.full((B, flat.ns), float("nan"), dtype=torch.float64, device="cuda")
    rbd.dynamics_contact_vjp_(st, dev(a), dev(b), dev(c), dev(tau), dev(fext), s_bar=sb, q=dev(q), v=dev(v), s=dev(s))
    close(host(sb), w["ref"][2], 1e-10, "s_bar alone")


def test_contact_dynamics_vjp_alone(rbd, walker130):
    """rbd_contact_dynamics_vjp (cw_bar, sdot_bar, s_out_bar) against the composition without the dynamics, each cotangent alone too; a state with every
    pair outside gives q̄ = v̄ = s̄ = 0 exactly."""
    w = walker130
    flat, B, (q, v, s, tau, fext), (_, b, c) = w["flat"], w["B"], w["inputs"], w["cot"]
    cwb = w["rng"].standard_normal((B, 6 * flat.n_bodies))
    st = rbd.MechanismState(flat, B)
    nan = lambda n: torch.full((B, n), float("nan"), dtype=torch.float64, device="cuda")
    z = lambda x: np.zeros_like(x)
    for use in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        ref, _, _ = w["case"].composition(q, v, s, tau, fext, None, b if use[1] else z(b), c if use[2] else z(c), cw_bar=cwb if use[0] else z(cwb))
        out = [nan(flat.nq), nan(flat.nv), nan(flat.ns)]
        rbd.contact_dynamics_vjp_(st, dev(cwb) if use[0] else None, dev(b) if use[1] else None, dev(c) if use[2] else None, *out, q=dev(q), v=dev(v), s=dev(s))
        assert "contact_adjoint_kernel" in rbd.last_kernel(st)
        for name, g, r in zip(NAMES, out, ref[:3]):
            close(host(g), r, 1e-10, name)
    # far on the outer side of both half-spaces: the floating joint's translation moves the world position by pred_rot · t
    nrm = np.array([h["outward_normal"] / np.linalg.norm(h["outward_normal"]) for h in flat.halfspaces])
    qo = q.copy()
    qo[:, 4:7] = flat.pred_rot[0].T @ (20.0 * nrm.sum(axis=0))
    _, info, _ = w["case"].composition(qo, v, s, tau, fext, None, b, c, cw_bar=cwb)
    assert not bool(info["inside"].any())
    out = [nan(flat.nq), nan(flat.nv), nan(flat.ns)]
    rbd.contact_dynamics_vjp_(st, dev(cwb), dev(b), dev(c), *out, q=dev(qo), v=dev(v), s=dev(s))
    assert all(bool((o == 0).all()) for o in out)


def with_contact(flat, points, halfspaces):
    """A copy of a flat model with contact points (dicts as FlatModel keeps them) and half-spaces."""
    m = copy.copy(flat)
    m.contact_points, m.halfspaces = points, halfspaces
    m.ns = 3 * len(points) * len(halfspaces)
    m._c = None
    m.__dict__.pop("_rbd_model", None)  # (the library's model cached on the copied object is the one without contact points)
    return m


def cond_bound(oracle, flat, q):
    """1e-10, or 1e-14·cond(M) where that is larger (test_contact.py's bound for v̇ of the 70-body tree): the two routes solve with M for total wrenches that
    differ by rounding."""
    M = oracle.mass_matrix(flat, q)
    Ms = np.tril(M) + np.transpose(np.tril(M, -1), (0, 2, 1))
    return max(1e-10, 1e-14 * np.linalg.cond(Ms).max())


def test_atlas_floating(rbd, oracle, models):
    """Atlas on a floating base, B = 67: two contact points on each foot body, one floor; the pelvis height per state puts the lowest foot point between 3 cm
    under and 1 cm over the floor, so that some feet touch and some do not."""
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
    case = Case(rbd, flat, bare, B)
    pos = torch.empty(B, 12, dtype=torch.float64, device="cuda")
    rbd.point_kinematics_(case.ref, pos, q=dev(q), v=dev(v))
    low = host(pos).reshape(B, 4, 3)[:, :, 2].min(axis=1)
    q[:, 4:7] = (rng.uniform(-0.03, 0.01, B) - low)[:, None] * up
    s = 1e-3 * rng.standard_normal((B, flat.ns))
    tau, fext = rng.random((B, flat.nv)), rng.random((B, 6 * flat.n_bodies))
    a, b, c = cotangents(flat, B, rng)
    ref, info, _ = case.composition(q, v, s, tau, fext, a, b, c)
    inside = info["inside"]
    assert bool(inside.any()) and not bool(inside.all()) and bool(cm.margins_ok(info).all())
    got, vd, sd = fused(rbd, flat, B, q, v, s, tau, fext, a, b, c)
    tol = cond_bound(oracle, bare, q)
    for name, g, r in zip(NAMES, got, ref):
        close(g, r, tol, name)
    vd_ref, _, sd_ref, _, _ = oracle.dynamics_contact(flat, q, v, s, tau, fext)
    close(vd, vd_ref, tol, "vdot")
    close(sd, sd_ref, 1e-10, "sdot")


def test_tree_of_more_than_64_bodies(rbd, oracle):
    """The 70-body tree of test_contact.py's any-size test with three contact points and one half-space, B = 8."""
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
    tau, fext = rng.random((B, flat.nv)), rng.random((B, 6 * flat.n_bodies))
    a, b, c = cotangents(flat, B, rng)
    case = Case(rbd, flat, bare, B)
    ref, info, _ = case.composition(q, v, s, tau, fext, a, b, c)
    assert bool(info["inside"].any()) and not bool(info["inside"].all()) and bool(cm.margins_ok(info).all())
    got, vd, sd = fused(rbd, flat, B, q, v, s, tau, fext, a, b, c)
    tol = cond_bound(oracle, bare, q)
    for name, g, r in zip(NAMES, got, ref):
        close(g, r, tol, name)
    vd_ref, _, sd_ref, _, _ = oracle.dynamics_contact(flat, q, v, s, tau, fext)
    close(vd, vd_ref, tol, "vdot")
    close(sd, sd_ref, 1e-10, "sdot")


def test_a_callers_points_survive(rbd, walker130):
    """The contact points' path tables are the workspace's own: rbd_point_kinematics gives the same positions before and after a contact VJP."""
    w = walker130
    flat, B, (q, v, s, tau, fext), cot = w["flat"], w["B"], w["inputs"], w["cot"]
    st = rbd.MechanismState(flat, B)
    rbd.set_points_(st, [1, 4], [[0.1, 0.2, 0.3], [-0.2, 0.0, 0.4]])
    p0, p1 = (torch.full((B, 6), float("nan"), dtype=torch.float64, device="cuda") for _ in range(2))
    rbd.point_kinematics_(st, p0, q=dev(q), v=dev(v))
    fused(rbd, flat, B, q, v, s, tau, fext, *cot, state=st)
    rbd.point_kinematics_(st, p1, q=dev(q), v=dev(v))
    assert bool(torch.isfinite(p0).all()) and torch.equal(p0, p1) and st.npoints == 2


def test_fp32_against_fp64(rbd):
    """fp32, walker, B = 64, on states a factor 1e-3 clear of the branch boundaries (fp32 rounds at 6e-8): per output, the error of the fp32 call against the
    fp64 call is at most 4 × the error of the composition in fp32 against itself in fp64, plus 1e-6 (errors relative to 1 + max|fp64 value|)."""
    flat, bare = walker_pair(rbd)
    B = 64
    rng, q, v, s, tau, fext = walker_inputs(rbd, flat, B, seed=6, vscales=(1.0,))
    a, b, c = cotangents(flat, B, rng)
    ref64, info, _ = Case(rbd, flat, bare, B).composition(q, v, s, tau, fext, a, b, c)
    assert bool(cm.margins_ok(info, rel=1e-3).all())
    ref32, info32, _ = Case(rbd, flat, bare, B, dtype=torch.float32).composition(q, v, s, tau, fext, a, b, c)
    assert torch.equal(cm.branch_of(info), cm.branch_of(info32))
    got64, _, _ = fused(rbd, flat, B, q, v, s, tau, fext, a, b, c)
    got32, _, _ = fused(rbd, flat, B, q, v, s, tau, fext, a, b, c, dtype=torch.float32)
    e = lambda x, r: np.abs(x - r).max() / (1 + np.abs(r).max())
    bad = []
    for name, g32, g64, r32, r64 in zip(NAMES, got32, got64, ref32, ref64):
        ours, theirs = e(g32, g64), e(r32, r64)
        print("%-9s fp32 call %.3e  fp32 composition %.3e  ratio %.2f" % (name, ours, theirs, ours / max(theirs, 1e-300)))
        if not ours <= 4 * theirs + 1e-6:
            bad.append((name, ours, theirs))
    assert not bad, bad


def test_errors_and_no_ops(rbd, models, walker130):
    from rigidbodydynamics_jl_amd import _capi
    L, p = _capi.lib(), (lambda t: ctypes.c_void_p(t.data_ptr()))
    w = walker130
    flat, B = w["flat"], w["B"]
    st = rbd.MechanismState(flat, B)
    z = lambda n, b=B: torch.zeros(b, n, dtype=torch.float64, device="cuda")
    s, vb, sb, qb = z(flat.ns), z(flat.nv), z(flat.ns), z(flat.nq)
    opts = st._opts()

    def both(state, batch, q, v, s, vbar, sbar, out, o):
        h = state.ws.handle
        return (L.rbd_dynamics_contact_vjp(h, batch, q, v, s, None, None, vbar, sbar, None, None, None, out, None, None, None, None, ctypes.byref(o)),
                L.rbd_contact_dynamics_vjp(h, batch, q, v, s, None, sbar, None, out, None, None, ctypes.byref(o)))
    # a model without contact points: RBD_ERR_INVALID_ARGUMENT, as rbd_contact_dynamics
    dp = rbd.MechanismState(models["double_pendulum"], 4)
    z4 = torch.zeros(4, 8, dtype=torch.float64, device="cuda")
    assert both(dp, 4, p(dp.q), p(dp.v), p(z4), p(z4), p(z4), p(z4), dp._opts()) == (1, 1)
    # loop joints: RBD_ERR_HAS_LOOPS
    fb = rbd.MechanismState(models["four_bar"], 4)
    assert both(fb, 4, p(fb.q), p(fb.v), p(z4), p(z4), p(z4), p(z4), fb._opts()) == (7, 7)
    # host memory: RBD_ERR_UNSUPPORTED
    hopts = _capi.Opts(opts.layout, _capi.MEM_HOST, opts.algorithm, opts.stabilization)
    assert both(st, B, p(st.q), p(st.v), p(s), p(vb), p(sb), p(qb), hopts) == (3, 3)
    # every cotangent NULL, or a NULL q / v / s: RBD_ERR_INVALID_ARGUMENT
    assert both(st, B, p(st.q), p(st.v), p(s), None, None, p(qb), opts) == (1, 1)
    assert both(st, B, None, p(st.v), p(s), p(vb), p(sb), p(qb), opts) == (1, 1)
    assert both(st, B, p(st.q), p(st.v), None, p(vb), p(sb), p(qb), opts) == (1, 1)
    # B == 0: a successful no-op; a batch beyond the workspace's: RBD_ERR_DIMENSION_MISMATCH
    qb.fill_(float("nan"))
    assert both(st, 0, p(st.q), p(st.v), p(s), p(vb), p(sb), p(qb), opts) == (0, 0)
    assert rbd.sync(st) == 0 and bool(torch.isnan(qb).all())
    assert both(st, B + 1, p(st.q), p(st.v), p(s), p(vb), p(sb), p(qb), opts) == (2, 2)
    # the existing derivative entry points keep refusing the model
    assert L.rbd_dynamics_vjp(st.ws.handle, B, p(st.q), p(st.v), None, None, p(vb), None, p(qb), None, None, None, ctypes.byref(opts)) == 3


def test_second_call_allocates_nothing(rbd, walker130):
    w = walker130
    flat, B, (q, v, s, tau, fext), (a, b, c) = w["flat"], w["B"], w["inputs"], w["cot"]
    st = rbd.MechanismState(flat, B)
    t = [dev(x) for x in (a, b, c, tau, fext)]  # (every tensor of the test made before the measurement)
    qd, vd_, sd_ = dev(q), dev(v), dev(s)
    out = [torch.empty(B, n, dtype=torch.float64, device="cuda") for n in (flat.nq, flat.nv, flat.ns, flat.nv, 6 * flat.n_bodies)]
    rbd.dynamics_contact_vjp_(st, *t, *out, q=qd, v=vd_, s=sd_)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    rbd.dynamics_contact_vjp_(st, *t, *out, q=qd, v=vd_, s=sd_)
    rbd.contact_dynamics_vjp_(st, t[4], t[1], t[2], *out[:3], q=qd, v=vd_, s=sd_)
    rbd.dynamics_contact_vjp_(st, None, t[1], None, None, None, *out[:3], q=qd, v=vd_, s=sd_)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0


def test_autograd_gradcheck(rbd):
    """torch.autograd.gradcheck (reverse mode) through autograd.dynamics_contact on the walker, B = 3, on states 1e-3 clear of the branch boundaries (gradcheck
    steps by 1e-6), the quaternion normalised in torch: the value is the articulated-body route's, a different function of raw q off the unit sphere."""
    from test_vjp_gpu import on_manifold
    flat, _ = walker_pair(rbd)
    B = 3
    rng, q, v, s, tau, fext = walker_inputs(rbd, flat, B, seed=5, vscales=(1.0,))
    info = cm.oracle_pair_info(__import__("oracle"), flat, q, v, s)
    assert bool(cm.margins_ok(info, rel=1e-3).all()) and bool(info["inside"].any())
    st = rbd.MechanismState(flat, B)
    g = lambda x: torch.tensor(x, dtype=torch.float64, device="cuda", requires_grad=True)
    f = lambda qq, *r: rbd.autograd.dynamics_contact(st, on_manifold(rbd, flat, qq), *r)
    assert torch.autograd.gradcheck(f, (g(q), g(v), g(s), g(tau), g(fext)))
    assert torch.autograd.gradcheck(f, (g(q), g(v), g(s)))  # (without the optional inputs)
    with pytest.raises(Exception):  # no jvp rule
        torch.func.jvp(lambda vv: rbd.autograd.dynamics_contact(st, g(q), vv, g(s))[0], (g(v),), (torch.ones_like(g(v)),))


def test_backward_through_an_euler_rollout(rbd):
    """loss.backward() through 5 explicit-Euler steps written in torch (q̇ from v for the floating joint and the 1-dof joints of the walker, the friction state
    integrated beside) gives finite, non-zero gradients in q₀, v₀, s₀ and every step's τ."""
    flat, _ = walker_pair(rbd)
    B, dt = 16, 1e-3
    rng, q, v, s, tau, _ = walker_inputs(rbd, flat, B, vscales=(1.0,))
    st = rbd.MechanismState(flat, B)
    g = lambda x: torch.tensor(x, dtype=torch.float64, device="cuda", requires_grad=True)
    q0, v0, s0 = g(q), g(v), g(s)
    taus = [g(tau * (k + 1) / 5) for k in range(5)]

    def qdot(qq, vv):  # QuaternionFloating (body-frame angular and linear velocity), then q̇ = v
        w, x, y, z = qq[:, 0], qq[:, 1], qq[:, 2], qq[:, 3]
        om, lin = vv[:, :3], vv[:, 3:6]
        quat = 0.5 * torch.stack([-x * om[:, 0] - y * om[:, 1] - z * om[:, 2], w * om[:, 0] + y * om[:, 2] - z * om[:, 1],
                                  w * om[:, 1] + z * om[:, 0] - x * om[:, 2], w * om[:, 2] + x * om[:, 1] - y * om[:, 0]], dim=1)
        u = qq[:, 1:4]
        rot = lin + 2 * torch.linalg.cross(u, torch.linalg.cross(u, lin) + w[:, None] * lin)
        return torch.cat([quat, rot, vv[:, 6:]], dim=1)

    qk, vk, sk = q0, v0, s0
    for k in range(5):
        vd, sd, s_out = rbd.autograd.dynamics_contact(st, qk, vk, sk, taus[k])
        qk, vk, sk = qk + dt * qdot(qk, vk), vk + dt * vd, s_out + dt * sd
    (qk.square().sum() + vk.square().sum() + sk.square().sum()).backward()
    for name, t in [("q0", q0), ("v0", v0), ("s0", s0)] + [("tau%d" % k, t) for k, t in enumerate(taus)]:
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any()), name
