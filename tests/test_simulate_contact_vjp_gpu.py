"""Reverse mode through simulate steps with soft contact on the GPU (rbd_simulate_contact_vjp, autograd.simulate_contact).  The reference is exact, a
composition of merged parts: backward() through the Munthe-Kaas RK4 step written in torch (tests/simulate_contact_ref.py, pinned to oracle/simulate_np.py by
test_simulate_contact_vjp_cpu.py) around autograd.dynamics_contact, whose pullback is rbd_dynamics_contact_vjp; the pair info of every stage state comes from
point kinematics on the bare model and the torch pair model (tests/contact_model_ref.py).  No difference quotients (gradcheck apart, which is torch's own)."""
import ctypes

import numpy as np
import pytest
import torch

import contact_model_ref as cm
import simulate_contact_ref as sr
from conftest import tune
from test_contact_vjp_gpu import Case, close, cond_bound, dev, host, interpreting_kernels, walker_inputs, walker_pair, with_contact  # noqa: F401 (the fixture is autouse)

pytestmark = pytest.mark.gpu
NAMES = ("q_bar", "v_bar", "s_bar", "tau_bar", "fext_bar")
DT = 1e-3


class Reference:
    """The torch step over autograd.dynamics_contact for a mechanism with contact (flat) — and, for the pair info of every stage state, the same mechanism
    without (bare) with the contact points set as points."""

    def __init__(self, rbd, flat, bare, B, dtype=torch.float64):
        self.rbd, self.flat, self.B, self.dtype = rbd, flat, B, dtype
        self.st = rbd.MechanismState(flat, B, dtype=dtype)
        self.case = Case(rbd, flat, bare, B, dtype)

    def dynamics(self, tau, fext):
        def f(q, v, s):
            vd, sd, _ = self.rbd.autograd.dynamics_contact(self.st, q, v, s, tau, fext)
            with torch.no_grad():
                pos, vel = (torch.empty(self.B, 3 * len(self.flat.contact_points), dtype=self.dtype, device="cuda") for _ in range(2))
                self.rbd.point_kinematics_(self.case.ref, pos, vel, q=q.detach().contiguous(), v=v.detach().contiguous())
                info = cm.contact_model(self.flat, pos, vel, s.detach(), self.case.tab)[3]
            return vd, sd, {k: x.cpu() for k, x in info.items()}
        return f

    def run(self, q, v, s, tau, fext, cot, nsteps, dt=DT):
        """backward() of Σ q⁺·a + Σ v⁺·b + Σ s⁺·c through nsteps steps; numpy (B, n) in; the five gradients, the final state (fp64 numpy) and the pair info of
        every stage of every step out."""
        D = lambda x: None if x is None else dev(x, dtype=self.dtype)
        qq, vv, ss = (D(x).requires_grad_(True) for x in (q, v, s))
        tt, ff = (None if x is None else D(x).requires_grad_(True) for x in (tau, fext))
        q1, v1, s1, infos = sr.rollout(self.flat, qq, vv, ss, dt, nsteps, self.dynamics(tt, ff))
        ((q1 * D(cot[0])).sum() + (v1 * D(cot[1])).sum() + (s1 * D(cot[2])).sum()).backward()
        grads = [None if x is None else host(x.grad) if x.grad is not None else np.zeros(x.shape) for x in (qq, vv, ss, tt, ff)]
        return grads, (host(q1), host(v1), host(s1)), infos


def call(rbd, flat, B, q, v, s, tau, fext, cot, nsteps, dt=DT, layout="aos", dtype=torch.float64, want=(True, True), state=None):
    """One rbd_simulate_contact_vjp call on NaN-prefilled τ̄ / f̄ext: the five gradients (None where not asked for) and the final (q, v, s), fp64 numpy (B, n)."""
    st = state or rbd.MechanismState(flat, B, dtype=dtype, layout=layout)
    D = lambda x: None if x is None else dev(x, layout, dtype)
    nan = lambda n: torch.full((B, n) if layout == "aos" else (n, B), float("nan"), dtype=dtype, device="cuda")
    qd, vd, sd = D(q), D(v), D(s)
    qb, vb, sb = (D(x) for x in cot)
    tb, fb = nan(flat.nv) if want[0] else None, nan(6 * flat.n_bodies) if want[1] else None
    rbd.simulate_contact_vjp_(qb, vb, sb, st, dt, nsteps, torques=D(tau), externalwrenches=D(fext), tau_bar=tb, fext_bar=fb, q=qd, v=vd, s=sd)
    assert rbd.sync(st) == 0
    if nsteps > 0:
        assert "contact_stage_adjoint_kernel" in rbd.last_kernel(st)
    H = lambda x: None if x is None else host(x, layout)
    return [H(x) for x in (qb, vb, sb, tb, fb)], (H(qd), H(vd), H(sd))


def cotangents(flat, B, rng):
    return rng.standard_normal((B, flat.nq)), rng.standard_normal((B, flat.nv)), rng.standard_normal((B, flat.ns))


def canon(q):
    """the floating base's quaternion up to sign (q and −q are the same rotation)"""
    q = q.copy()
    sg = np.sign(q[:, :1])
    sg[sg == 0] = 1
    q[:, :4] *= sg
    return q


def stages(infos):
    return [info for step in infos for info in step]


def all_margins(infos, rel=1e-6):
    """per state: every pair at every stage of every step holds the branch margins"""
    ok = torch.stack([cm.margins_ok(i, rel).reshape(i["inside"].shape[0], -1).all(dim=1) for i in stages(infos)])
    return ok.all(dim=0)


def branches(infos):
    return torch.stack([cm.branch_of(i) for i in stages(infos)])  # (stages, B, P, H)


def np_rollout(oracle, flat, q, v, s, tau, fext, nsteps, dt=DT):
    """simulate_np.step_contact for the whole batch, with external wrenches (step_contact itself takes none): its local_rate / global_coordinates in their
    batched forms around oracle.dynamics_contact."""
    import simulate_np as snp
    q, v, s = q.copy(), v.copy(), s.copy()
    for _ in range(nsteps):
        phids, vds, sds = [], [], []
        for i in range(4):
            a = 0.0 if i == 0 else dt * sr.RK4_A[i - 1]
            qq = snp.global_coordinates_batch(flat, q, a * phids[-1]) if i else q
            vv, ss = (v + a * vds[-1], s + a * sds[-1]) if i else (v, s)
            vd, _, sd, _, _ = oracle.dynamics_contact(flat, qq, vv, ss, tau, fext)
            vds.append(vd); sds.append(sd)
            phids.append(snp.local_rate_batch(flat, q, qq, vv))
        comb = lambda xs: sum(dt * sr.RK4_B[i] * xs[i] for i in range(4))
        q, v, s = snp.global_coordinates_batch(flat, q, comb(phids)), v + comb(vds), s + comb(sds)
    return q, v, s


def test_the_reference_is_rbd_simulate_vjp_without_contact(rbd):
    """The reference validated first: on the bare walker (no contact), B = 16, 3 steps, backward() through the torch step over autograd.dynamics equals
    rbd_simulate_vjp's (q̄, v̄, τ̄, f̄ext) at 1e-10·(1 + max|ref|)."""
    flat, bare = walker_pair(rbd)
    B = 16
    rng, q, v, _, tau, fext = walker_inputs(rbd, flat, B)
    a, b = rng.standard_normal((B, bare.nq)), rng.standard_normal((B, bare.nv))
    st = rbd.MechanismState(bare, B)
    qq, vv, tt, ff = (dev(x).requires_grad_(True) for x in (q, v, tau, fext))
    q1, v1, _, _ = sr.rollout(bare, qq, vv, None, DT, 3, lambda x, y, _s: (rbd.autograd.dynamics(st, x, y, tt, ff), None, None))
    ((q1 * dev(a)).sum() + (v1 * dev(b)).sum()).backward()
    qb, vb = dev(a), dev(b)
    tb, fb = (torch.full((B, n), float("nan"), dtype=torch.float64, device="cuda") for n in (bare.nv, 6 * bare.n_bodies))
    qd, vd = dev(q), dev(v)
    rbd.simulate_vjp_(qb, vb, st, DT, 3, torques=dev(tau), externalwrenches=dev(fext), tau_bar=tb, fext_bar=fb, q=qd, v=vd)
    for name, got, ref in zip(("q_bar", "v_bar", "tau_bar", "fext_bar"), (qb, vb, tb, fb), (qq, vv, tt, ff)):
        close(host(ref.grad), host(got), 1e-10, name)
    close(host(q1), host(qd), 1e-10, "q")
    close(host(v1), host(vd), 1e-10, "v")


@pytest.fixture(scope="module")
def walker130(rbd, oracle, interpreting_kernels):
    """The walker, B = 130, 3 steps: inputs, cotangents, the composition's gradients, final state and pair info (computed once, shared, left unchanged)."""
    flat, bare = walker_pair(rbd)
    B, nsteps = 130, 3
    rng, q, v, s, tau, fext = walker_inputs(rbd, flat, B, seed=5)
    cot = cotangents(flat, B, rng)
    ref = Reference(rbd, flat, bare, B)
    grads, final, infos = ref.run(q, v, s, tau, fext, cot, nsteps)
    return dict(flat=flat, bare=bare, B=B, nsteps=nsteps, inputs=(q, v, s, tau, fext), cot=cot, ref=grads, final=final, infos=infos, reference=ref, rng=rng)


def test_walker_conditions_hold(walker130):
    """Asserted, not assumed: every pair at every stage of every step is clear of the branch boundaries (rel 1e-6); at stage 0 every branch is taken by at
    least 5 % of the pairs; at least 10 % of the states have a pair whose branch differs between two stages."""
    infos = walker130["infos"]
    assert len(stages(infos)) == 12
    ok = all_margins(infos)
    cov = cm.coverage(infos[0][0])
    br = branches(infos)
    changed = (br != br[:1]).any(dim=0).reshape(walker130["B"], -1).any(dim=1)
    print("margins %d / %d" % (int(ok.sum()), ok.numel()), dict(zip(cm.BRANCHES, cov)), "states changing branch", int(changed.sum()))
    assert bool(ok.all())
    assert min(cov) >= 0.05, dict(zip(cm.BRANCHES, cov))
    assert float(changed.double().mean()) >= 0.10


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_walker_against_the_composition(rbd, oracle, walker130, layout):
    """q̄, v̄, s̄, τ̄, f̄ext of one call (3 steps, fext given and f̄ext asked for: a stage's contact pullback fed the accumulated f̄ext fails here) at
    1e-10·(1 + max|ref|) of the composition; the final (q, v, s) at 1e-10 of simulate_np's step with the oracle's dynamics! at every stage (quaternions up to
    sign) and of the composition's."""
    w = walker130
    got, final = call(rbd, w["flat"], w["B"], *w["inputs"], w["cot"], w["nsteps"], layout=layout)
    for name, g, r in zip(NAMES, got, w["ref"]):
        close(g, r, 1e-10, name)
    ref_state = np_rollout(oracle, w["flat"], *w["inputs"], w["nsteps"])
    for name, g, r, c in zip("qvs", final, ref_state, w["final"]):
        close(canon(g) if name == "q" else g, canon(r) if name == "q" else r, 1e-10, name + " (oracle)")
        close(canon(g) if name == "q" else g, canon(c) if name == "q" else c, 1e-10, name + " (composition)")


def test_partial_outputs_and_optional_inputs(rbd, oracle, walker130):
    """Without tau_bar / fext_bar the same q̄, v̄, s̄; without tau / fext the composition's gradients, and the final state of simulate_np.step_contact."""
    import simulate_np as snp
    w = walker130
    flat, B, (q, v, s, tau, fext), cot, n = w["flat"], w["B"], w["inputs"], w["cot"], w["nsteps"]
    full, _ = call(rbd, flat, B, q, v, s, tau, fext, cot, n)
    for want in ((False, False), (True, False), (False, True)):
        got, _ = call(rbd, flat, B, q, v, s, tau, fext, cot, n, want=want)
        for name, g, r in zip(NAMES, got, full):
            if g is None:
                continue
            assert np.array_equal(g, r), (want, name)
        assert (got[3] is None) == (not want[0]) and (got[4] is None) == (not want[1])
    ref, rfinal, _ = w["reference"].run(q, v, s, None, None, cot, n)
    got, final = call(rbd, flat, B, q, v, s, None, None, cot, n)
    for name, g, r in zip(NAMES[:3], got, ref):
        close(g, r, 1e-10, name + " (no tau, no fext)")
    assert np.isfinite(got[3]).all() and np.isfinite(got[4]).all()
    rq, rv, rs = q.copy(), v.copy(), s.copy()
    for _ in range(n):
        for b in range(B):
            rq[b], rv[b], rs[b] = snp.step_contact(flat, rq[b], rv[b], rs[b], DT)
    for name, g, r in zip("qvs", final, (rq, rv, rs)):
        close(canon(g) if name == "q" else g, canon(r) if name == "q" else r, 1e-10, name + " (step_contact)")


def test_no_contact_anywhere_is_rbd_simulate_vjp(rbd, walker130):
    """The walker 5 m clear of both half-spaces, B = 16, 2 steps: q̄, v̄, τ̄, f̄ext equal rbd_simulate_vjp on the bare model at 1e-12·(1 + max); s_bar returns
    bit-identical (a pair outside at all four stages passes s̄⁺ through) and s is unchanged."""
    w = walker130
    flat, bare, B = w["flat"], w["bare"], 16
    q, v, s, tau, fext = (x[:B].copy() for x in w["inputs"])
    cot = tuple(x[:B].copy() for x in w["cot"])
    nrm = np.array([h["outward_normal"] / np.linalg.norm(h["outward_normal"]) for h in flat.halfspaces])
    assert nrm[0] @ nrm[1] > 0  # (moving along the sum of the normals leaves both half-spaces)
    q[:, 4:7] += flat.pred_rot[0].T @ (5.0 * nrm.sum(axis=0))
    _, _, infos = Reference(rbd, flat, bare, B).run(q, v, s, tau, fext, cot, 2)
    assert not any(bool(i["inside"].any()) for i in stages(infos)) and min(float(i["sep"].min()) for i in stages(infos)) > 1.0
    got, final = call(rbd, flat, B, q, v, s, tau, fext, cot, 2)
    st = rbd.MechanismState(bare, B)
    qb, vb, qd, vd = dev(cot[0]), dev(cot[1]), dev(q), dev(v)
    tb, fb = (torch.full((B, n), float("nan"), dtype=torch.float64, device="cuda") for n in (bare.nv, 6 * bare.n_bodies))
    rbd.simulate_vjp_(qb, vb, st, DT, 2, torques=dev(tau), externalwrenches=dev(fext), tau_bar=tb, fext_bar=fb, q=qd, v=vd)
    for name, g, r in zip(("q_bar", "v_bar", "tau_bar", "fext_bar"), (got[0], got[1], got[3], got[4]), (qb, vb, tb, fb)):
        close(g, host(r), 1e-12, name)
    close(final[0], host(qd), 1e-12, "q")
    close(final[1], host(vd), 1e-12, "v")
    assert np.array_equal(got[2], cot[2]) and np.array_equal(final[2], s)


def test_one_call_equals_chained_one_step_calls(rbd, walker130):
    """One 5-step call equals five 1-step calls — the states forward, then the cotangents chained backward, τ̄ and f̄ext summed — at 1e-12·(1 + max)."""
    w = walker130
    flat, B = w["flat"], 32
    q, v, s, tau, fext = (x[:B].copy() for x in w["inputs"])
    cot = tuple(x[:B].copy() for x in w["cot"])
    one, final = call(rbd, flat, B, q, v, s, tau, fext, cot, 5)
    st = rbd.MechanismState(flat, B)
    states = [(q, v, s)]
    for _ in range(4):
        _, nxt = call(rbd, flat, B, *states[-1], tau, fext, cot, 1, state=st)
        states.append(nxt)
    tb, fb = 0.0, 0.0
    for k in reversed(range(5)):
        g, nxt = call(rbd, flat, B, *states[k], tau, fext, cot, 1, state=st)
        if k == 4:
            for name, a, b in zip("qvs", nxt, final):
                close(a, b, 1e-12, name)
        cot, tb, fb = tuple(g[:3]), tb + g[3], fb + g[4]
    for name, g, r in zip(NAMES, list(cot) + [tb, fb], one):
        close(g, r, 1e-12, name)


def test_two_level_checkpoints_include_s(rbd, walker130, monkeypatch):
    """7 steps with room for 2 step starts (every 3rd kept, the segments' others recomputed, the friction state in the slots; 7 is no multiple of 3) gives
    what keeping every start gives, at 1e-12·(1 + max)."""
    w = walker130
    flat, B = w["flat"], 32
    q, v, s, tau, fext = (x[:B].copy() for x in w["inputs"])
    cot = tuple(x[:B].copy() for x in w["cot"])
    ref, rfinal = call(rbd, flat, B, q, v, s, tau, fext, cot, 7)
    tune(monkeypatch, sim_vjp_ckpt_steps=2)
    got, final = call(rbd, flat, B, q, v, s, tau, fext, cot, 7)
    for name, g, r in zip(NAMES + ("q", "v", "s"), got + list(final), ref + list(rfinal)):
        close(g, r, 1e-12, name)


def atlas_with_feet(rbd, bare, B, rng, position):
    """test_atlas_floating's construction: two contact points on each foot body, one floor; the pelvis height per state puts the lowest foot point between
    3 cm under and 1 cm over the floor.  position(flat, q, v) -> the contact points' positions (B, P, 3)."""
    feet = [bare.body_names.index(n) for n in ("l_foot", "r_foot")]
    hc = rbd.hunt_crossley_hertz()
    par = dict(hc_k=hc.k, hc_lambda=hc.lam, hc_n=hc.n, mu=0.8, k=20e3, b=100.0)
    pts = [dict(par, body=f, location=np.array([x, 0.0, -0.08])) for f in feet for x in (0.15, -0.08)]
    flat = with_contact(bare, pts, [dict(point=np.zeros(3), outward_normal=np.array([0.0, 0.0, 1.0]))])
    q, v = rbd.rand_configuration(bare, B, rng), rbd.rand_velocity(bare, B, rng)
    up = bare.pred_rot[0].T @ np.array([0.0, 0.0, 1.0])
    q[:, 4:7] = 0
    low = position(flat, q, v)[:, :, 2].min(axis=1)
    q[:, 4:7] = (rng.uniform(-0.03, 0.01, B) - low)[:, None] * up
    return flat, q, v


def gpu_positions(rbd, bare, B):
    def position(flat, q, v):
        st = rbd.MechanismState(bare, B)
        rbd.set_points_(st, [c["body"] for c in flat.contact_points], [c["location"] for c in flat.contact_points])
        pos = torch.empty(B, 3 * len(flat.contact_points), dtype=torch.float64, device="cuda")
        rbd.point_kinematics_(st, pos, q=dev(q), v=dev(v))
        return host(pos).reshape(B, -1, 3)
    return position


def test_atlas_floating(rbd, oracle, models):
    """Atlas on a floating base with test_atlas_floating's feet and floor, B = 67, 2 steps, at cond_bound (max(1e-10, 1e-14·cond M)): some pairs inside and some
    not, margins at every stage."""
    bare = models["atlas_floating"]
    B = 67
    rng = np.random.default_rng(23)
    flat, q, v = atlas_with_feet(rbd, bare, B, rng, gpu_positions(rbd, bare, B))
    s = 1e-3 * rng.standard_normal((B, flat.ns))
    tau, fext = rng.random((B, flat.nv)), rng.random((B, 6 * flat.n_bodies))
    cot = cotangents(flat, B, rng)
    ref, rfinal, infos = Reference(rbd, flat, bare, B).run(q, v, s, tau, fext, cot, 2)
    inside = torch.stack([i["inside"] for i in stages(infos)])
    assert bool(inside.any()) and not bool(inside.all()) and bool(all_margins(infos).all())
    got, final = call(rbd, flat, B, q, v, s, tau, fext, cot, 2)
    tol = cond_bound(oracle, bare, q)
    for name, g, r in zip(NAMES + ("q", "v", "s"), got + list(final), ref + list(rfinal)):
        close(g, r, tol, name)


def big_tree(rbd, bare):
    """The 70-body tree of test_tree_of_more_than_64_bodies: three contact points, one half-space."""
    rng = np.random.default_rng(15)
    mech = rbd.rand_tree_mechanism(rng, ["QuaternionFloating"] + ["Revolute"] * 69)
    for k in (3, 35, 69):
        model = rbd.SoftContactModel(rbd.hunt_crossley_hertz(k=2e3 * (1 + rng.random()), alpha=0.3 * rng.random()),
                                     rbd.ViscoelasticCoulombModel(0.3 + rng.random(), 1e3 * (1 + rng.random()), 1e2 * (1 + rng.random())))
        rbd.add_contact_point_(mech.bodies[1:][k], rbd.ContactPoint(0.3 * rng.standard_normal(3), model))
    rbd.add_environment_primitive_(mech, rbd.HalfSpace3D([0, 0, 0.2], [0.1, -0.2, 1.0]))
    return rbd.flatten(cm.strip_contact(mech) if bare else mech), rng


def test_tree_of_more_than_64_bodies(rbd, oracle):
    """The 70-body tree (per-body kinematics from the any-size kernels), B = 8, 1 step, at cond_bound."""
    (flat, rng), (bare, _) = big_tree(rbd, False), big_tree(rbd, True)
    assert flat.n_bodies == 70 and flat.ns == 9
    B = 8
    q, v = rbd.rand_configuration(flat, B, rng), rbd.rand_velocity(flat, B, rng)
    s = 1e-3 * rng.standard_normal((B, flat.ns))
    tau, fext = rng.random((B, flat.nv)), rng.random((B, 6 * flat.n_bodies))
    cot = cotangents(flat, B, rng)
    ref, rfinal, infos = Reference(rbd, flat, bare, B).run(q, v, s, tau, fext, cot, 1)
    inside = torch.stack([i["inside"] for i in stages(infos)])
    assert bool(inside.any()) and not bool(inside.all()) and bool(all_margins(infos).all())
    got, final = call(rbd, flat, B, q, v, s, tau, fext, cot, 1)
    tol = cond_bound(oracle, bare, q)
    for name, g, r in zip(NAMES + ("q", "v", "s"), got + list(final), ref + list(rfinal)):
        close(g, r, tol, name)


def test_fp32_against_fp64(rbd):
    """fp32, walker, B = 64, 2 steps, on states a factor 1e-3 clear of the branch boundaries at every stage, whose fp32 and fp64 reference rollouts take the
    same branches: per output, the error of the fp32 call against the fp64 call is at most 4 × the error of the torch composition in fp32 against itself in
    fp64, plus 1e-6 (errors relative to 1 + max|fp64 value|).  dt = 5e-4: with 1e-3 one pair of state 63 comes within 8.2e-4 of the stick / slip boundary at
    the last stage of the second step (oracle, CPU), with 5e-4 all 64 states hold the margins at every stage."""
    flat, bare = walker_pair(rbd)
    B, n, dt = 64, 2, 5e-4
    rng, q, v, s, tau, fext = walker_inputs(rbd, flat, B, seed=6, vscales=(1.0,))
    cot = cotangents(flat, B, rng)
    ref64, _, infos = Reference(rbd, flat, bare, B).run(q, v, s, tau, fext, cot, n, dt=dt)
    ok = all_margins(infos, rel=1e-3)
    print("margins %d / %d" % (int(ok.sum()), B))
    assert bool(ok.all())
    ref32, _, infos32 = Reference(rbd, flat, bare, B, dtype=torch.float32).run(q, v, s, tau, fext, cot, n, dt=dt)
    assert torch.equal(branches(infos), branches(infos32))
    got64, _ = call(rbd, flat, B, q, v, s, tau, fext, cot, n, dt=dt)
    got32, _ = call(rbd, flat, B, q, v, s, tau, fext, cot, n, dt=dt, dtype=torch.float32)
    e = lambda x, r: np.abs(x - r).max() / (1 + np.abs(r).max())
    bad = []
    for name, g32, g64, r32, r64 in zip(NAMES, got32, got64, ref32, ref64):
        ours, theirs = e(g32, g64), e(r32, r64)
        print("%-9s fp32 call %.3e  fp32 composition %.3e  ratio %.2f" % (name, ours, theirs, ours / max(theirs, 1e-300)))
        assert np.isfinite(g32).all()
        if not ours <= 4 * theirs + 1e-6:
            bad.append((name, ours, theirs))
    assert not bad, bad


def test_errors_and_no_ops(rbd, models, walker130):
    L, p = rbd._capi.lib(), (lambda t: None if t is None else ctypes.c_void_p(t.data_ptr()))
    w = walker130
    flat, B = w["flat"], w["B"]
    st = rbd.MechanismState(flat, B)
    rbd.set_points_(st, [1, 4], [[0.1, 0.2, 0.3], [-0.2, 0.0, 0.4]])
    q, v, s, tau, fext = (dev(x) for x in w["inputs"])
    qb, vb, sb = (dev(x) for x in w["cot"])
    tb, fb = (torch.full((B, n), float("nan"), dtype=torch.float64, device="cuda") for n in (flat.nv, 6 * flat.n_bodies))
    opts = st._opts()

    def run(state=st, batch=B, q=q, v=v, s=s, dt=DT, n=1, qb=qb, vb=vb, sb=sb, o=opts, tb=tb, fb=fb):
        return L.rbd_simulate_contact_vjp(state.ws.handle, batch, p(q), p(v), p(s), p(tau), p(fext), ctypes.c_double(dt), n, p(qb), p(vb), p(sb), p(tb), p(fb),
                                          ctypes.byref(o))
    p0 = torch.full((B, 6), float("nan"), dtype=torch.float64, device="cuda")
    rbd.point_kinematics_(st, p0, q=q, v=v)
    keep = [x.clone() for x in (q, v, s, qb, vb, sb)]
    same = lambda: all(torch.equal(a, b) for a, b in zip(keep, (q, v, s, qb, vb, sb)))
    # dt <= 0, nsteps < 0, a NULL q, v, s, q̄, v̄ or s̄: RBD_ERR_INVALID_ARGUMENT
    for kw in (dict(dt=0.0), dict(dt=-DT), dict(dt=float("nan")), dict(n=-1), dict(q=None), dict(v=None), dict(s=None), dict(qb=None), dict(vb=None), dict(sb=None)):
        assert run(**kw) == 1, kw
    # host memory: RBD_ERR_UNSUPPORTED; a batch beyond the workspace's: RBD_ERR_DIMENSION_MISMATCH
    assert run(o=rbd._capi.Opts(opts.layout, rbd._capi.MEM_HOST, opts.algorithm, opts.stabilization)) == 3
    assert run(batch=B + 1) == 2
    # a model without contact points: RBD_ERR_INVALID_ARGUMENT; loop joints: RBD_ERR_HAS_LOOPS
    z4 = torch.zeros(4, 64, dtype=torch.float64, device="cuda")
    dp = rbd.MechanismState(models["double_pendulum"], 4)
    assert run(state=dp, batch=4, q=dp.q, v=dp.v, s=z4, qb=z4, vb=z4, sb=z4, o=dp._opts(), tb=None, fb=None) == 1
    four = rbd.MechanismState(models["four_bar"], 4)
    assert run(state=four, batch=4, q=four.q, v=four.v, s=z4, qb=z4, vb=z4, sb=z4, o=four._opts(), tb=None, fb=None) == 7
    assert rbd.sync(st) == 0 and same() and bool(torch.isnan(tb).all()) and bool(torch.isnan(fb).all())
    # B == 0: a successful no-op that writes nothing
    assert run(batch=0, n=3) == 0
    assert rbd.sync(st) == 0 and same() and bool(torch.isnan(tb).all()) and bool(torch.isnan(fb).all())
    # nsteps == 0: the state and the three cotangents as they were, τ̄ and f̄ext zeroed
    assert run(n=0) == 0
    assert rbd.sync(st) == 0 and same() and bool((tb == 0).all()) and bool((fb == 0).all())
    with pytest.raises(ValueError):
        rbd.simulate_contact_vjp_(qb, vb, sb, st, DT, -1)
    with pytest.raises(ValueError):
        rbd.simulate_contact_vjp_(qb, vb, None, st, DT)
    with pytest.raises(rbd.DimensionMismatch):
        rbd.simulate_contact_vjp_(qb, vb, torch.zeros((B, flat.ns + 1), dtype=torch.float64, device="cuda"), st, DT)
    # the contact-free rollout VJP keeps refusing the model
    assert L.rbd_simulate_vjp(st.ws.handle, B, p(q), p(v), None, None, ctypes.c_double(DT), 1, p(qb), p(vb), None, None, ctypes.byref(opts)) == 3
    # a real call, then: the caller's points are still the workspace's
    assert run(n=2) == 0 and rbd.sync(st) == 0 and not same()
    p1 = torch.full((B, 6), float("nan"), dtype=torch.float64, device="cuda")
    rbd.point_kinematics_(st, p1, q=keep[0], v=keep[1])
    assert bool(torch.isfinite(p0).all()) and torch.equal(p0, p1) and st.npoints == 2


def test_second_call_allocates_nothing(rbd, walker130):
    w = walker130
    flat, B = w["flat"], w["B"]
    st = rbd.MechanismState(flat, B)
    q, v, s, tau, fext = (dev(x) for x in w["inputs"])  # (every tensor of the test made before the measurement)
    qb, vb, sb = (dev(x) for x in w["cot"])
    tb, fb = (torch.empty(B, n, dtype=torch.float64, device="cuda") for n in (flat.nv, 6 * flat.n_bodies))
    rbd.simulate_contact_vjp_(qb, vb, sb, st, DT, 4, torques=tau, externalwrenches=fext, tau_bar=tb, fext_bar=fb, q=q, v=v, s=s)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    rbd.simulate_contact_vjp_(qb, vb, sb, st, DT, 4, torques=tau, externalwrenches=fext, tau_bar=tb, fext_bar=fb, q=q, v=v, s=s)
    rbd.simulate_contact_vjp_(qb, vb, sb, st, DT, 2, torques=tau, q=q, v=v, s=s)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0


def test_autograd_gradcheck(rbd):
    """torch.autograd.gradcheck (reverse mode) through autograd.simulate_contact on the walker, B = 3, 2 steps, on states 1e-3 clear of the branch boundaries
    at every stage (gradcheck steps by 1e-6), the quaternion normalised in torch: the value is the articulated-body route's, a different function of raw q
    off the unit sphere.  With and without the optional inputs; no jvp rule."""
    from test_vjp_gpu import on_manifold
    flat, bare = walker_pair(rbd)
    B = 3
    rng, q, v, s, tau, fext = walker_inputs(rbd, flat, B, seed=5, vscales=(1.0,))
    _, _, infos = Reference(rbd, flat, bare, B).run(q, v, s, tau, fext, cotangents(flat, B, rng), 2)
    assert bool(all_margins(infos, rel=1e-3).all()) and bool(torch.stack([i["inside"] for i in stages(infos)]).any())
    st = rbd.MechanismState(flat, B)
    g = lambda x: torch.tensor(x, dtype=torch.float64, device="cuda", requires_grad=True)
    f = lambda qq, *r: rbd.autograd.simulate_contact(st, on_manifold(rbd, flat, qq), *r, dt=DT, nsteps=2)
    assert torch.autograd.gradcheck(f, (g(q), g(v), g(s), g(tau), g(fext)))
    assert torch.autograd.gradcheck(f, (g(q), g(v), g(s)))  # (without the optional inputs)
    with pytest.raises(Exception):  # no jvp rule
        torch.func.jvp(lambda vv: rbd.autograd.simulate_contact(st, g(q), vv, g(s))[0], (g(v),), (torch.ones_like(g(v)),))


def test_backward_through_a_loop_of_one_step_calls(rbd):
    """loss.backward() through a Python loop of 5 one-step autograd.simulate_contact calls with a torque per step gives finite, non-zero gradients in q₀, v₀,
    s₀ and every τ_k, equal at 1e-12·(1 + max) to the chained rbd_simulate_contact_vjp calls from the same step starts."""
    flat, _ = walker_pair(rbd)
    B, N = 16, 5
    rng, q, v, s, tau, _ = walker_inputs(rbd, flat, B, vscales=(1.0,))
    st = rbd.MechanismState(flat, B)
    g = lambda x: torch.tensor(x, dtype=torch.float64, device="cuda", requires_grad=True)
    q0, v0, s0 = g(q), g(v), g(s)
    taus = [g(tau * (k + 1) / N) for k in range(N)]
    xs = [(q0, v0, s0)]
    for k in range(N):
        xs.append(rbd.autograd.simulate_contact(st, *xs[-1], taus[k], dt=DT))
    qk, vk, sk = xs[-1]
    (qk.square().sum() + vk.square().sum() + sk.square().sum()).backward()
    for name, t in [("q0", q0), ("v0", v0), ("s0", s0)] + [("tau%d" % k, t) for k, t in enumerate(taus)]:
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any()), name
    cot = [2 * x.detach().clone() for x in xs[-1]]
    for k in reversed(range(N)):
        qs, vs, ss = (x.detach().clone() for x in xs[k])
        tb = torch.full((B, flat.nv), float("nan"), dtype=torch.float64, device="cuda")
        rbd.simulate_contact_vjp_(*cot, st, DT, 1, torques=taus[k].detach(), tau_bar=tb, q=qs, v=vs, s=ss)
        close(host(taus[k].grad), host(tb), 1e-12, "tau%d" % k)
    for name, t, c in zip(("q0", "v0", "s0"), (q0, v0, s0), cot):
        close(host(t.grad), host(c), 1e-12, name)
