"""rbd_simulate_contact_controlled on the GPU: `simulate(state, T, control!)` of a mechanism with contact points under the device-side controllers, against
the numpy step with a controller (tests/simulate_contact_controlled_ref.py: oracle/simulate_np.py's step around oracle.dynamics_contact), against
rbd_simulate_contact (the CONSTANT kind: one code path since the fold of DESIGN.md §3.14) and what rbd_simulate_contact / rbd_dynamics_contact computed before
that fold (tests/golden/vectors/simulate_contact_parent.npz, recorded by tests/golden/make_simulate_contact_parent.py), and the Python callback path of
simulate_.  The conditions the parity tests assume of their inputs (branch margins,
pairs in and out of contact, branch changes) are asserted on the CPU, on the same inputs: test_simulate_contact_controlled_cpu.py."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

import simulate_contact_controlled_ref as ref

pytestmark = pytest.mark.gpu
DT = ref.DT


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
    """(..., B, n) numpy -> device tensor in the layout ((..., n, B) for soa); None stays None"""
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)
    return (t if layout == "aos" else t.transpose(-1, -2).contiguous()).cuda()


def host(t, layout="aos"):
    t = t.detach().double().cpu()
    return (t if layout == "aos" else t.t()).numpy().copy()


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def control(rbd, kind, tau=None, q_des=None, kp=None, kd=None, per_stage=0):
    c = rbd._capi.Control()
    c.kind, c.per_stage = kind, per_stage
    c.tau, c.q_des, c.kp, c.kd = (None if t is None else t.data_ptr() for t in (tau, q_des, kp, kd))
    c.keep = (tau, q_des, kp, kd)  # (the descriptor holds addresses only)
    return c


def simulate(rbd, st, q, v, s, ctl, fext, nsteps, dt=DT, B=None):
    """one rbd_simulate_contact_controlled call on device tensors; the status"""
    return rbd._capi.lib().rbd_simulate_contact_controlled(st.ws.handle, st.batch if B is None else B, ptr(q), ptr(v), ptr(s), None if ctl is None else ctypes.byref(ctl),
                                                           ptr(fext), ctypes.c_double(dt), nsteps, ctypes.byref(st._opts()))


def run_case(rbd, w, case, layout="aos", dtype=torch.float64, fext=True, state=None):
    """One call on a case of simulate_contact_controlled_ref (pd, pd_null, table_per_stage, table_per_step, constant): the final (q, v, s), fp64 numpy (B, n)."""
    C = rbd._capi
    st = state or rbd.MechanismState(w["flat"], w["B"], dtype=dtype, layout=layout)
    D = lambda x: dev(x, layout, dtype)
    q, v, s, fe = D(w["q"]), D(w["v"]), D(w["s"]), D(w["fext"]) if fext else None
    gains = lambda: dict(kp=torch.as_tensor(w["kp"], dtype=dtype).cuda(), kd=torch.as_tensor(w["kd"], dtype=dtype).cuda())
    if case == "pd":
        ctl = control(rbd, C.CONTROL_PD, tau=D(w["tau"]), q_des=D(w["q_des"]), **gains())
    elif case == "pd_null":
        ctl = control(rbd, C.CONTROL_PD, **gains())
    elif case == "constant":
        ctl = control(rbd, C.CONTROL_CONSTANT, tau=D(w["tau"]))
    else:
        per = case == "table_per_stage"
        ctl = control(rbd, C.CONTROL_TABLE, tau=D(w["table"] if per else w["table"][:w["nsteps"]]), per_stage=int(per))
    assert simulate(rbd, st, q, v, s, ctl, fe, w["nsteps"]) == 0
    assert rbd.sync(st) == 0
    k = rbd.last_kernel(st)
    assert "contact_head_kernel" in k and "contact_sim_kernel" in k, k
    return host(q, layout), host(v, layout), host(s, layout)


def simulate_contact(rbd, w, dtype=torch.float64, fext=True, layout="aos"):
    """rbd_simulate_contact (constant τ = the feed-forward) on the same inputs"""
    st = rbd.MechanismState(w["flat"], w["B"], dtype=dtype, layout=layout)
    D = lambda x: dev(x, layout, dtype)
    q, v, s, tau, fe = D(w["q"]), D(w["v"]), D(w["s"]), D(w["tau"]), D(w["fext"]) if fext else None
    stt = rbd._capi.lib().rbd_simulate_contact(st.ws.handle, w["B"], ptr(q), ptr(v), ptr(s), ptr(tau), ptr(fe), ctypes.c_double(DT), w["nsteps"],
                                              ctypes.byref(st._opts()))
    assert stt == 0 and rbd.sync(st) == 0
    k = rbd.last_kernel(st)
    assert "contact_head_kernel" in k and "contact_sim_kernel" in k, k
    return host(q, layout), host(v, layout), host(s, layout)


def close(got, want, tol, what):
    """final (q, v, s) triples: quaternion up to sign, each within tol·(1 + max|want|); figures printed before they are asserted"""
    worst = 0.0
    for name, g, r in zip("qvs", got, want):
        if name == "q":
            g, r = ref.canon(g), ref.canon(r)
        err, bound = np.abs(g - r).max(), tol * (1 + np.abs(r).max())
        print("%-28s %s max|err| %.3e  max|ref| %.3e  bound %.3e" % (what, name, err, np.abs(r).max(), bound))
        assert np.isfinite(g).all(), (what, name)
        worst = max(worst, err / bound)
    assert worst <= 1.0, (what, worst)


@pytest.fixture(scope="module")
def parent():
    """What the commit before the fold computed on the walker's inputs, every `every`-th state (tests/golden/make_simulate_contact_parent.py)."""
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vectors", "simulate_contact_parent.npz")))


def recorded(parent, w, name, keys="qvs"):
    """The recorded arrays `name`_{keys} as fp64 — after the assertion that they were recorded on the inputs of `w`: a SHA-256 over the bytes of q, v, s, tau, fext."""
    h = hashlib.sha256()
    for k in ("q", "v", "s", "tau", "fext"):
        h.update(np.ascontiguousarray(w[k], dtype=np.float64).tobytes())
    assert h.hexdigest() == str(parent["input_hash"]), "walker_case no longer builds the inputs simulate_contact_parent.npz was recorded on"
    return tuple(parent["%s_%s" % (name, k)].astype(np.float64) for k in keys)


def thin(parent, got):
    """the recorded states of full-batch results"""
    return tuple(g[::int(parent["every"])] for g in got)


@pytest.fixture(scope="module")
def walker(rbd, oracle):
    """The walker, B = 130, 3 steps: the inputs and, per controller case, the reference's final state (computed once on first use, shared, left unchanged)."""
    w = ref.walker_case(rbd)
    cache = {}

    def reference(case):
        if case not in cache:
            ctl = ref.constant_control(w["tau"]) if case == "constant" else ref.walker_control(w, case)
            cache[case] = ref.rollout(oracle, w["flat"], w["q"], w["v"], w["s"], ctl, w["fext"], w["nsteps"])[:3]
        return cache[case]
    return dict(w, reference=reference)


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("case", ref.WALKER_CASES)
def test_walker_against_the_numpy_step(rbd, walker, case, layout):
    """Walker (QuaternionFloating + Revolute, Revolute, Prismatic, Revolute; 4 points × 2 half-spaces), B = 130, 3 steps, dt = 1e-3, fp64, fext given: PD with
    feed-forward and q_des, PD with both NULL, a table with a distinct entry per stage, a table per step — final q (quaternion up to sign), v, s within
    1e-10·(1 + max|ref|) of the numpy step with the controller evaluated at every stage state."""
    close(run_case(rbd, walker, case, layout), walker["reference"](case), 1e-10, f"{case} {layout}")


def test_atlas_with_pd_on_every_joint(rbd, oracle, models):
    """Atlas floating with its eight foot points, B = 65, 2 steps, PD on all 30 1-dof joints, fp64: a 31-body level structure with multi-child bodies."""
    a = ref.atlas_case(rbd, oracle, models["atlas_floating"])
    want = ref.rollout(oracle, a["flat"], a["q"], a["v"], a["s"], ref.pd_control(a["flat"], a["kp"], a["kd"], a["q_des"], a["tau"]), a["fext"], a["nsteps"])[:3]
    close(run_case(rbd, a, "pd"), want, 1e-10, "atlas pd")


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_constant_kind_is_simulate_contact(rbd, oracle, walker, parent, layout):
    """CONSTANT and rbd_simulate_contact are one code path: equal bit for bit in fp64 and fp32 (the wrapper's forwarding of tau and fext).  Both against what
    rbd_simulate_contact computed before the fold, on its stage of contact_stage_kernel + rnea_kernel + contact_kernel (recorded, AOS, every second state): fp64
    within 1e-12·(1 + max), fp32 within 16·2⁻²³·(1 + max) (the head kernel's sweep orders the same arithmetic differently from rnea_kernel's).  And fp64 within
    1e-10·(1 + max) of the numpy step with the constant controller, the reference of the four controller cases."""
    for dtype, name, tol in ((torch.float64, "f64", 1e-12), (torch.float32, "f32", 16 * 2.0 ** -23)):
        got = run_case(rbd, walker, "constant", layout, dtype)
        plain = simulate_contact(rbd, walker, dtype, layout=layout)
        for k, g, r in zip("qvs", got, plain):
            assert np.array_equal(g, r), (name, k)
        want = recorded(parent, walker, "sim_" + name)
        if name == "f64":
            print("constant f64 %s bit-identical to the recording: %s" % (layout, all(np.array_equal(g, r) for g, r in zip(thin(parent, got), want))))
        close(thin(parent, got), want, tol, f"constant {name} {layout} vs recording")
        close(thin(parent, plain), want, tol, f"simulate_contact {name} {layout} vs recording")
        if name == "f64":
            close(got, walker["reference"]("constant"), 1e-10, f"constant f64 {layout} vs numpy")


def test_fp32_with_pd(rbd, oracle, walker, parent):
    """fp32, PD with feed-forward and q_des (no external wrenches: simulate_np.simulate_contact takes none), error against the fp64 numpy step.  The yardstick:
    the error rbd_simulate_contact showed in fp32 BEFORE the fold (the recorded run without fext, on the recorded states — not the code under test) against
    simulate_np.simulate_contact on the same inputs with the feed-forward as constant τ.  The bound is 4 × that (the trajectories differ).  Errors: max over
    q, v, s of max|err| / (1 + max|ref|)."""
    import simulate_np as snp
    w = walker
    err = lambda got, want: max(np.abs((ref.canon(g) if n == "q" else g) - (ref.canon(r) if n == "q" else r)).max() / (1 + np.abs(r).max())
                                for n, g, r in zip("qvs", got, want))
    want_c = snp.simulate_contact(w["flat"], w["q"], w["v"], w["s"], (w["nsteps"] - 0.5) * DT, DT, w["tau"])[1:]
    yard = err(recorded(parent, w, "sim_f32_nofext"), thin(parent, want_c))
    want_pd = ref.rollout(oracle, w["flat"], w["q"], w["v"], w["s"], ref.walker_control(w, "pd"), None, w["nsteps"])[:3]
    got = run_case(rbd, w, "pd", dtype=torch.float32, fext=False)
    ours = err(got, want_pd)
    print("fp32 PD error %.3e  yardstick (rbd_simulate_contact fp32 before the fold, recorded) %.3e  ratio %.2f" % (ours, yard, ours / yard))
    assert all(np.isfinite(g).all() for g in got)
    assert ours <= 4 * yard


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_dynamics_contact_on_the_head_kernels_export(rbd, oracle, walker, parent, layout):
    """rbd_dynamics_contact reads contact_head_kernel's export since the fold (run_contact_kinematics; rnea_kernel's before): v̇ and ṡ on the walker's inputs,
    B = 130 (the head kernel's grid ends in a ragged block), against what the commit before computed — fp64 within 1e-12·(1 + max), fp32 within
    16·2⁻²³·(1 + max) — and the pairs reset to s == 0 exactly those of oracle.dynamics_contact."""
    w = walker
    reset = oracle.dynamics_contact(w["flat"], w["q"], w["v"], w["s"].copy(), w["tau"], w["fext"])[1] == 0
    assert reset.any() and not reset.all()
    for dtype, name, tol in ((torch.float64, "f64", 1e-12), (torch.float32, "f32", 16 * 2.0 ** -23)):
        want = recorded(parent, w, "dyn_" + name, ("vdot", "sdot"))
        st = rbd.MechanismState(w["flat"], w["B"], dtype=dtype, layout=layout)
        q, v, s, tau, fe = (dev(w[k], layout, dtype) for k in ("q", "v", "s", "tau", "fext"))
        vd, sd = torch.empty_like(v), torch.empty_like(s)
        assert rbd._capi.lib().rbd_dynamics_contact(st.ws.handle, w["B"], ptr(q), ptr(v), ptr(s), ptr(tau), ptr(fe), ptr(vd), None, ptr(sd), None, None,
                                                    ctypes.byref(st._opts())) == 0
        assert rbd.sync(st) == 0
        for what, g, r in zip(("vdot", "sdot"), thin(parent, (host(vd, layout), host(sd, layout))), want):
            e, bound = np.abs(g - r).max(), tol * (1 + np.abs(r).max())
            print("dynamics_contact %s %s %-4s max|err| %.3e  max|ref| %.3e  bound %.3e" % (name, layout, what, e, np.abs(r).max(), bound))
            assert np.isfinite(g).all() and e <= bound, (name, what)
        assert np.array_equal(host(s, layout) == 0, reset), name


def test_one_call_of_three_steps_is_three_calls_of_one(rbd, walker):
    """A per-stage table: one 3-step call equals three 1-step calls with the table pointer advanced by 4 entries per call, at 1e-13·(1 + max)."""
    w = walker
    one = run_case(rbd, w, "table_per_stage")
    st = rbd.MechanismState(w["flat"], w["B"])
    q, v, s, fe, table = (dev(w[k]) for k in ("q", "v", "s", "fext", "table"))
    for k in range(3):
        ctl = control(rbd, rbd._capi.CONTROL_TABLE, tau=table[4 * k:], per_stage=1)
        assert simulate(rbd, st, q, v, s, ctl, fe, 1) == 0
    assert rbd.sync(st) == 0
    close((host(q), host(v), host(s)), one, 1e-13, "3 x 1 step")


def test_ball_has_no_coordinate_for_the_pd_law(rbd):
    """The ball of test_contact.py (one floating body, no 1-dof joint), B = 9, 20 steps: PD with non-zero gains equals rbd_simulate_contact with
    tau = the feed-forward at 1e-12·(1 + max)."""
    from test_contact import ball
    mech, com, _ = ball(rbd, np.random.default_rng(61))
    flat = rbd.flatten(mech)
    B = 9
    rng = np.random.default_rng(62)
    q = np.tile(np.array([1.0, 0, 0, 0, 1.0, 2.0, 0.0]), (B, 1))
    q[:, 6] = np.linspace(-0.004, 0.006, B) - com[2]  # some balls start in the floor, some reach it, some do not
    w = dict(flat=flat, B=B, nsteps=20, q=q, v=0.1 * rng.standard_normal((B, 6)), s=1e-4 * rng.standard_normal((B, 3)), tau=rng.standard_normal((B, 6)),
             fext=None, kp=1 + rng.random(6), kd=1 + rng.random(6), q_des=rng.standard_normal((B, 7)))
    got = run_case(rbd, w, "pd", fext=False)
    want = simulate_contact(rbd, w, fext=False)
    touched = (want[2] != w["s"]).any(axis=1)  # (a ball that stays clear of the floor at every stage keeps its s: ṡ = 0 there)
    assert touched.any() and not touched.all()
    close(got, want, 1e-12, "ball")


def test_python_callback_path(rbd, walker):
    """simulate_ on the walker with a callback that writes the PD law in torch (B = 7, 2 steps) equals the device-side PD at 1e-11·(1 + max); store=True
    returns nsteps + 1 snapshots of q, v, s, the last one the final state."""
    w = {k: (x[:7] if isinstance(x, np.ndarray) and x.ndim == 2 else x) for k, x in walker.items()}
    w.update(B=7, nsteps=2, table=None)
    flat = w["flat"]
    want = run_case(rbd, w, "pd")
    qi = ref.one_dof(flat)
    on = torch.as_tensor(qi >= 0).cuda()
    qsel = torch.as_tensor(qi[qi >= 0]).cuda()
    kp, kd, qd, tff = (dev(w[k]) for k in ("kp", "kd", "q_des", "tau"))
    times = []

    def callback(tau, t, state):
        times.append(t)
        tau.copy_(tff)
        tau[:, on] -= kp[on] * (state.q[:, qsel] - qd[:, qsel]) + kd[on] * state.v[:, on]
    fe = dev(w["fext"])
    for store in (False, True):
        st = rbd.MechanismState(flat, 7)
        rbd.set_configuration_(st, w["q"]); rbd.set_velocity_(st, w["v"])
        st.s.copy_(dev(w["s"]))
        del times[:]
        out = rbd.simulate_(st, 1.5 * DT, control_=callback, dt=DT, externalwrenches=fe, store=store)
        assert rbd.sync(st) == 0
        assert np.allclose(times, [0, DT / 2, DT / 2, DT, DT, 1.5 * DT, 1.5 * DT, 2 * DT], rtol=0, atol=1e-15)
        close((host(st.q), host(st.v), host(st.s)), want, 1e-11, "callback" + (" store" if store else ""))
        if store:
            ts, qs, vs, ss = out
            assert len(ts) == len(qs) == len(vs) == len(ss) == 3
            assert torch.equal(qs[0], dev(w["q"])) and torch.equal(ss[0], dev(w["s"]))
            assert torch.equal(qs[-1], st.q) and torch.equal(vs[-1], st.v) and torch.equal(ss[-1], st.s)
            assert not torch.equal(qs[1], qs[0]) and not torch.equal(qs[2], qs[1])
        else:
            assert len(out) == 3
    # the device controllers through simulate_: the same call as the C entry point's; store=True stays unbuilt
    st = rbd.MechanismState(flat, 7)
    rbd.set_configuration_(st, w["q"]); rbd.set_velocity_(st, w["v"])
    st.s.copy_(dev(w["s"]))
    pd = rbd.PDControl(torch.as_tensor(w["kp"]), torch.as_tensor(w["kd"]), qd, tff)
    with pytest.raises(NotImplementedError):
        rbd.simulate_(st, 1.5 * DT, control_=pd, dt=DT, externalwrenches=fe, store=True)
    rbd.simulate_(st, 1.5 * DT, control_=pd, dt=DT, externalwrenches=fe)
    assert rbd.sync(st) == 0
    for g, r in zip((host(st.q), host(st.v), host(st.s)), want):
        assert np.array_equal(g, r)


def test_argument_checks_and_no_ops(rbd, models, walker):
    C = rbd._capi
    w = walker
    flat, B = w["flat"], w["B"]
    st = rbd.MechanismState(flat, B)
    q, v, s, tau, fe, table = (dev(w[k]) for k in ("q", "v", "s", "tau", "fext", "table"))
    kp, kd = torch.as_tensor(w["kp"]).cuda(), torch.as_tensor(w["kd"]).cuda()
    keep = [x.clone() for x in (q, v, s)]
    same = lambda: all(torch.equal(a, b) for a, b in zip(keep, (q, v, s)))
    const = control(rbd, C.CONTROL_CONSTANT, tau=tau)
    INVALID, UNSUPPORTED = 1, 3
    assert simulate(rbd, st, q, v, s, None, fe, 1) == INVALID  # NULL control
    assert simulate(rbd, st, q, v, s, control(rbd, C.CONTROL_TABLE, per_stage=1), fe, 1) == INVALID  # TABLE without tau
    assert simulate(rbd, st, q, v, s, control(rbd, C.CONTROL_PD, tau=tau, kp=kp), fe, 1) == INVALID  # PD without kd
    assert simulate(rbd, st, q, v, s, control(rbd, C.CONTROL_PD, tau=tau, kd=kd), fe, 1) == INVALID  # PD without kp
    assert simulate(rbd, st, q, v, s, control(rbd, 3, tau=tau), fe, 1) == INVALID  # kind out of range
    assert simulate(rbd, st, q, v, s, control(rbd, -1, tau=tau), fe, 1) == INVALID
    assert simulate(rbd, st, q, v, s, const, fe, 1, dt=0.0) == INVALID
    assert simulate(rbd, st, q, v, s, const, fe, -1) == INVALID
    for miss in range(3):
        args = [q, v, s]
        args[miss] = None
        assert simulate(rbd, st, *args, const, fe, 1) == INVALID
    # a model without contact points (rbd_simulate_controlled's); host memory
    dp = rbd.MechanismState(models["double_pendulum"], 4)
    z4 = torch.zeros(4, 8, dtype=torch.float64, device="cuda")
    assert simulate(rbd, dp, dp.q, dp.v, z4, control(rbd, C.CONTROL_CONSTANT), None, 1) == INVALID
    o = st._opts()
    ho = C.Opts(o.layout, C.MEM_HOST, o.algorithm, o.stabilization)
    assert C.lib().rbd_simulate_contact_controlled(st.ws.handle, B, ptr(q), ptr(v), ptr(s), ctypes.byref(const), ptr(fe), ctypes.c_double(DT), 1,
                                                   ctypes.byref(ho)) == UNSUPPORTED
    assert rbd.sync(st) == 0 and same()
    # B == 0 and nsteps == 0: successful no-ops
    assert simulate(rbd, st, q, v, s, const, fe, 3, B=0) == 0
    assert simulate(rbd, st, q, v, s, const, fe, 0) == 0
    assert rbd.sync(st) == 0 and same()
    # the entry point without the additional state keeps refusing the model
    assert C.lib().rbd_simulate_controlled(st.ws.handle, B, ptr(q), ptr(v), ctypes.byref(const), ptr(fe), ctypes.c_double(DT), 1, ctypes.byref(o)) == UNSUPPORTED
    # only the first call (or a larger B) allocates
    pdc = control(rbd, C.CONTROL_PD, tau=tau, kp=kp, kd=kd)
    assert simulate(rbd, st, q, v, s, pdc, fe, 2) == 0
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    assert simulate(rbd, st, q, v, s, pdc, fe, 2) == 0
    assert simulate(rbd, st, q, v, s, control(rbd, C.CONTROL_TABLE, tau=table, per_stage=1), None, 3) == 0
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    assert rbd.sync(st) == 0 and not same()
