"""`simulate(state, T, control!)` of a mechanism with contact points in numpy — the reference of the rbd_simulate_contact_controlled tests (not a test itself).

The Munthe-Kaas RK4 step of oracle/simulate_np.py (global_coordinates, local_rate, RK4_A / RK4_B / RK4_C) around oracle.dynamics_contact for (v̇, ṡ), with the
controller control(b, t, q_b, v_b) -> τ_b evaluated at each stage state before that stage's dynamics, as the reference's closure calls control!(τ, t, state)
(src/simulate.jl:42-48).  s goes through the tableau from the UN-reset s of the step start, like simulate_np.step_contact; the reset acts inside the stage.

Also here, so that the CPU test checks the very inputs the GPU tests run: the walker and Atlas cases (seeds chosen on the CPU so that the branch conditions
test_simulate_contact_controlled_cpu.py asserts hold) and their controllers."""
import copy

import numpy as np

import contact_model_ref as cm

DT = 1e-3
FEET = ("l_foot", "r_foot")  # Atlas' eight foot points of the contact benchmarks: four sole corners per foot, one floor
SOLE = [(x, y, -0.08) for x in (0.17, -0.08) for y in (0.06, -0.06)]


def step(oracle, flat, q0, v0, s0, dt, control, fext=None, t0=0.0):
    """One step for the whole batch; returns q⁺, v⁺, s⁺ and the oracle's pair info of the four stage states."""
    import simulate_np as snp
    B = q0.shape[0]
    phids, vds, sds, infos = [], [], [], []
    for i in range(4):
        q, v, s = q0, v0, s0
        if i:
            a = dt * snp.RK4_A[i, i - 1]
            q = np.stack([snp.global_coordinates(flat, q0[b], a * phids[-1][b]) for b in range(B)])
            v, s = v0 + a * vds[-1], s0 + a * sds[-1]
        tau = np.stack([control(b, t0 + snp.RK4_C[i] * dt, q[b], v[b]) for b in range(B)])
        infos.append(cm.oracle_pair_info(oracle, flat, q, v, s))
        vd, _, sd, _, _ = oracle.dynamics_contact(flat, q, v, s, tau, fext)
        vds.append(vd); sds.append(sd)
        phids.append(np.stack([snp.local_rate(flat, q0[b], q[b], v[b]) for b in range(B)]))
    comb = lambda xs: sum(dt * snp.RK4_B[i] * xs[i] for i in range(4))
    phi = comb(phids)
    return np.stack([snp.global_coordinates(flat, q0[b], phi[b]) for b in range(B)]), v0 + comb(vds), s0 + comb(sds), infos


def rollout(oracle, flat, q, v, s, control, fext, nsteps, dt=DT):
    """nsteps steps from t = 0; the final (q, v, s) and the pair info of every stage of every step (nsteps lists of four)."""
    q, v, s = (np.array(x, float) for x in (q, v, s))
    infos = []
    for k in range(nsteps):
        q, v, s, info = step(oracle, flat, q, v, s, dt, control, fext, k * dt)
        infos.append(info)
    return q, v, s, infos


def one_dof(flat):
    """per velocity coordinate: the configuration coordinate of its Revolute / Prismatic joint, or -1 (the PD law leaves that coordinate's τ alone)"""
    qi = -np.ones(flat.nv, dtype=int)
    for i in range(flat.n_bodies):
        if int(flat.joint_type[i]) in (1, 2):
            qi[int(flat.v_offset[i])] = int(flat.q_offset[i])
    return qi


def pd_control(flat, kp, kd, q_des, tau):
    """RBD_CONTROL_PD as a callback: τ_i = tau_i − kp_i (q_i − q_des_i) − kd_i v_i on the 1-dof joints, tau elsewhere (q_des, tau None = 0)."""
    qi = one_dof(flat)
    on = qi >= 0

    def control(b, t, q, v):
        out = np.zeros(flat.nv) if tau is None else tau[b].copy()
        qd = 0.0 if q_des is None else q_des[b][qi[on]]
        out[on] -= kp[on] * (q[qi[on]] - qd) + kd[on] * v[on]
        return out
    return control


def table_control(table, per_stage, dt=DT):
    """RBD_CONTROL_TABLE as a callback: entry 4·step + stage at the stage times t, t + h/2, t + h/2, t + h — the two middle stages share a time, so the
    stage comes from a count of the calls per state —, or entry `step`."""
    calls = {}

    def control(b, t, q, v):
        k = calls.get(b, 0)
        calls[b] = k + 1
        return table[k if per_stage else k // 4][b]
    return control


def constant_control(tau):
    return lambda b, t, q, v: tau[b]


def walker_case(rbd, B=130, seed=5):
    """The walker of contact_model_ref (QuaternionFloating + Revolute, Revolute, Prismatic, Revolute; 4 points × 2 half-spaces, ns = 24) with the states of
    test_simulate_contact_vjp_gpu.py's walker130, external wrenches, and the data of the four controller cases."""
    rng = np.random.default_rng(seed)
    flat = rbd.flatten(cm.walker(rbd, rng))
    q, v, s = cm.walker_states(rbd, flat, B, rng)
    tau, fext = rng.random((B, flat.nv)), rng.random((B, 6 * flat.n_bodies))
    kp, kd = 20 * rng.random(flat.nv), 2 * rng.random(flat.nv)
    q_des = 0.3 * rng.standard_normal((B, flat.nq))
    table = rng.standard_normal((12, B, flat.nv))  # 3 steps × 4 stages, a distinct entry each
    return dict(flat=flat, B=B, nsteps=3, q=q, v=v, s=s, tau=tau, fext=fext, kp=kp, kd=kd, q_des=q_des, table=table)


WALKER_CASES = ("pd", "pd_null", "table_per_stage", "table_per_step")


def walker_control(w, case):
    """the numpy callback of one of WALKER_CASES"""
    if case == "pd":
        return pd_control(w["flat"], w["kp"], w["kd"], w["q_des"], w["tau"])
    if case == "pd_null":
        return pd_control(w["flat"], w["kp"], w["kd"], None, None)
    return table_control(w["table"], case == "table_per_stage")


def with_contact(flat, points, halfspaces):
    """A copy of a flat model with contact points (dicts as FlatModel keeps them) and half-spaces."""
    m = copy.copy(flat)
    m.contact_points, m.halfspaces = points, halfspaces
    m.ns = 3 * len(points) * len(halfspaces)
    m._c = None
    m.__dict__.pop("_rbd_model", None)  # (the library's model cached on the copied object is the one without contact points)
    return m


def atlas_case(rbd, oracle, bare, B=65, seed=23):
    """Atlas on a floating base with four sole points per foot and one floor; the pelvis height per state puts the lowest sole point between 3 cm under and
    1 cm over the floor (positions from the oracle's kinematics).  PD on every 1-dof joint with the small gains of test_simulate_device_side_controllers (the
    wrist links have 4e-4 kg m² about their axes: stiff gains would need a smaller step)."""
    from point_kinematics_ref import reference
    rng = np.random.default_rng(seed)
    hc = rbd.hunt_crossley_hertz()
    par = dict(hc_k=hc.k, hc_lambda=hc.lam, hc_n=hc.n, mu=0.8, k=20e3, b=100.0)
    pts = [dict(par, body=list(bare.body_names).index(f), location=np.array(r)) for f in FEET for r in SOLE]
    flat = with_contact(bare, pts, [dict(point=np.zeros(3), outward_normal=np.array([0.0, 0.0, 1.0]))])
    q, v = rbd.rand_configuration(bare, B, rng), rbd.rand_velocity(bare, B, rng)
    q[:, 4:7] = 0
    pos = reference(oracle, bare, q, v, None, [c["body"] for c in pts], [c["location"] for c in pts], jac=False)[0]
    up = bare.pred_rot[0].T @ np.array([0.0, 0.0, 1.0])
    q[:, 4:7] = (rng.uniform(-0.03, 0.01, B) - pos[:, :, 2].min(axis=1))[:, None] * up
    s = 1e-3 * rng.standard_normal((B, flat.ns))
    tau, fext = rng.random((B, flat.nv)), rng.random((B, 6 * flat.n_bodies))
    kp, kd = 2 * rng.random(flat.nv), 0.02 * rng.random(flat.nv)
    q_des = q + 0.3 * rng.standard_normal((B, flat.nq))
    return dict(flat=flat, B=B, nsteps=2, q=q, v=v, s=s, tau=tau, fext=fext, kp=kp, kd=kd, q_des=q_des)


def stages(infos):
    return [info for step_ in infos for info in step_]


def conditions(infos, rel=1e-6):
    """What the parity tests assume of their inputs, from the pair info of every stage of every step: (every pair clear of the branch boundaries, some pair in
    contact at some stage, some pair not in contact at some stage, some pair changing branch between two stages of the rollout)."""
    import torch
    st = stages(infos)
    margins = all(bool(cm.margins_ok(i, rel).all()) for i in st)
    inside = torch.stack([i["inside"] for i in st])
    br = torch.stack([cm.branch_of(i) for i in st])
    return margins, bool(inside.any()), bool((~inside).any()), bool((br != br[:1]).any())


def canon(q):
    """the floating base's quaternion up to sign (q and −q are the same rotation)"""
    q = q.copy()
    sg = np.sign(q[:, :1])
    sg[sg == 0] = 1
    q[:, :4] *= sg
    return q
