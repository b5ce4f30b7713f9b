"""The Munthe-Kaas RK4 step of `simulate` in torch, differentiable by torch.autograd: the exact reference of the rollout VJP tests (not a test itself).

A batch-first port of oracle/simulate_np.py's local_rate / global_coordinates / step_contact for Fixed / Revolute / Prismatic / QuaternionFloating tree joints;
the dynamics of every stage come from a callable, f(q, v, s) -> (v̇, ṡ, info) (ṡ and info None without contact; info is whatever the caller wants kept per
stage, the pair info of tests/contact_model_ref.py in the contact tests).  Its own pin is the oracle (test_simulate_contact_vjp_cpu.py).

The maps are functions of the RAW coordinates q, as every derivative of the library: the quaternion enters the relative rotation unnormalised and the rotation
matrix by the unnormalised formula.  The small-angle branches of the reference (θ < eps in exp, log_with_time_derivative and the rotation vector of a
quaternion) are removable singularities; a literal autograd pass through them gives 0/0 at θ = 0 and drops the first-order terms exactly where every step
starts (stage 0 has q = q0).  Every coefficient that is singular at θ = 0 is therefore a power series in θ² below a threshold (csrc/rbd_tangent_mk.hpp's:
1e-2 in fp64, 0.5 in fp32) and the closed form above it, the branch not taken evaluated at a safe argument so that torch.where passes no 0 · NaN back.  At
θ <= eps the VALUE of ϕ̇ is the reference's branch (the body twist itself) and the derivative that of the smooth map."""
import torch

FIXED, REVOLUTE, PRISMATIC, FLOATING = 0, 1, 2, 3
RK4_A = (0.5, 0.5, 1.0)  # a_{i+1,i}
RK4_B = (1 / 6, 1 / 3, 1 / 3, 1 / 6)

# Taylor coefficients in t = θ² (x = θ/2, α = x cot x, β = x²/sin²x)
CA = (1 / 12, 1 / 720, 1 / 30240, 1 / 1209600, 1 / 47900160, 691 / 1307674368000)  # (1 − α)/θ²
A_ = (1 / 12, 0.0, -1 / 30240, -1 / 604800, -1 / 15966720, -691 / 326918592000)  # (2(1 − α) + (α − β)/2)/θ²
BC = (-1 / 720, -1 / 15120, -1 / 403200, -1 / 11975040, -691 / 261534873600, -1 / 12454041600)  # ((1 − α) + (α − β)/2)/θ⁴
EA = (1 / 2, -1 / 24, 1 / 720, -1 / 40320, 1 / 3628800, -1 / 479001600)  # (1 − cos θ)/θ²
EB = (1 / 6, -1 / 120, 1 / 5040, -1 / 362880, 1 / 39916800, -1 / 6227020800)  # (θ − sin θ)/θ³
QC = (1.0, -1 / 8, 1 / 384, -1 / 46080, 1 / 10321920, -1 / 3715891200)  # cos(θ/2)
QS = (1 / 2, -1 / 48, 1 / 3840, -1 / 645120, 1 / 185794560, -1 / 81749606400)  # sin(θ/2)/θ
AT = (1.0, -1 / 3, 1 / 5, -1 / 7, 1 / 9, -1 / 11)  # atan(√z)/√z


def series_theta(dtype):
    return 0.5 if dtype == torch.float32 else 1e-2


def _series(t, c):
    r = t * c[5] + c[4]
    for k in (3, 2, 1, 0):
        r = r * t + c[k]
    return r


def _cross(a, b):
    return torch.linalg.cross(a, b, dim=-1)


def qmul(a, b):
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], dim=-1)


def qconj(a):
    return a * torch.tensor([1.0, -1.0, -1.0, -1.0], dtype=a.dtype, device=a.device)


def qrotate(q, x):
    """R(q) x by the unnormalised formula (oracle qrot)."""
    w, a, b, c = q.unbind(-1)
    x0, x1, x2 = x.unbind(-1)
    return torch.stack([(1 - 2 * (b * b + c * c)) * x0 + 2 * (a * b - w * c) * x1 + 2 * (a * c + w * b) * x2,
                        2 * (a * b + w * c) * x0 + (1 - 2 * (a * a + c * c)) * x1 + 2 * (b * c - w * a) * x2,
                        2 * (a * c - w * b) * x0 + 2 * (b * c + w * a) * x1 + (1 - 2 * (a * a + b * b)) * x2], dim=-1)


def rotvec_from_quat(q):
    """θ/|u| · u for the quaternion (w, u), θ = 2 atan2(|u|, w): (2/w) atan(√z)/√z · u with z = |u|²/w² as a series near u = 0."""
    w, u = q[..., 0], q[..., 1:]
    u2 = (u * u).sum(-1)
    lim = series_theta(q.dtype) / 2
    ser = (w > 0) & (u2 < lim * lim * w * w)
    one = torch.ones_like(w)
    ws = torch.where(ser, w, one)
    k_ser = 2 / ws * _series(torch.where(ser, u2, torch.zeros_like(u2)) / (ws * ws), AT)
    closed = ~ser & (u2 > 0)
    sq = torch.sqrt(torch.where(closed, u2, one))
    k_cl = 2 * torch.atan2(sq, torch.where(closed, w, one)) / sq
    k = torch.where(ser, k_ser, torch.where(closed, k_cl, 2 * one))
    return k[..., None] * u


def quat_from_rotvec(r):
    t2 = (r * r).sum(-1)
    lim = series_theta(r.dtype)
    small = t2 < lim * lim
    tser, th = torch.where(small, t2, torch.zeros_like(t2)), torch.sqrt(torch.where(small, torch.ones_like(t2), t2))
    c = torch.where(small, _series(tser, QC), torch.cos(th / 2))
    k = torch.where(small, _series(tser, QS), torch.sin(th / 2) / th)
    return torch.cat([c[..., None], k[..., None] * r], dim=-1)


def se3_comm(x, y):
    return torch.cat([_cross(x[..., :3], y[..., :3]), _cross(x[..., :3], y[..., 3:]) + _cross(x[..., 3:], y[..., :3])], dim=-1)


def floating_local_rate(q0, q, v):
    """log_with_time_derivative of inv(T0) T with the body twist v (spatialmotion.jl:226-304): ϕ̇ (…, 6)."""
    q0c = qconj(q0[..., :4])
    dq = qmul(q0c, q[..., :4])
    dp = qrotate(q0c, q[..., 4:7] - q0[..., 4:7])
    psi = rotvec_from_quat(dq)
    t2 = (psi * psi).sum(-1)
    lim = series_theta(q.dtype)
    small = t2 < lim * lim
    zero, one = torch.zeros_like(t2), torch.ones_like(t2)
    tser, tcl = torch.where(small, t2, zero), torch.where(small, one, t2)
    h = torch.sqrt(tcl) / 2
    s2, c2 = torch.sin(h), torch.cos(h)
    alpha, beta = h * c2 / s2, h * h / (s2 * s2)
    ca = torch.where(small, _series(tser, CA), (1 - alpha) / tcl)
    A = torch.where(small, _series(tser, A_), (2 * (1 - alpha) + 0.5 * (alpha - beta)) / tcl)
    Bc = torch.where(small, _series(tser, BC), ((1 - alpha) + 0.5 * (alpha - beta)) / (tcl * tcl))
    x1 = _cross(psi, dp)
    x2 = _cross(psi, x1)
    X = torch.cat([psi, dp - 0.5 * x1 + ca[..., None] * x2], dim=-1)
    a1 = se3_comm(X, v)
    a2 = se3_comm(X, a1)
    a3 = se3_comm(X, a2)
    a4 = se3_comm(X, a3)
    o = v + 0.5 * a1 + A[..., None] * a2 + Bc[..., None] * a4
    eps = torch.finfo(q.dtype).eps
    tiny = ~(t2 > eps * eps)  # the reference's branch: the body twist itself (the value only)
    return o + torch.where(tiny[..., None], (v - o).detach(), torch.zeros_like(o))


def floating_global(q0, phi):
    """exp(::Twist) (spatialmotion.jl:311-332) applied to q0: the translation is V ν = ν + a ω × ν + b ω × (ω × ν)."""
    pr, pt = phi[..., :3], phi[..., 3:]
    dq = quat_from_rotvec(pr)
    t2 = (pr * pr).sum(-1)
    lim = series_theta(phi.dtype)
    small = t2 < lim * lim
    zero, one = torch.zeros_like(t2), torch.ones_like(t2)
    tser, tcl = torch.where(small, t2, zero), torch.where(small, one, t2)
    th = torch.sqrt(tcl)
    a = torch.where(small, _series(tser, EA), (1 - torch.cos(th)) / tcl)
    b = torch.where(small, _series(tser, EB), (th - torch.sin(th)) / (tcl * th))
    c1 = _cross(pr, pt)
    c2 = _cross(pr, c1)
    tr = pt + a[..., None] * c1 + b[..., None] * c2
    return torch.cat([qmul(q0[..., :4], dq), q0[..., 4:7] + qrotate(q0[..., :4], tr)], dim=-1)


def _joints(flat):
    one_q, one_v, floating = [], [], []
    for i in range(flat.n_bodies):
        t, qo, vo = int(flat.joint_type[i]), int(flat.q_offset[i]), int(flat.v_offset[i])
        if t in (REVOLUTE, PRISMATIC):
            one_q.append(qo); one_v.append(vo)
        elif t == FLOATING:
            floating.append((qo, vo))
        else:
            assert t == FIXED, "simulate_contact_ref: Fixed / Revolute / Prismatic / QuaternionFloating joints only"
    return one_q, one_v, floating


def local_rate(flat, q0, q, v):
    """ϕ̇ of local_coordinates!(ϕ, ϕ̇, state, q0), (B, nv)."""
    _, _, floating = _joints(flat)
    out = v.clone()  # 1-coordinate joints: ϕ̇ = v
    for qo, vo in floating:
        out[:, vo:vo + 6] = floating_local_rate(q0[:, qo:qo + 7], q[:, qo:qo + 7], v[:, vo:vo + 6])
    return out


def global_coordinates(flat, q0, phi):
    one_q, one_v, floating = _joints(flat)
    q = torch.zeros_like(q0)
    if one_q:
        q[:, one_q] = q0[:, one_q] + phi[:, one_v]
    for qo, vo in floating:
        q[:, qo:qo + 7] = floating_global(q0[:, qo:qo + 7], phi[:, vo:vo + 6])
    return q


def step(flat, q0, v0, s0, dt, f):
    """One MuntheKaasIntegrator step with the RK4 tableau (ode_integrators.jl:233-299), s through the tableau like v (s0 None: no additional state).  Stage
    0 is evaluated AT (q0, v0, s0) itself.  Returns q⁺, v⁺, s⁺ and the list of the four stages' info."""
    phids, vds, sds, infos = [], [], [], []
    for i in range(4):
        if i == 0:
            q, v, s = q0, v0, s0
        else:
            a = dt * RK4_A[i - 1]
            q = global_coordinates(flat, q0, a * phids[-1])
            v = v0 + a * vds[-1]
            s = None if s0 is None else s0 + a * sds[-1]
        vd, sd, info = f(q, v, s)
        vds.append(vd); sds.append(sd); infos.append(info)
        phids.append(local_rate(flat, q0, q, v))
    comb = lambda xs: sum(dt * RK4_B[i] * xs[i] for i in range(4))
    return global_coordinates(flat, q0, comb(phids)), v0 + comb(vds), None if s0 is None else s0 + comb(sds), infos


def rollout(flat, q, v, s, dt, nsteps, f):
    """nsteps steps; returns the final (q, v, s) and the info of every stage of every step (nsteps lists of four)."""
    infos = []
    for _ in range(nsteps):
        q, v, s, info = step(flat, q, v, s, dt, f)
        infos.append(info)
    return q, v, s, infos
