"""The soft contact model of one (contact point, half-space) pair in torch fp64 — the reference's default models (src/contact.jl: Hunt–Crossley normal force,
viscoelastic Coulomb friction, half-spaces) with the branches of csrc/rbd_contact.hpp —, differentiable by torch.autograd: the exact reference of the contact
VJP tests.  Its own pin is the oracle (test_contact_vjp_cpu.py::test_torch_model_against_the_oracle).

Two choices keep autograd finite where the model is: the slip scale is μ fn / ‖f_s⁰‖ (sqrt(m2 / n2) has an infinite derivative at fn = 0, and differs from it
by rounding only), and the values a branch does not take are replaced by safe ones before pow and sqrt (torch.where passes 0 · NaN = NaN back otherwise)."""
import numpy as np
import torch

PARAMS = ("hc_k", "hc_lambda", "hc_n", "mu", "k", "b")
BRANCHES = ("outside", "clamped", "stick", "slip")


def pair_model(pos, vel, x, par, h, n):
    """pos, vel, x: (..., 3); par: (..., 6) in the order of PARAMS; h, n: (..., 3) the half-space's point and unit outward normal (all broadcast).
    Returns f, xd, x_out (..., 3) and `info`: inside / pushing / slip masks and the quantities the branch margins are stated in."""
    hck, hcl, hcn, mu, k, b = (par[..., i:i + 1] for i in range(6))
    sep = ((pos - h) * n).sum(-1, keepdim=True)
    inside = sep <= 0
    z = torch.where(inside, -sep, torch.ones_like(sep))
    zd = -(vel * n).sum(-1, keepdim=True)
    zn = z ** hcn
    fr = hcl * zn * zd + hck * zn
    pushing = fr > 0
    fn = torch.where(pushing, fr, torch.zeros_like(fr))
    f0 = -k * x - b * (vel + zd * n)
    n2 = (f0 * f0).sum(-1, keepdim=True)
    m2 = (mu * fn) ** 2
    slip = n2 > m2
    sc = torch.where(slip, mu * fn / torch.sqrt(torch.where(slip, n2, torch.ones_like(n2))), torch.ones_like(n2))
    fs = f0 * sc
    zero = torch.zeros_like(fs)
    f = torch.where(inside, fn * n + fs, zero)
    xd = torch.where(inside, (-k * x - fs) / b, zero)
    x_out = torch.where(inside, x + zero, zero)
    info = dict(inside=inside[..., 0], pushing=pushing[..., 0], slip=slip[..., 0], sep=sep[..., 0], fr=fr[..., 0], kzn=(hck * zn)[..., 0], n2=n2[..., 0], m2=m2[..., 0])
    return f, xd, x_out, info


def branch_of(info):
    """0 outside, 1 clamped (inside, fn ≤ 0), 2 sticking, 3 slipping — per pair."""
    inside, pushing, slip = info["inside"], info["pushing"], info["slip"]
    return torch.where(~inside, 0, torch.where(~pushing, 1, torch.where(slip, 3, 2)))


def margins_ok(info, rel=1e-6):
    """The conditions on the inputs under which the branch is stable: |sep| ≥ rel, and for inside pairs |fn| ≥ rel·k zⁿ and |n2 − m2| ≥ rel·max(n2, m2)."""
    inside = info["inside"]
    ok = info["sep"].abs() >= rel
    ok &= ~inside | (info["fr"].abs() >= rel * info["kzn"])
    ok &= ~inside | ((info["n2"] - info["m2"]).abs() >= rel * torch.maximum(info["n2"], info["m2"]))
    return ok


def coverage(info):
    """The fraction of the pairs on each of the four branches."""
    br = branch_of(info).reshape(-1)
    return [float((br == i).double().mean()) for i in range(4)]


def tables(flat, dtype=torch.float64, device="cpu"):
    """The model's contact tables as tensors: body (P,) long, loc (P, 3), par (P, 6), h and n (H, 3), the normals normalised as the library does."""
    cps = flat.contact_points
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=dtype, device=device)
    body = torch.as_tensor([c["body"] for c in cps], dtype=torch.long, device=device)
    loc = t([c["location"] for c in cps])
    par = t([[c[name] for name in ("hc_k", "hc_lambda", "hc_n", "mu", "k", "b")] for c in cps])
    nrm = np.asarray([hs["outward_normal"] for hs in flat.halfspaces], dtype=np.float64)
    nrm = nrm / np.sqrt((nrm * nrm).sum(axis=1, keepdims=True))
    return body, loc, par, t([hs["point"] for hs in flat.halfspaces]), t(nrm)


def contact_model(flat, pos, vel, s, tab=None):
    """contact_dynamics! from the contact points' positions and velocities in the root frame: pos, vel (B, 3P), s (B, ns), batch first.
    Returns contactwrenches (B, 6·n_bodies), ṡ (B, ns), s after the resets (B, ns) and the pair info ((B, P, H) each)."""
    body, loc, par, h, n = tab if tab is not None else tables(flat, pos.dtype, pos.device)
    B, P, H = pos.shape[0], body.shape[0], h.shape[0]
    p3, v3 = pos.reshape(B, P, 1, 3), vel.reshape(B, P, 1, 3)
    f, xd, x_out, info = pair_model(p3, v3, s.reshape(B, P, H, 3), par.reshape(1, P, 1, 6), h.reshape(1, 1, H, 3), n.reshape(1, 1, H, 3))
    fsum = f.sum(dim=2)  # (B, P, 3)
    w = torch.cat([torch.linalg.cross(pos.reshape(B, P, 3), fsum), fsum], dim=-1)  # Wrench(point, force): (pos × f; f)
    cw = torch.zeros(B, flat.n_bodies, 6, dtype=pos.dtype, device=pos.device).index_add(1, body, w)
    return cw.reshape(B, -1), xd.reshape(B, -1), x_out.reshape(B, -1), info


def walker(rbd, rng, bare=False):
    """The walker of test_contact.py — a small floating tree with contact points on several bodies (two on one of them) and two half-spaces — and, with
    `bare`, the same mechanism from the same random draws without its contact points and environment."""
    mech = rbd.rand_tree_mechanism(rng, ["QuaternionFloating", "Revolute", "Revolute", "Prismatic", "Revolute"])
    bodies = mech.bodies[1:]
    for b, npts in zip((bodies[0], bodies[2], bodies[4]), (1, 2, 1)):
        for _ in range(npts):
            model = rbd.SoftContactModel(rbd.hunt_crossley_hertz(k=2e3 * (1 + rng.random()), alpha=0.3 * rng.random()),
                                         rbd.ViscoelasticCoulombModel(0.3 + rng.random(), 1e3 * (1 + rng.random()), 1e2 * (1 + rng.random())))
            rbd.add_contact_point_(b, rbd.ContactPoint(0.3 * rng.standard_normal(3), model))
    rbd.add_environment_primitive_(mech, rbd.HalfSpace3D([0, 0, 0.2], [0.1, -0.2, 1.0]))
    rbd.add_environment_primitive_(mech, rbd.HalfSpace3D([0.3, 0, 0], [1.0, 0.3, 0.1]))
    return strip_contact(mech) if bare else mech


def strip_contact(mech):
    for b in mech.bodies:
        b.contact_points = []
    mech.environment = []
    return mech


def walker_states(rbd, flat, B, rng, vscales=(1.0, 10.0, 30.0), sscale=1e-3):
    """Random states of the walker near its two half-spaces — the states of test_contact.py with the velocity of each state rescaled by one of `vscales`
    (the Hunt–Crossley force clamps only where a point leaves faster than k / λ, several m/s here) and the friction state by `sscale`."""
    q, v = rbd.rand_configuration(flat, B, rng), rbd.rand_velocity(flat, B, rng)
    v *= rng.choice(np.asarray(vscales), B)[:, None]
    q[:, 4:7] *= 0.5
    s = sscale * rng.standard_normal((B, flat.ns))
    return q, v, s


def oracle_pair_info(oracle, flat, q, v, s):
    """The pair info of contact_model at the contact points' positions and velocities formed from the oracle's per-body kinematics (CPU)."""
    from point_kinematics_ref import reference
    B = q.shape[0]
    pos, vel, _, _ = reference(oracle, flat, q, v, None, [c["body"] for c in flat.contact_points], [c["location"] for c in flat.contact_points], jac=False)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)
    return contact_model(flat, T(pos.reshape(B, -1)), T(vel.reshape(B, -1)), T(s))[3]
