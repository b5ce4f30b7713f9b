"""The form of the articulated-body recursion that the banked kernels run (csrc/rbd_bank.hpp, RBD_BANK_BIAS_SWEEP) against the textbook form, in
numpy, on random trees, everything expressed in the root frame as the kernels have it.

Textbook (Featherstone): c_i = [T_i, vJ_i];  bottom-up  Ia = IA - U U'/D,  pa = pA + Ia c + U u/D;  top-down  a' = a_parent + c,  v̇ = (u - U'a')/D,  a = a' + S v̇.
Kernel: the bias accelerations are summed on the way down, z_i = z_parent + [T_parent, T_i] (= z_parent + c_i, since T_i = T_parent + vJ_i), the body's own
I_i z_i joins its bias force, and the recursion runs with c = 0 on a' = a - z:  pa = pA + U u/D,  v̇ = (u - U'a'_parent)/D,  a' = a'_parent + S v̇.
The joint accelerations v̇ of the two agree to rounding: max |Δv̇| <= 1e-12 max |v̇| per tree (observed: 5e-15 over 200 trees of up to 31 bodies).
Fixed joints are S = 0 with 1/D = 0, as the kernels carry them."""
import numpy as np


def crm(x):
    """spatial cross product matrix of a motion vector (angular; linear): crm(x) y = [x, y], the se(3) commutator"""
    w, v = x[:3], x[3:]
    sk = lambda a: np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    m = np.zeros((6, 6))
    m[:3, :3] = sk(w)
    m[3:, :3] = sk(v)
    m[3:, 3:] = sk(w)
    return m


def random_tree(rng, n):
    """parents (-1: the world, body 0 alone), motion subspaces (a zero column: fixed joint), rigid inertias about a point away from the body, all in one frame"""
    parent = np.array([-1] + [int(rng.integers(max(0, i - 4), i)) for i in range(1, n)])
    S = np.zeros((n, 6))
    I = np.zeros((n, 6, 6))
    for i in range(n):
        kind = rng.choice(["revolute", "prismatic", "fixed"], p=[0.7, 0.15, 0.15])
        a = rng.standard_normal(3)
        a /= np.linalg.norm(a)
        r = rng.standard_normal(3)
        if kind == "revolute":
            S[i] = np.concatenate([a, np.cross(r, a)])
        elif kind == "prismatic":
            S[i] = np.concatenate([np.zeros(3), a])
        m = rng.uniform(0.5, 2.0)
        c = rng.standard_normal(3)  # centre of mass, from the frame's origin
        A = rng.standard_normal((3, 3))
        Jc = A @ A.T * 0.05 + 0.02 * np.eye(3)
        cx = crm(np.concatenate([c, np.zeros(3)]))[:3, :3]
        I[i, :3, :3] = Jc + m * cx @ cx.T
        I[i, :3, 3:] = m * cx
        I[i, 3:, :3] = m * cx.T
        I[i, 3:, 3:] = m * np.eye(3)
    return parent, S, I


def kinematics(parent, S, v):
    n = len(parent)
    Tw, vJ = np.zeros((n, 6)), np.zeros((n, 6))
    for i in range(n):
        vJ[i] = S[i] * v[i]
        Tw[i] = (Tw[parent[i]] if parent[i] >= 0 else 0.0) + vJ[i]
    return Tw, vJ


def finish(IA, pA, S, tau):
    U = IA @ S
    D = S @ U
    Dinv = 0.0 if D == 0.0 else 1.0 / D  # fixed joint
    return U, Dinv, tau - S @ pA


def aba_textbook(parent, S, I, v, tau, fext, a0):
    n = len(parent)
    Tw, vJ = kinematics(parent, S, v)
    c = np.array([crm(Tw[i]) @ vJ[i] for i in range(n)])
    IA = I.copy()
    pA = np.array([-crm(Tw[i]).T @ (I[i] @ Tw[i]) - fext[i] for i in range(n)])  # T x* I T - f
    U, Dinv, u = np.zeros((n, 6)), np.zeros(n), np.zeros(n)
    for i in range(n - 1, -1, -1):
        U[i], Dinv[i], u[i] = finish(IA[i], pA[i], S[i], tau[i])
        if parent[i] >= 0:
            Ia = IA[i] - np.outer(U[i], U[i]) * Dinv[i]
            IA[parent[i]] += Ia
            pA[parent[i]] += pA[i] + Ia @ c[i] + U[i] * (Dinv[i] * u[i])
    a, vd = np.zeros((n, 6)), np.zeros(n)
    for i in range(n):
        ap = (a[parent[i]] if parent[i] >= 0 else a0) + c[i]
        vd[i] = Dinv[i] * (u[i] - U[i] @ ap)
        a[i] = ap + S[i] * vd[i]
    return vd


def aba_bias_sweep(parent, S, I, v, tau, fext, a0):
    n = len(parent)
    Tw, _ = kinematics(parent, S, v)
    z = np.zeros((n, 6))
    for i in range(n):
        if parent[i] >= 0:
            z[i] = z[parent[i]] + crm(Tw[parent[i]]) @ Tw[i]
    IA = I.copy()
    pA = np.array([-crm(Tw[i]).T @ (I[i] @ Tw[i]) + I[i] @ z[i] - fext[i] for i in range(n)])
    U, Dinv, u = np.zeros((n, 6)), np.zeros(n), np.zeros(n)
    for i in range(n - 1, -1, -1):
        U[i], Dinv[i], u[i] = finish(IA[i], pA[i], S[i], tau[i])
        if parent[i] >= 0:
            IA[parent[i]] += IA[i] - np.outer(U[i], U[i]) * Dinv[i]
            pA[parent[i]] += pA[i] + U[i] * (Dinv[i] * u[i])
    a, vd = np.zeros((n, 6)), np.zeros(n)
    for i in range(n):
        ap = a[parent[i]] if parent[i] >= 0 else a0
        vd[i] = Dinv[i] * (u[i] - U[i] @ ap)
        a[i] = ap + S[i] * vd[i]
    return vd


def test_bias_sweep_form_matches_textbook_form():
    rng = np.random.default_rng(7)
    a0 = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 9.81])  # -gravity
    worst, fixed, wide = 0.0, 0, 0
    for t in range(200):
        n = int(rng.integers(2, 32)) if t else 31
        parent, S, I = random_tree(rng, n)
        fixed += int((np.abs(S).sum(axis=1) == 0).sum())
        wide += int((np.bincount(parent[1:], minlength=n) >= 3).sum())
        v = rng.standard_normal(n) * 2.0
        tau = rng.standard_normal(n)
        fext = rng.standard_normal((n, 6)) * (t % 2)  # every other tree without external wrenches
        ref = aba_textbook(parent, S, I, v, tau, fext, a0)
        got = aba_bias_sweep(parent, S, I, v, tau, fext, a0)
        assert np.isfinite(ref).all() and np.abs(ref).max() > 0
        fix = np.abs(S).sum(axis=1) == 0
        assert (got[fix] == 0).all() and (ref[fix] == 0).all()
        worst = max(worst, np.abs(got - ref).max() / np.abs(ref).max())
    print(f"200 trees: max relative difference of v̇ {worst:.2e}; {fixed} fixed joints, {wide} bodies with three or more children")
    assert fixed > 50 and wide > 50
    assert worst <= 1e-12, worst


def test_bias_acceleration_of_a_body_on_the_world_is_zero():
    """level 0: T_parent = 0, so z = 0 for every joint type — the floating-base solve and the world's a' = -g need no correction"""
    rng = np.random.default_rng(8)
    parent, S, _ = random_tree(rng, 6)
    Tw, vJ = kinematics(parent, S, rng.standard_normal(6))
    assert parent[0] == -1 and np.array_equal(Tw[0], vJ[0])
    assert not (crm(Tw[0]) @ vJ[0]).any() or np.abs(crm(Tw[0]) @ vJ[0]).max() <= 1e-16 * np.abs(Tw[0]).max() ** 2
    for i in range(1, 6):  # [T_parent, T_i] = [T_i, vJ_i]
        assert np.allclose(crm(Tw[parent[i]]) @ Tw[i], crm(Tw[i]) @ vJ[i], rtol=0, atol=1e-14 * max(1.0, np.abs(Tw).max() ** 2))
