"""What the derivative tests hold the kernels to, and the plain fp64 evaluation the bounds come from (a module of helpers, no tests).

The reference is the quad-precision oracle (oracle/rbd_oracle_q.c): exact to double rounding, so a bound states the arithmetic of the result, not the reference.
  * No solve in the result (tangents, Jacobians and VJPs of inverse dynamics): the project's fp64 parity number, err <= 1e-10 (1 + max|ref|).
  * Through M⁻¹ (everything of dynamics): state by state, ‖got − ref‖ / ‖ref‖ <= C · cond₂(M_b) · eps64, the form of test_gpu_parity.assert_fp32_forward.
    C is not fitted to the kernels: it is what a plain numpy fp64 evaluation of the same quantity loses — −M⁻¹ (∂τ/∂·) formed from the quad ∂τ and the fp64
    oracle's M, against the quad derivative of dynamics — at its worst over the test models and states, times the project's margin of 8
    (scripts/measure_derivative_parity.py writes profiles/derivative_parity.txt)."""
import numpy as np

EPS64 = np.finfo(np.float64).eps
MARGIN = 8.0  # the C of test_gpu_parity.assert_fp32_forward
# profiles/derivative_parity.txt, column "constant": the largest err / (cond₂(M_b) eps64) of the numpy fp64 chain rule per model, over the Jacobians and
# the directional derivative on the test states
FP64_LOSS = {"atlas_floating": 2.755e-02, "atlas_fixed": 2.619e-02, "valkyrie_floating": 4.171e-02, "double_pendulum": 2.360e+00,
             "randmech1": 1.539e-01, "randmech2": 2.620e-01, "randmech3": 2.774e-01, "inner_floating": 1.333e+00, "mixed20": 7.901e-01,
             "chain70": 1.118e-02, "tree20": 2.929e-02, "limbs_humanoid": 3.405e-02, "limbs_only_children": 2.258e+00, "limbs_quadruped": 5.183e-01,
             "limbs_three": 2.773e-01, "nv66_spherical": 1.784e-01, "nv65_mixed": 2.919e-02}


def C_solve(name):
    return MARGIN * FP64_LOSS[name]


def close(got, ref, tol, what=""):
    err = np.abs(got - ref).max()
    assert err <= tol * (1 + np.abs(ref).max()), (what, err, np.abs(ref).max())


def sym(M):
    """The oracle's mass matrix (lower triangle) made symmetric."""
    return np.tril(M) + np.transpose(np.tril(M, -1), (0, 2, 1))


def cond_M(oracle, flat, q):
    return np.linalg.cond(sym(oracle.mass_matrix(flat, q)))


def solve_loss(got, ref, kappa):
    """err_b / (cond₂(M_b) eps64) per state; got, ref: [B, ...] (a state's matrix counts as one vector)."""
    B = ref.shape[0]
    g, r = got.reshape(B, -1), ref.reshape(B, -1)
    return np.linalg.norm(g - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-300) / (kappa * EPS64)


def assert_solve_forward(got, ref, kappa, name, what=""):
    """Forward error of a result through M⁻¹, state by state: ‖got − ref‖ / ‖ref‖ <= C · cond₂(M_b) · eps64 with the model's C (profiles/derivative_parity.txt).
    Prints the figure before it asserts (pytest -s: the observed column of that file)."""
    loss = solve_loss(got, ref, kappa)
    worst = int(np.argmax(loss))
    print("observed %-20s %-28s loss %.3e   bound %.3e" % (name, what, loss[worst], C_solve(name)))
    assert (loss <= C_solve(name)).all(), (name, what, worst, float(loss[worst]), C_solve(name), float(kappa[worst]))


def assert_no_solve(got, ref, name, what=""):
    """A result with no solve in it: the project's fp64 parity number, err <= 1e-10 (1 + max|ref|)."""
    print("observed %-20s %-28s err  %.3e   bound 1e-10" % (name, what, np.abs(got - ref).max() / (1 + np.abs(ref).max())))
    close(got, ref, 1e-10, (name, what))


def jvp_directions(flat, B, ntan, seed=3):
    """Random directions in (q, v, v̇, τ, f_ext), [B, ntan, n] each; dq is NOT projected on any quaternion's unit sphere (raw-coordinate derivatives)."""
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal((B, ntan, n)) for k, n in (("q", flat.nq), ("v", flat.nv), ("vd", flat.nv), ("tau", flat.nv), ("f", 6 * flat.n_bodies))}


def fp64_chain_rule(oracle, flat, q, v, tau, fext, nthreads=None):
    """The plain fp64 evaluation of the dynamics Jacobians: v̇ from the fp64 oracle, ∂τ/∂(q, v) at that v̇ from the quad oracle (exact), M from the fp64 oracle,
    then −M⁻¹ ∂τ/∂· and M⁻¹ by numpy's fp64 solve.  Returns dict(q, v, x) like oracle.jacobians."""
    vd = oracle.dynamics(flat, q, v, tau, fext)
    T = oracle.jacobians(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext, wrt="qv", nthreads=nthreads)
    Ms = sym(oracle.mass_matrix(flat, q))
    return dict(q=-np.linalg.solve(Ms, T["q"]), v=-np.linalg.solve(Ms, T["v"]), x=np.linalg.inv(Ms))


def fp64_chain_rule_jvp(oracle, flat, q, v, tau, fext, dq, dv, dtau, dfext):
    """The same for one direction: M⁻¹ (dτ − ∂τ/∂(q, v, f_ext)·d) with the quad directional derivative of inverse dynamics at the fp64 v̇."""
    vd = oracle.dynamics(flat, q, v, tau, fext)
    dT = oracle.jvp(flat, oracle.WHAT_INVERSE_DYNAMICS, q, v, vd, fext, dq, dv, None, dfext)
    return np.linalg.solve(sym(oracle.mass_matrix(flat, q)), (dtau - dT)[:, :, None])[:, :, 0]
