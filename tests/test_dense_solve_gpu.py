"""The dense solve L = chol(M), x = M⁻¹(rhs − c) on its own: every kernel launch_chol_solve / dense_solve (csrc/rbd_capi.hip) can pick, at every size where
the choice changes and next to it, in both scalar types and both layouts, on caller-provided matrices through rbd_cholesky_solve; then the routes that end in
it on mechanisms at and beyond 64 velocity coordinates.

    nv <= 40   chol_mfma_kernel<NT> (fp32, 16 states per wavefront), chol_mfma64_kernel<NT> (fp64, 4 per wavefront), NT in {1, 2, 4, 6, 8, 9, 10}    "tile"
    41 .. 48   chol_reg_kernel<T, 48>                                                                                                                "reg"
    49 .. 64   chol_solve_kernel (factor in LDS, one row per lane)                                                                                  "lds"
    > 64       big_chol_solve_kernel (one thread per state), also for trees of at most 64 bodies                                                    "thread"

Reference and bounds: tests/dense_solve_ref.py (long double; Higham Thm 10.3 / 10.4 evaluated on the device's own L̂ and x̂; C = 1, for the tile kernels
C = 1 + κ of the 4 x 4 diagonal tiles).  tests/test_dense_solve_bounds_cpu.py shows that LAPACK passes them and a slightly wrong factor does not.
Every figure is printed before it is asserted (pytest -s; profiles/dense_solve_parity.txt keeps a run's).

Measured on an MI355X: profiles/dense_solve_parity.txt.  Largest fraction of the class's bound, factor / solution: tile 0.85 / 0.35 (fp64) and
0.75 / 0.19 (fp32), both at nv = 1, where the figure is 1.7 and 1.5 times the C = 1 bound (the tile kernels multiply by 1 / sqrt(d) instead of dividing) and
C = 1 + κ = 2; reg 0.24 / 0.006; lds 0.18 / 0.004; thread 0.17 / 0.003.  LAPACK on the CPU: 0.90 / 0.62 at nv = 1, below 0.09 / 0.003 from nv = 36 up."""
import ctypes

import numpy as np
import pytest
import torch

import dense_solve_ref as ref
from conftest import rand_inputs
from test_derivatives_gpu import NV_OVER_64_TYPES, at_most_3_children  # (the two nv > 64 mechanisms of the derivative tests: one definition)

pytestmark = pytest.mark.gpu

TD = {"f64": torch.float64, "f32": torch.float32}
ND = {"f64": np.float64, "f32": np.float32}
TOL = {"f64": 1e-12, "f32": 2e-5}  # the forward tolerance of test_gpu_parity's direct tests
SIZES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 25, 32, 33, 36, 37, 40, 41, 44, 47, 48, 49, 63, 64, 65, 66, 96, 129]
EDGE_SIZES = [7, 36, 44, 58, 66]  # one per kernel (two tile instantiations)
B_RAGGED = 37  # ragged for 16 and for 4 states per wavefront, and for 4 states per workgroup


def kernel_class(nv):
    return "tile" if nv <= 40 else "reg" if nv <= 48 else "lds" if nv <= 64 else "thread"


_models, _cases = {}, {}


def chol_model(rbd, nv):
    """A mechanism with nv velocity coordinates and at most 64 bodies (rbd_cholesky_solve uses nothing else of it)."""
    if nv not in _models:
        types = ["Revolute"] * nv if nv <= 64 else ["QuaternionSpherical"] * (nv // 3) + ["Revolute"] * (nv % 3)
        _models[nv] = rbd.flatten(rbd.rand_tree_mechanism(np.random.default_rng(200 + nv), types, at_most_3_children))
        assert _models[nv].nv == nv and _models[nv].n_bodies <= 64
    return _models[nv]


def case(nv, dtype):
    """The matrices of a size and type with their long-double factor and solution: computed once, shared, never modified."""
    key = (nv, dtype)
    if key not in _cases:
        A, b = ref.spd_family(nv, B_RAGGED, ND[dtype], 1000 + nv)
        L = ref.cholesky_ld(A)
        c = dict(A=A, b=b, L=L, x=ref.solve_ld(L, b), kappa=ref.tile_kappa(L))
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cases[key] = c
    return _cases[key]


def pack(A, upper=0.0):
    """[B, nv, nv] -> [B, nv nv] column-major per state, the lower triangle of A and `upper` in the strict upper one."""
    nv = A.shape[-1]
    M = np.where(np.tri(nv, dtype=bool), A, A.dtype.type(upper))
    return M.transpose(0, 2, 1).reshape(A.shape[0], nv * nv)


def unpack(t, nv):
    """[B, nv nv] column-major per state -> [B, row, col] (everything, the strict upper triangle included)."""
    return t.reshape(t.shape[0], nv, nv).transpose(0, 2, 1)


def to_dev(a, dtype, layout):
    t = torch.as_tensor(np.ascontiguousarray(a), dtype=TD[dtype])
    return (t if layout == "aos" else t.t().contiguous()).cuda()


def to_host(t, layout):
    t = t.detach().cpu()
    return (t if layout == "aos" else t.t()).numpy().copy()  # in the scalar type: bit patterns kept


P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())


def solve(rbd, st, B, M, rhs, x, L):
    from rigidbodydynamics_jl_amd import _capi
    opts = st._opts()
    assert _capi.lib().rbd_cholesky_solve(st.ws.handle, B, P(M), P(rhs), P(x), P(L), ctypes.byref(opts)) == 0


def run(rbd, st, dtype, layout, M, b, want_L=True, fill=float("nan")):
    """One call on host arrays M [B, nv nv], b [B, nv]: (x [B, nv], L [B, nv nv] or None, status of rbd.sync)."""
    B = M.shape[0]
    Md, bd = to_dev(M, dtype, layout), to_dev(b, dtype, layout)
    x = torch.full_like(bd, fill)
    L = torch.full_like(Md, fill) if want_L else None
    solve(rbd, st, B, Md, bd, x, L)
    status = rbd.sync(st)
    return to_host(x, layout), (to_host(L, layout) if want_L else None), status


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cls", ["tile", "reg", "lds", "thread"])
def test_factor_and_solution_at_every_dispatch_edge(rbd, cls, dtype, layout):
    """Every size of SIZES that the kernel class serves, B = 1 and B = 37: the derived backward bounds on the device's L̂ and x̂ (elementwise for the factor),
    the forward checks of the existing direct tests, status 0, and nothing written above the diagonal of L_out."""
    worst = dict(factor=0.0, solution=0.0)
    failures = []
    for nv in [n for n in SIZES if kernel_class(n) == cls]:
        c = case(nv, dtype)
        st = rbd.MechanismState(chol_model(rbd, nv), B_RAGGED, dtype=TD[dtype], layout=layout)
        C = 1.0 + c["kappa"] if cls == "tile" else 1.0
        for B in (1, B_RAGGED):
            A, b = c["A"][:B], c["b"][:B]
            x, L, status = run(rbd, st, dtype, layout, pack(A), b)
            assert status == 0, (nv, B, status)
            Lfull = unpack(L, nv)
            iu = np.triu_indices(nv, 1)
            assert np.isnan(Lfull[:, iu[0], iu[1]]).all(), (nv, B, "the strict upper triangle of L_out was written")
            Lg = np.tril(Lfull)
            assert np.isfinite(Lg).all() and np.isfinite(x).all(), (nv, B)
            f, s = ref.factor_figure(A, Lg, ND[dtype]), ref.solution_figure(A, b, Lg, x, ND[dtype])
            print("dense_solve %-6s %s %s nv %3d B %2d  factor %.3e  solution %.3e  of the C = 1 bound; C = %.2f" % (cls, dtype, layout, nv, B, f, s, C))
            worst["factor"], worst["solution"] = max(worst["factor"], f / C), max(worst["solution"], s / C)
            if f > C or s > C:
                failures.append((nv, B, f, s, C))
            assert np.abs(Lg - c["L"][:B]).max() <= TOL[dtype] * np.abs(A).max() ** 0.5, (nv, B)
            assert np.abs(x - c["x"][:B]).max() <= TOL[dtype] * max(1.0, float(np.abs(c["x"][:B]).max())), (nv, B)
    print("dense_solve_worst %-6s %s %s  factor %.3e  solution %.3e  of the bound C" % (cls, dtype, layout, worst["factor"], worst["solution"]))
    assert not failures, failures


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nv", EDGE_SIZES)
def test_upper_triangle_is_never_read(rbd, nv, dtype, layout):
    c = case(nv, dtype)
    st = rbd.MechanismState(chol_model(rbd, nv), B_RAGGED, dtype=TD[dtype], layout=layout)
    x0, L0, s0 = run(rbd, st, dtype, layout, pack(c["A"]), c["b"])
    x1, L1, s1 = run(rbd, st, dtype, layout, pack(c["A"], float("nan")), c["b"])
    assert s0 == 0 and s1 == 0
    assert np.isfinite(x0).all() and x0.tobytes() == x1.tobytes()
    il = np.tril_indices(nv)
    a, b = unpack(L0, nv)[:, il[0], il[1]], unpack(L1, nv)[:, il[0], il[1]]
    assert np.isfinite(a).all() and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nv", EDGE_SIZES)
def test_canaries_behind_x_and_l_out(rbd, nv, dtype):
    """AOS buffers with 3 states of 777 behind the 37 of the call stay untouched; without L_out the same x bit for bit."""
    c = case(nv, dtype)
    B = B_RAGGED
    st = rbd.MechanismState(chol_model(rbd, nv), B, dtype=TD[dtype])
    M, b = to_dev(pack(c["A"]), dtype, "aos"), to_dev(c["b"], dtype, "aos")
    x = torch.full((B + 3, nv), 777.0, dtype=TD[dtype], device="cuda")
    L = torch.full((B + 3, nv * nv), 777.0, dtype=TD[dtype], device="cuda")
    solve(rbd, st, B, M, b, x, L)
    assert rbd.sync(st) == 0
    assert (x[B:] == 777).all() and (L[B:] == 777).all()
    assert torch.isfinite(x[:B]).all() and (x[:B] != 777).all()
    iu = np.triu_indices(nv, 1)
    assert (unpack(L[:B].cpu().numpy(), nv)[:, iu[0], iu[1]] == 777).all()
    x2 = torch.full((B + 3, nv), 777.0, dtype=TD[dtype], device="cuda")
    solve(rbd, st, B, M, b, x2, None)
    assert rbd.sync(st) == 0
    assert torch.equal(x, x2)


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nv", EDGE_SIZES)
def test_states_are_independent_and_the_flag_is_reported_once(rbd, nv, dtype, layout):
    """One bad state (all NaN, or −A: not positive definite) at the head, inside, at the start of a second fp32 wavefront, at the ragged tail: every other
    state's x and L bit-identical to the clean run, rbd.sync 8 once and then 0; the clean run 0."""
    c = case(nv, dtype)
    st = rbd.MechanismState(chol_model(rbd, nv), B_RAGGED, dtype=TD[dtype], layout=layout)
    M = pack(c["A"])
    x0, L0, s0 = run(rbd, st, dtype, layout, M, c["b"])
    assert s0 == 0 and rbd.sync(st) == 0
    assert np.isfinite(x0).all()
    il = np.tril_indices(nv)
    low = lambda L: unpack(L, nv)[:, il[0], il[1]]
    for bad in (0, 5, 16, 36):
        keep = [i for i in range(B_RAGGED) if i != bad]
        for kind in ("nan", "negated"):
            Mb = M.copy()
            Mb[bad] = np.nan if kind == "nan" else -M[bad]
            x1, L1, s1 = run(rbd, st, dtype, layout, Mb, c["b"])
            assert s1 == 8, (bad, kind, s1)
            assert rbd.sync(st) == 0
            assert x1[keep].tobytes() == x0[keep].tobytes(), (bad, kind)
            assert low(L1)[keep].tobytes() == low(L0)[keep].tobytes(), (bad, kind)


# ---- through the routes: mechanisms at and beyond 64 velocity coordinates, at most 64 bodies -------------------------------------------------------------------
ROUTE_MECHANISMS = {
    "nv66_spherical": NV_OVER_64_TYPES["nv66_spherical"],
    "nv65_mixed": NV_OVER_64_TYPES["nv65_mixed"],
    "nv96_floating": ["QuaternionFloating"] * 16,
    "nv64_revolute": ["Revolute"] * 64,  # both lane limits at once: 64 bodies, 64 rows
    "nv44_floating_revolute": ["QuaternionFloating"] + ["Revolute"] * 38,  # chol_reg_kernel
    # a hub with 11 children: more than a lane-per-body record lists (8), so M and c come from the any-size kernels — and the solve, chosen by nv alone,
    # from the tile kernels (nv = 22), not from the any-size route's one-thread kernel
    "nv22_hub_11_children": [("QuaternionFloating", [(k, [("Revolute", [])] if i < 2 else []) for i, k in enumerate(
        ["Revolute", "Prismatic", "Planar", "QuaternionSpherical", "SinCosRevolute", "Revolute", "Revolute", "Prismatic", "Revolute", "Fixed", "Revolute"])])],
}
ROUTE_NV = {"nv66_spherical": (22, 66), "nv65_mixed": (26, 65), "nv96_floating": (16, 96), "nv64_revolute": (64, 64), "nv44_floating_revolute": (39, 44),
            "nv22_hub_11_children": (14, 22)}
_route_models = {}


def route_model(rbd, name):
    if name not in _route_models:
        rng = np.random.default_rng(5)
        mech = rbd.builders.tree_mechanism(rng, ROUTE_MECHANISMS[name]) if "hub" in name else rbd.rand_tree_mechanism(rng, ROUTE_MECHANISMS[name], at_most_3_children)
        _route_models[name] = rbd.flatten(mech)
        assert (_route_models[name].n_bodies, _route_models[name].nv) == ROUTE_NV[name]
    return _route_models[name]


def sym(M):
    return np.tril(M) + np.transpose(np.tril(M, -1), (0, 2, 1))


def make(rbd, model, B, dtype, layout, seed):
    q, v, tau, fe = rand_inputs(rbd, model, B, seed, fext=True)
    state = rbd.MechanismState(model, B, dtype=TD[dtype], layout=layout)
    rbd.set_configuration_(state, q)
    rbd.set_velocity_(state, v)
    q, v, tau, fe = [a.astype(ND[dtype]).astype(np.float64) for a in (q, v, tau, fe)]  # the inputs as the device sees them
    return state, q, v, tau, fe


def h64(t, layout):
    return to_host(t, layout).astype(np.float64)


def assert_solution(dtype, got, Ms, r, what):
    """x̂ of M x = r: fp64 against numpy's solve of the oracle's M at 1e-9 max(1, max|ref|) (the LDS-kernel test's), fp32 by the normwise backward error
    ‖M x̂ − r‖ / (‖M‖‖x̂‖ + ‖r‖) <= 2e-5 with the oracle's M."""
    assert np.isfinite(got).all(), what
    if dtype == "f64":
        xr = np.linalg.solve(Ms, r[..., None])[..., 0]
        err = np.abs(got - xr).max() / max(1.0, np.abs(xr).max())
        print("route %-28s f64 err %.3e  bound 1e-9" % (what, err))
        assert err <= 1e-9, (what, err)
    else:
        res = np.einsum("bij,bj->bi", Ms, got) - r
        eta = (np.linalg.norm(res, axis=1) / (np.linalg.norm(Ms, axis=(1, 2)) * np.linalg.norm(got, axis=1) + np.linalg.norm(r, axis=1))).max()
        print("route %-28s f32 eta %.3e  bound 2e-5" % (what, eta))
        assert eta <= 2e-5, (what, eta)


def assert_lower(dtype, Mg, Mr, what):
    il = np.tril_indices(Mr.shape[-1])
    g, r = Mg[:, il[0], il[1]], Mr[:, il[0], il[1]]
    assert np.isfinite(g).all(), what
    if dtype == "f64":
        assert np.abs(g - r).max() <= 1e-10 * max(1.0, np.abs(r).max()), what  # (test_dynamics_crba_cholesky_route_f64)
    else:
        assert np.abs(g - r).max() <= 2e-5 * np.abs(r).max(), what  # (test_rnea_crba_f32: no solve involved)


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", list(ROUTE_MECHANISMS))
def test_routes_on_mechanisms_at_and_beyond_64_coordinates(rbd, oracle, name, dtype, layout):
    """dynamics! (CRBA and ABA), mass_matrix_solve (Cholesky with and without M_out, packed, ABA) at the library's default routing for B = 21, against the
    oracle's M, c and dynamics; rbd.sync == 0 after each call."""
    model = route_model(rbd, name)
    nv, B = model.nv, 21
    state, q, v, tau, fe = make(rbd, model, B, dtype, layout, 77)
    d = lambda a: to_dev(a, dtype, layout)
    Mr = oracle.mass_matrix(model, q)
    Ms, cr = sym(Mr), oracle.dynamics_bias(model, q, v, fe)
    ref_vd = oracle.dynamics(model, q, v, tau, fe)
    assert np.abs(ref_vd - np.linalg.solve(Ms, (tau - cr)[..., None])[..., 0]).max() <= 1e-10 * max(1.0, np.abs(ref_vd).max())  # the oracle against itself
    # dynamics!, the reference's route: v̇, result.massmatrix (lower), result.dynamicsbias
    result = rbd.DynamicsResult(model, B, dtype=TD[dtype], layout=layout)
    result.massmatrix.fill_(float("nan"))
    rbd.dynamics_(result, state, d(tau), d(fe), algorithm="crba")
    assert rbd.sync(state) == 0
    vd_crba = h64(result.vd, layout)
    assert_solution(dtype, vd_crba, Ms, tau - cr, name + " dynamics crba")
    assert_lower(dtype, unpack(h64(result.massmatrix, layout), nv), Mr, name + " result.massmatrix")
    cg = h64(result.dynamicsbias, layout)
    assert np.abs(cg - cr).max() <= (1e-10 * max(1.0, np.abs(cr).max()) if dtype == "f64" else 2e-5 * np.abs(cr).max())
    # the fused ABA agrees
    r2 = rbd.DynamicsResult(model, B, dtype=TD[dtype], layout=layout)
    rbd.dynamics_(r2, state, d(tau), d(fe), algorithm="aba")
    assert rbd.sync(state) == 0
    vd_aba = h64(r2.vd, layout)
    assert_solution(dtype, vd_aba, Ms, tau - cr, name + " dynamics aba")
    if dtype == "f64":
        assert np.abs(vd_aba - vd_crba).max() <= 1e-9 * max(1.0, np.abs(ref_vd).max())
    else:  # fp32, the two routes against each other, state by state: each is held to 8 cond₂(M_b) eps32 of the solution (test_gpu_parity.assert_fp32_forward), so
        # they are within twice that of one another
        gap = np.linalg.norm(vd_aba - vd_crba, axis=1) / np.linalg.norm(vd_crba, axis=1)
        bound = 2 * 8.0 * np.linalg.cond(Ms) * np.finfo(np.float32).eps
        print("route %-28s f32 aba vs crba %.3e of 16 cond eps32" % (name, (gap / bound).max()))
        assert (gap <= bound).all(), (name, float((gap / bound).max()))
    # mass_matrix_solve: Cholesky with M_out, without, packed; ABA
    rhs = tau
    x = torch.full_like(state.v, float("nan"))
    Mout = torch.full_like(result.massmatrix, float("nan"))
    rbd.mass_matrix_solve_(x, state, d(rhs), Mout, algorithm="cholesky")
    assert rbd.sync(state) == 0
    x_with = x.clone()
    assert_solution(dtype, h64(x, layout), Ms, rhs, name + " solve cholesky M_out")
    assert_lower(dtype, unpack(h64(Mout, layout), nv), Mr, name + " M_out")
    x.fill_(float("nan"))
    rbd.mass_matrix_solve_(x, state, d(rhs), None, algorithm="cholesky")
    assert rbd.sync(state) == 0
    assert_solution(dtype, h64(x, layout), Ms, rhs, name + " solve cholesky")
    assert torch.equal(x, x_with)  # the same kernels at this batch, with or without the caller's M
    npk = nv * (nv + 1) // 2
    Pk = torch.full((B, npk) if layout == "aos" else (npk, B), float("nan"), dtype=TD[dtype], device="cuda")
    x.fill_(float("nan"))
    rbd.mass_matrix_solve_(x, state, d(rhs), Pk, algorithm="cholesky", packed=True)
    assert rbd.sync(state) == 0
    assert_solution(dtype, h64(x, layout), Ms, rhs, name + " solve packed")
    Pg = h64(Pk, layout)
    i, j = np.tril_indices(nv)
    Mp = np.zeros((B, nv, nv))
    Mp[:, i, j] = Pg[:, i + j * (2 * nv - j - 1) // 2]
    assert np.isfinite(Pg).all()
    assert_lower(dtype, Mp, Mr, name + " packed M_out")
    x.fill_(float("nan"))
    rbd.mass_matrix_solve_(x, state, d(rhs), None, algorithm="aba")
    assert rbd.sync(state) == 0
    assert_solution(dtype, h64(x, layout), Ms, rhs, name + " solve aba")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nv", EDGE_SIZES)
def test_rhs_conventions_through_dynamics(rbd, oracle, nv, dtype):
    """The right-hand side rhs − c with either part missing, through rbd_dynamics on the reference's route: τ = None gives M⁻¹(−c), with and without external
    wrenches; τ without wrenches."""
    model = chol_model(rbd, nv)
    B = B_RAGGED
    state, q, v, tau, fe = make(rbd, model, B, dtype, "aos", 78)
    Ms = sym(oracle.mass_matrix(model, q))
    for what, t, f in (("no tau, no wrenches", None, None), ("no tau, wrenches", None, fe), ("tau, no wrenches", tau, None)):
        c = oracle.dynamics_bias(model, q, v, f)
        result = rbd.DynamicsResult(model, B, dtype=TD[dtype])
        result.vd.fill_(float("nan"))
        rbd.dynamics_(result, state, None if t is None else to_dev(t, dtype, "aos"), None if f is None else to_dev(f, dtype, "aos"), algorithm="crba")
        assert rbd.sync(state) == 0
        r = (0.0 if t is None else t) - c
        assert_solution(dtype, h64(result.vd, "aos"), Ms, r, "nv %d %s" % (nv, what))
        if dtype == "f64":
            vr = oracle.dynamics(model, q, v, t, f)
            assert np.abs(h64(result.vd, "aos") - vr).max() <= 1e-9 * max(1.0, np.abs(vr).max())
