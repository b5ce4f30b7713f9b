"""The checker of tests/test_dense_solve_gpu.py checked on the CPU (tests/dense_solve_ref.py): the long-double reference is a Cholesky solve, a correct
working-precision factorisation (numpy's LAPACK) passes the derived bounds at C = 1, and a factor that is wrong by a few units of the bound fails them.
That is the evidence that the GPU tests notice a slightly wrong kernel."""
import numpy as np
import pytest

import dense_solve_ref as ref

SIZES = [1, 5, 36, 48, 65, 96]
B = 37
DTYPES = {"f32": np.float32, "f64": np.float64}
# one entry of the factor scaled by 1 + this: 1000 (fp32) and 1800 (fp64) units in the last place
NUDGE = {"f32": 1.2e-4, "f64": 4e-13}


def family(nv, dtype):
    return ref.spd_family(nv, B, DTYPES[dtype], 1000 + nv)


def test_long_double_has_a_64_bit_mantissa():
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("nv", SIZES)
def test_reference_is_a_cholesky_solve(nv):
    A, b = family(nv, "f64")
    L = ref.cholesky_ld(A)
    assert (np.triu(L, 1) == 0).all() and (np.diagonal(L, axis1=1, axis2=2) > 0).all()
    Al = A.astype(np.longdouble)
    assert np.abs(L @ L.transpose(0, 2, 1) - Al).max() <= 8 * nv * np.finfo(np.longdouble).eps * np.abs(Al).max()
    x = ref.solve_ld(L, b)
    r = np.einsum("bij,bj->bi", Al, x) - b
    assert np.abs(r).max() <= 64 * nv * np.finfo(np.longdouble).eps * np.abs(Al).max() * np.abs(x).max()
    assert np.abs(L.astype(np.float64) - np.linalg.cholesky(A)).max() <= 1e-13 * np.abs(A).max() ** 0.5


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nv", SIZES)
def test_lapack_passes_at_c_1(nv, dtype):
    A, b = family(nv, dtype)
    L, x = ref.lapack_solution(A, b)
    f, s = ref.factor_figure(A, L, A.dtype), ref.solution_figure(A, b, L, x, A.dtype)
    print("lapack %s nv %3d  factor %.3e  solution %.3e  (of the C = 1 bound)  tile kappa %.2f" % (dtype, nv, f, s, ref.tile_kappa(ref.cholesky_ld(A))))
    assert f <= 1.0 and s <= 1.0, (f, s)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nv", SIZES)
def test_a_slightly_wrong_factor_fails(nv, dtype):
    A, b = family(nv, dtype)
    L, _ = ref.lapack_solution(A, b)
    bad = L.astype(np.longdouble)
    bad[B // 2, nv - 1, nv - 1] *= 1 + np.longdouble(NUDGE[dtype])  # one entry of one state
    f = ref.factor_figure(A, bad, A.dtype)
    print("nudged %s nv %3d  factor %.3e of the C = 1 bound" % (dtype, nv, f))
    assert f > 2 * (1.0 + ref.tile_kappa(ref.cholesky_ld(A))), f  # twice over the tile kernels' C = 1 + κ as well (κ <= 4.2 on these matrices)


def test_tile_kappa_counts_the_real_part_of_a_ragged_tile():
    L = np.zeros((1, 5, 5))
    L[0] = np.diag([6.0, 6.0, 6.0, 6.0, 6.0])
    assert ref.tile_kappa(L) == 1.0  # (padding the last 1 x 1 tile with ones would give 6)
    L[0, 1, 0] = 6.0
    assert ref.tile_kappa(L) == 4.0  # [[6, 0], [6, 6]] inside the first tile: ‖T‖ = 12, ‖T⁻¹‖ = 1/3
    for nv in SIZES:
        if nv <= 40:
            assert ref.tile_kappa(ref.cholesky_ld(family(nv, "f64")[0])) <= 4.2


def test_figures_flag_what_is_not_finite_and_nonzero_structural_zeros():
    A, b = family(5, "f64")
    L, x = ref.lapack_solution(A, b)
    bad = L.copy()
    bad[3, 4, 2] = np.nan
    assert ref.factor_figure(A, bad, A.dtype) == np.inf and ref.solution_figure(A, b, bad, x, A.dtype) == np.inf
    # a block-diagonal matrix: the bound of an entry outside the blocks is exactly zero, any residual there is a failure
    A[:, 3:, :3] = 0
    A[:, :3, 3:] = 0
    L = np.linalg.cholesky(A)
    assert ref.factor_figure(A, L, A.dtype) <= 1.0
    A2 = A.copy()
    A2[0, 4, 1] = A2[0, 1, 4] = 1e-30
    assert ref.factor_figure(A2, L, A.dtype) == np.inf
