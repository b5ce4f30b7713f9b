"""What the dense-solve tests hold the Cholesky kernels to (a module of helpers, no tests; numpy only).

The reference is a plain Cholesky factorisation and two substitutions on np.longdouble (64-bit mantissa on x86), batched over the leading axis.  The bounds
are the textbook's, evaluated in long double on the DEVICE's results (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.3, 10.4):

  factor     |L̂ L̂ᵀ − A| <= C γ_{n+1} |L̂||L̂ᵀ|              elementwise on the lower triangle (mass matrices have structural zeros: no ratios)
  solution   ‖b − A x̂‖₂ <= C γ_{3n+1} ‖|L̂||L̂ᵀ|‖_F ‖x̂‖₂

with γ_k = k u / (1 − k u), u the unit roundoff of the scalar type.  C = 1 for the kernels that take square roots and divide in IEEE arithmetic, one
row per lane or one thread per state (chol_solve_kernel divides by the pivot's root; chol_reg_kernel and big_chol_solve_kernel multiply the column by the
correctly rounded 1 / sqrt(d): one rounding more for an off-diagonal entry, whose column j <= n − 1 has j + 1 <= n roundings in the theorem's count, so
γ_{n+1} still covers it — they measure 0.24 of the bound at most); the MFMA tile kernels multiply by inverted 4 x 4 diagonal tiles, which the theorems do not cover: C = 1 + κ with κ the largest ∞-norm
condition number of the 4 x 4 diagonal tiles of the long-double factor (tile_kappa)."""
import numpy as np

LD = np.longdouble
UNIT_ROUNDOFF = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def spd_family(nv, B, dtype, seed):
    """A = G Gᵀ + nv I and b from a seeded generator, ROUNDED to dtype before anything else (the reference and the bounds see what the device sees); A is
    symmetric after the rounding.  Returns (A [B, nv, nv], b [B, nv]) in dtype."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((B, nv, nv))
    A = (G @ G.transpose(0, 2, 1) + nv * np.eye(nv)).astype(dtype)
    A = np.tril(A) + np.tril(A, -1).transpose(0, 2, 1)
    return A, rng.standard_normal((B, nv)).astype(dtype)


def cholesky_ld(A):
    """Lower Cholesky factor of every A[b] in long double (left-looking, column by column)."""
    A = np.asarray(A, dtype=LD)
    n = A.shape[-1]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[:, j, j] - np.einsum("bk,bk->b", L[:, j, :j], L[:, j, :j])
        L[:, j, j] = np.sqrt(d)
        if j + 1 < n:
            s = A[:, j + 1:, j] - np.einsum("bik,bk->bi", L[:, j + 1:, :j], L[:, j, :j])
            L[:, j + 1:, j] = s / L[:, j, j, None]
    return L


def solve_ld(L, b, dtype=LD):
    """x = (L Lᵀ)⁻¹ b in long double (or, for the LAPACK-style figures, in the working precision `dtype`): forward, then backward substitution."""
    L, x = np.asarray(L, dtype=dtype), np.array(b, dtype=dtype)
    n = L.shape[-1]
    for i in range(n):
        x[:, i] = (x[:, i] - np.einsum("bk,bk->b", L[:, i, :i], x[:, :i])) / L[:, i, i]
    for i in range(n - 1, -1, -1):
        x[:, i] = (x[:, i] - np.einsum("bk,bk->b", L[:, i + 1:, i], x[:, i + 1:])) / L[:, i, i]
    return x


def gamma(k, dtype):
    u = LD(UNIT_ROUNDOFF[np.dtype(dtype)])
    return k * u / (1 - k * u)


def tile_kappa(Lref):
    """The largest ∞-norm condition number of the 4 x 4 diagonal tiles of the (long double) factor, over the batch.  A ragged last tile counts with its real
    m x m part only: the identity the tile kernels pad it with carries no rounding error (1 / sqrt(1) and the products with it are exact)."""
    Lref = np.asarray(Lref, dtype=LD)
    n = Lref.shape[-1]
    worst = 0.0
    for t0 in range(0, n, 4):
        m = min(4, n - t0)
        T = Lref[:, t0:t0 + m, t0:t0 + m]
        Ti = np.zeros_like(T)  # inverse of a lower-triangular tile by forward substitution on the identity
        for c in range(m):
            for r in range(c, m):
                Ti[:, r, c] = ((1.0 if r == c else 0.0) - np.einsum("bk,bk->b", T[:, r, c:r], Ti[:, c:r, c])) / T[:, r, r]
        k = np.abs(T).sum(axis=2).max(axis=1) * np.abs(Ti).sum(axis=2).max(axis=1)
        worst = max(worst, float(k.max()))
    return worst


def factor_figure(A, Lhat, dtype):
    """max over the lower triangle and the batch of |L̂L̂ᵀ − A| / (γ_{n+1} |L̂||L̂ᵀ|) where the bound is non-zero; where it is zero the residual must be zero
    too (else inf).  <= C passes.  An entry of L̂ that is not finite gives inf."""
    A, L = np.asarray(A, dtype=LD), np.tril(np.asarray(Lhat, dtype=LD))
    n = A.shape[-1]
    if not np.isfinite(L).all():
        return np.inf
    res = np.abs(L @ L.transpose(0, 2, 1) - A)
    bound = gamma(n + 1, dtype) * (np.abs(L) @ np.abs(L).transpose(0, 2, 1))
    il = np.tril_indices(n)
    res, bound = res[:, il[0], il[1]], bound[:, il[0], il[1]]
    if (res[bound == 0] != 0).any():
        return np.inf
    nz = bound > 0
    return float((res[nz] / bound[nz]).max())


def solution_figure(A, b, Lhat, xhat, dtype):
    """max over the batch of ‖b − A x̂‖₂ / (γ_{3n+1} ‖|L̂||L̂ᵀ|‖_F ‖x̂‖₂).  <= C passes."""
    A, b, L, x = (np.asarray(a, dtype=LD) for a in (A, b, np.tril(np.asarray(Lhat, dtype=LD)), xhat))
    n = A.shape[-1]
    if not (np.isfinite(L).all() and np.isfinite(x).all()):
        return np.inf
    r = np.sqrt(((b - np.einsum("bij,bj->bi", A, x)) ** 2).sum(axis=1))
    LL = np.abs(L) @ np.abs(L).transpose(0, 2, 1)
    bound = gamma(3 * n + 1, dtype) * np.sqrt((LL ** 2).sum(axis=(1, 2))) * np.sqrt((x ** 2).sum(axis=1))
    return float((r / bound).max())


def lapack_solution(A, b):
    """The working precision of A on the CPU: (L, x) with L from numpy's LAPACK (potrf) and x from that factor by the two substitutions, every operation
    rounded to A's type (cho_solve style)."""
    L = np.linalg.cholesky(A)
    assert L.dtype == A.dtype
    x = solve_ld(L, b, A.dtype)
    assert x.dtype == A.dtype
    return L, x
