"""What numpy's LAPACK in the working precision reaches of the bounds that tests/test_dense_solve_gpu.py holds the Cholesky kernels to, on the same matrices:
the CPU part of profiles/dense_solve_parity.txt.  No GPU.  The GPU part of that file is the "dense_solve_worst" lines the GPU test prints (pytest -s).

  python scripts/measure_dense_solve_parity.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dense_solve_ref as ref  # noqa: E402

SIZES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 25, 32, 33, 36, 37, 40, 41, 44, 47, 48, 49, 63, 64, 65, 66, 96, 129]  # tests/test_dense_solve_gpu.py
B = 37


def kernel_class(nv):
    return "tile" if nv <= 40 else "reg" if nv <= 48 else "lds" if nv <= 64 else "thread"


def main():
    print("# fraction of the C = 1 bounds (factor: elementwise |LL' - A| <= gamma_{n+1} |L||L'|; solution: ||b - Ax|| <= gamma_{3n+1} || |L||L'| ||_F ||x||)")
    print("# reached by numpy's LAPACK potrf + two substitutions in the working precision, %d matrices per size; kappa: the largest inf-norm condition of a" % B)
    print("# 4 x 4 diagonal tile of the long-double factor (the tile kernels' C = 1 + kappa)")
    worst = {}
    for nv in SIZES:
        for name, dt in (("f64", np.float64), ("f32", np.float32)):
            A, b = ref.spd_family(nv, B, dt, 1000 + nv)
            L, x = ref.lapack_solution(A, b)
            f, s = ref.factor_figure(A, L, dt), ref.solution_figure(A, b, L, x, dt)
            kappa = ref.tile_kappa(ref.cholesky_ld(A))
            cond = np.linalg.cond(A.astype(np.float64)).max()
            print("lapack %-6s %s nv %3d  factor %.3e  solution %.3e  kappa %5.2f  cond %.1f" % (kernel_class(nv), name, nv, f, s, kappa, cond))
            w = worst.setdefault((kernel_class(nv), name), [0.0, 0.0, 0.0])
            w[0], w[1] = max(w[0], f), max(w[1], s)
            if nv <= 40:
                w[2] = max(w[2], kappa)
    for (cls, name), w in worst.items():
        print("lapack_worst %-6s %s  factor %.3e  solution %.3e  of the C = 1 bound%s" % (cls, name, w[0], w[1], "   largest kappa %.2f" % w[2] if cls == "tile" else ""))


if __name__ == "__main__":
    main()
