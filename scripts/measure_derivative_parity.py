"""What a plain fp64 evaluation of the dynamics derivatives loses against the quad-precision oracle, per model: the origin of the constant of
tests/derivative_parity.py.  No GPU.  Writes the first part of profiles/derivative_parity.txt (the GPU's observed errors are appended by the GPU tests' records).

  python scripts/measure_derivative_parity.py > profiles/derivative_parity.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import oracle  # noqa: E402
import rbd_amd as rbd  # noqa: E402
from conftest import LIMBS, build_models, rand_inputs  # noqa: E402
from derivative_parity import cond_M, fp64_chain_rule, fp64_chain_rule_jvp, jvp_directions, solve_loss  # noqa: E402
from test_derivatives_gpu import FD_MODELS, NV_OVER_64, model  # noqa: E402

B, SEED = 8, 11  # the states of tests/test_derivatives_gpu.py::test_jacobians_against_the_quad_oracle (its first 8) and of test_jvp_against_the_quad_oracle


def jvp_loss(flat, name):
    """The same for the directional derivatives along (dq, dv, dτ, df_ext), on the states and directions of test_jvp_against_the_quad_oracle."""
    Bj, ntan = (4096, 1) if name == "atlas_floating" else (16, 2)
    q, v, tau, fext = rand_inputs(rbd, flat, Bj, SEED, fext=True)
    d = jvp_directions(flat, Bj, ntan)
    kappa = cond_M(oracle, flat, q)
    ref = oracle.jvp(flat, oracle.WHAT_DYNAMICS, q, v, tau, fext, d["q"], d["v"], d["tau"], d["f"])
    got = [fp64_chain_rule_jvp(oracle, flat, q, v, tau, fext, d["q"][:, k], d["v"][:, k], d["tau"][:, k], d["f"][:, k]) for k in range(ntan)]
    return max(solve_loss(got[k], ref[:, k], kappa).max() for k in range(ntan))


def main():
    models = build_models(rbd)
    print("# err_b / (cond2(M_b) eps64), worst of %d states (rand_inputs seed %d, external wrenches present): numpy fp64 chain rule -M^-1 (dtau/d.) [quad dtau, fp64 M, fp64 vdot]" % (B, SEED))
    print("# against the quad derivative of dynamics.  Columns: dvdot/dq, dvdot/dv, dvdot/dtau = M^-1 (a state's matrix as one vector),")
    print("# the directional derivatives along (dq, dv, dtau, dfext) on the states of the JVP test (4096 for atlas_floating, else 16), the model's constant = the largest of the four, max cond2(M).")
    worst = 0.0
    for name in FD_MODELS + ["tree20"] + LIMBS + NV_OVER_64:
        flat = model(rbd, models, name)
        q, v, tau, fext = rand_inputs(rbd, flat, B, SEED, fext=True)
        ref = oracle.jacobians(flat, oracle.WHAT_DYNAMICS, q, v, tau, fext)
        got = fp64_chain_rule(oracle, flat, q, v, tau, fext)
        kappa = cond_M(oracle, flat, q)
        loss = [solve_loss(got[k], ref[k], kappa).max() for k in "qvx"]
        loss.append(jvp_loss(flat, name))
        worst = max(worst, *loss)
        print("fp64_chain_rule %-20s %.3e %.3e %.3e %.3e   constant %.3e   cond %.2e" % (name, *loss, max(loss), kappa.max()))
        sys.stdout.flush()
    print("# worst over models: %.3e   (tests/derivative_parity.py FP64_LOSS holds the constants; a bound is 8 x the model's)" % worst)


if __name__ == "__main__":
    main()
