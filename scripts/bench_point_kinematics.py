"""Times point kinematics of four points (two hands, two feet) on Atlas with a floating base, three ways:
  (a) rbd_point_kinematics with all four outputs (positions, velocities, bias accelerations, point Jacobians): one launch;
  (b) what the library offered for the same information before: four rbd_geometric_jacobian calls (6 × nv each) plus one per-body call
      (rbd_dynamics_bias_bodies: the bodies' accelerations) — the per-point finish in torch is NOT included, so (b) is a lower bound;
  (c) rbd_point_kinematics_vjp of (pos, vel).
HIP events around `--iters` calls after `--warmup`; one JSON line per (dtype, batch) on stdout, and with --out the lines appended to that file.
  python scripts/bench_point_kinematics.py [--cases f64:4096,f64:65536,f32:65536] [--iters 20] [--warmup 5] [--out profiles/point_kinematics_bench.jsonl]"""
import argparse
import json
import os
import sys

os.environ.setdefault("RBD_JIT_ASYNC", "0")  # wait for the kernels compiled per mechanism instead of starting on the interpreting ones

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import rbd_amd as rbd  # noqa: E402
from bench_derivatives import timed  # noqa: E402

POINT_BODIES = ("l_hand", "r_hand", "l_foot", "r_foot")


def case(model, dtype, B, iters, warmup):
    nq, nv, P = model.nq, model.nv, len(POINT_BODIES)
    rng = np.random.default_rng(0)
    td = dict(dtype=dtype, device="cuda")
    s = rbd.MechanismState(model, B, dtype=dtype)
    rbd.set_configuration_(s, rbd.rand_configuration(model, B, rng))
    rbd.set_velocity_(s, rbd.rand_velocity(model, B, rng))
    bodies = [list(model.body_names).index(n) for n in POINT_BODIES]
    rbd.set_points_(s, bodies, 0.1 * rng.standard_normal((P, 3)))
    pos, vel, acc = (torch.empty((B, 3 * P), **td) for _ in range(3))
    jac = torch.empty((B, 3 * nv * P), **td)
    a_ms = timed(lambda: rbd.point_kinematics_(s, pos, vel, acc, jac), iters, warmup)
    a_kernel = rbd.last_kernel(s)
    a_pos_ms = timed(lambda: rbd.point_kinematics_(s, pos, vel), iters, warmup)
    # (b) four geometric Jacobians and the per-body call
    J = [torch.empty((B, 6 * nv), **td) for _ in range(P)]
    r = rbd.DynamicsResult(model, B, dtype=dtype, bodies=True)

    def old():
        for k, b in enumerate(bodies):
            rbd.geometric_jacobian_(J[k], s, -1, b)
        rbd.dynamics_bias_(r, s)
    b_ms = timed(old, iters, warmup)
    b_jac_ms = timed(lambda: [rbd.geometric_jacobian_(J[k], s, -1, b) for k, b in enumerate(bodies)], iters, warmup)
    rbd.geometric_jacobian_(J[0], s, -1, bodies[0])
    b_kernel = rbd.last_kernel(s)
    # (c) the pullback
    qb, vb = torch.empty((B, nq), **td), torch.empty((B, nv), **td)
    pbar, wbar = torch.as_tensor(rng.standard_normal((B, 3 * P)), **td), torch.as_tensor(rng.standard_normal((B, 3 * P)), **td)
    c_ms = timed(lambda: rbd.point_kinematics_vjp_(s, pbar, wbar, qb, vb), iters, warmup)
    c_kernel = rbd.last_kernel(s)
    return dict(metric="point_kinematics", mechanism="atlas_floating", points=list(POINT_BODIES), dtype=str(dtype).replace("torch.", ""), B=B, nq=nq, nv=nv,
                a_point_kinematics_ms=round(a_ms, 4), a_kernel=a_kernel, a_pos_vel_only_ms=round(a_pos_ms, 4), b_four_jacobians_plus_bodies_ms=round(b_ms, 4),
                b_four_jacobians_ms=round(b_jac_ms, 4), b_kernel=b_kernel, c_vjp_ms=round(c_ms, 4), c_kernel=c_kernel, a_over_b=round(a_ms / b_ms, 3),
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="f64:4096,f64:65536,f32:65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    model = rbd.load_flat_model(os.path.join(ROOT, "tests", "golden", "models", "atlas_floating.json"))
    for c in a.cases.split(","):
        dt, B = c.split(":")
        res = case(model, torch.float64 if dt == "f64" else torch.float32, int(B), a.iters, a.warmup)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
