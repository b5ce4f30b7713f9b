"""Times forward mode through dynamics! with soft contact on Atlas with a floating base, four contact points per foot and one floor (the set-up of
scripts/bench_contact_vjp.py), three ways in one run:
  (a) rbd_dynamics_contact_derivatives with every output: the seven Jacobians, v̇ and ṡ in one call;
  (b) the same Jacobians by rows, the only route before: nv + ns calls of rbd_dynamics_contact_vjp with unit cotangents (each repeats the forward contact
      launch, CRBA and the Cholesky factorisation);
  (c) rbd_dynamics_derivatives on the model WITHOUT contact points, every output: the floor of (a); (a) − (c) is what contact costs in forward mode.
HIP events around `--iters` calls after `--warmup` ((b): one call = the nv + ns VJP calls); (a) and (b) are also compared on the same inputs.  One JSON line per
(dtype, batch) on stdout, and with --out the lines appended to that file.  One run is one sample: the spread between runs is not in the line.
  python scripts/bench_contact_jvp.py [--cases f64:4096,f64:65536,f32:65536] [--iters 20] [--warmup 5] [--out profiles/contact_jvp_bench.jsonl]"""
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
from bench_contact_vjp import with_contact  # noqa: E402
from bench_derivatives import timed  # noqa: E402


def case(bare, dtype, B, iters, warmup):
    flat = with_contact(bare)
    nq, nv, nb, ns, P = flat.nq, flat.nv, flat.n_bodies, flat.ns, len(flat.contact_points)
    rng = np.random.default_rng(0)
    td = dict(dtype=dtype, device="cuda")
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), **td)
    sb = rbd.MechanismState(bare, B, dtype=dtype)  # the model without contact points: (c), and the sole points' heights
    rbd.set_points_(sb, [c["body"] for c in flat.contact_points], [c["location"] for c in flat.contact_points])
    q, v = rbd.rand_configuration(bare, B, rng), rbd.rand_velocity(bare, B, rng)
    # the pelvis height puts the lowest sole point of each state between 3 cm under and 1 cm over the floor
    q[:, 4:7] = 0
    pos = torch.empty((B, 3 * P), **td)
    rbd.point_kinematics_(sb, pos, q=T(q), v=T(v))
    low = pos.double().cpu().numpy().reshape(B, P, 3)[:, :, 2].min(axis=1)
    q[:, 4:7] = (rng.uniform(-0.03, 0.01, B) - low)[:, None] * (bare.pred_rot[0].T @ np.array([0.0, 0.0, 1.0]))
    q, v, s = T(q), T(v), T(1e-3 * rng.standard_normal((B, ns)))
    tau, fext = T(rng.standard_normal((B, nv))), T(rng.standard_normal((B, 6 * nb)))
    sc = rbd.MechanismState(flat, B, dtype=dtype)
    # (a)
    shapes = [(nv, nq), (nv, nv), (nv, ns), (nv, nv), (ns, nq), (ns, nv), (ns, ns)]
    jac = [torch.empty((B, r * c), **td) for r, c in shapes]
    vd, sd = torch.empty((B, nv), **td), torch.empty((B, ns), **td)
    a_ms = timed(lambda: rbd.dynamics_contact_derivatives_(sc, tau, fext, *jac, vdout=vd, sdout=sd, q=q, v=v, s=s), iters, warmup)
    a_kernel = rbd.last_kernel(sc)
    # (b): row i of (∂v̇/∂·) from the cotangent e_i of v̇, row j of (∂ṡ/∂·) from e_j of ṡ
    eye_v, eye_s = torch.eye(nv, **td), torch.eye(ns, **td)
    unit_v = [eye_v[i].expand(B, nv).contiguous() for i in range(nv)]
    unit_s = [eye_s[j].expand(B, ns).contiguous() for j in range(ns)]
    rows = [torch.empty((B, n), **td) for n in (nq, nv, ns, nv)]
    J = [torch.empty((B, c, r), **td) for r, c in shapes]  # (column-major per state, as (a) writes them)

    def by_rows(keep=False):
        for i in range(nv):
            rbd.dynamics_contact_vjp_(sc, unit_v[i], None, None, tau, fext, *rows, q=q, v=v, s=s)
            if keep:
                for k in range(4):
                    J[k][:, :, i] = rows[k]
        for j in range(ns):
            rbd.dynamics_contact_vjp_(sc, None, unit_s[j], None, tau, fext, *rows[:3], q=q, v=v, s=s)
            if keep:
                for k in range(3):
                    J[4 + k][:, :, j] = rows[k]
    b_ms = timed(by_rows, iters, warmup)
    by_rows(keep=True)
    agree = max(float((x.reshape(B, -1) - y).abs().max() / (1 + x.abs().max())) for x, y in zip(J, jac))
    # (c)
    sb.q.copy_(q)
    sb.v.copy_(v)
    jb = [torch.empty((B, r * c), **td) for r, c in (shapes[0], shapes[1], shapes[3])]
    c_ms = timed(lambda: rbd.dynamics_derivatives_(sb, tau, *jb, externalwrenches=fext, vdout=vd), iters, warmup)
    c_kernel = rbd.last_kernel(sb)
    return dict(metric="dynamics_contact_derivatives", mechanism="atlas_floating", contact_points=P, halfspaces=1, dtype=str(dtype).replace("torch.", ""), B=B,
                nq=nq, nv=nv, ns=ns, a_dynamics_contact_derivatives_ms=round(a_ms, 4), a_kernel=a_kernel, b_vjp_rows_ms=round(b_ms, 4), b_vjp_calls=nv + ns,
                c_dynamics_derivatives_bare_ms=round(c_ms, 4), c_kernel=c_kernel, a_over_b=round(a_ms / b_ms, 4), a_minus_c_ms=round(a_ms - c_ms, 4),
                a_vs_b_max_rel_diff=agree, runs=1, iters=iters, warmup=warmup, device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="f64:4096,f64:65536,f32:65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bare = rbd.load_flat_model(os.path.join(ROOT, "tests", "golden", "models", "atlas_floating.json"))
    for c in a.cases.split(","):
        dt, B = c.split(":")
        res = case(bare, torch.float64 if dt == "f64" else torch.float32, int(B), a.iters, a.warmup)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
