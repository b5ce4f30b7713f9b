"""Times the step Jacobians of `simulate` with soft contact (A = ∂x⁺/∂x, B = ∂x⁺/∂τ, x = (q; v; s)) on Atlas with a floating base, four contact points per
foot and one floor (the set-up of scripts/bench_contact_vjp.py), three ways in one run:
  (a) rbd_simulate_contact_step_derivatives with both outputs: one call;
  (b) the same Jacobians by rows, the only route before: nx = nq + nv + ns one-step calls of rbd_simulate_contact_vjp with unit cotangents of (q⁺; v⁺; s⁺)
      (each repeats the four forward contact launches, four CRBA + Cholesky and four adjoint passes);
  (c) rbd_simulate_step_derivatives on the model WITHOUT contact points, both outputs: the floor of (a); (a) − (c) is what contact costs.
Every call starts from the same state (three small copies before it, in all three routes).  HIP events around `--iters` calls after `--warmup` ((b): one call =
the nx VJP calls); (a) and (b) are also compared on the same inputs.  One JSON line per (dtype, batch) on stdout, and with --out the lines appended to that
file.  One run is one sample: the spread between runs is not in the line.
  python scripts/bench_simulate_contact_jvp.py [--cases f64:4096,f64:65536,f32:65536] [--iters 20] [--warmup 5] [--out profiles/simulate_contact_jvp_bench.jsonl]"""
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


def case(bare, dtype, B, iters, warmup, dt):
    flat = with_contact(bare)
    nq, nv, nb, ns, P = flat.nq, flat.nv, flat.n_bodies, flat.ns, len(flat.contact_points)
    nx = nq + nv + ns
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
    q0, v0, s0 = T(q), T(v), T(1e-3 * rng.standard_normal((B, ns)))
    tau, fext = T(rng.standard_normal((B, nv))), T(rng.standard_normal((B, 6 * nb)))
    q, v, s = q0.clone(), v0.clone(), s0.clone()

    def start():
        q.copy_(q0)
        v.copy_(v0)
        s.copy_(s0)
    sc = rbd.MechanismState(flat, B, dtype=dtype)
    # (a)
    A, Bt = torch.empty((B, nx * nx), **td), torch.empty((B, nx * nv), **td)

    def forward():
        start()
        rbd.simulate_contact_step_derivatives_(sc, dt, tau, A, Bt, fext, q=q, v=v, s=s)
    a_ms = timed(forward, iters, warmup)
    a_kernel = rbd.last_kernel(sc)
    # (b): row i of [A B] from the cotangent e_i of (q⁺; v⁺; s⁺)
    eye = torch.eye(nx, **td)
    cot = [torch.empty((B, n), **td) for n in (nq, nv, ns)]
    tb = torch.empty((B, nv), **td)
    Ar, Br = torch.empty((B, nx, nx), **td), torch.empty((B, nv, nx), **td)  # (column-major per state, as (a) writes them)

    def by_rows(keep=False):
        for i in range(nx):
            start()
            for c, (c0, c1) in zip(cot, ((0, nq), (nq, nq + nv), (nq + nv, nx))):
                c.copy_(eye[i, c0:c1].expand(B, c1 - c0))
            rbd.simulate_contact_vjp_(*cot, sc, dt, 1, torques=tau, externalwrenches=fext, tau_bar=tb, q=q, v=v, s=s)
            if keep:
                Ar[:, :, i] = torch.cat(cot, dim=1)
                Br[:, :, i] = tb
    b_ms = timed(by_rows, iters, warmup)
    by_rows(keep=True)
    forward()
    agree = max(float((x.reshape(B, -1) - y).abs().max() / (1 + x.abs().max())) for x, y in ((Ar, A), (Br, Bt)))
    # (c)
    n2 = nq + nv
    Ab, Bb = torch.empty((B, n2 * n2), **td), torch.empty((B, n2 * nv), **td)

    def bare_step():
        sb.q.copy_(q0)
        sb.v.copy_(v0)
        s.copy_(s0)  # (the third copy of the other routes)
        rbd.simulate_step_derivatives_(sb, dt, tau, Ab, Bb, fext)
    c_ms = timed(bare_step, iters, warmup)
    c_kernel = rbd.last_kernel(sb)
    return dict(metric="simulate_contact_step_derivatives", mechanism="atlas_floating", contact_points=P, halfspaces=1, dtype=str(dtype).replace("torch.", ""),
                B=B, dt=dt, nq=nq, nv=nv, ns=ns, nx=nx, a_simulate_contact_step_derivatives_ms=round(a_ms, 4), a_kernel=a_kernel,
                b_vjp_rows_ms=round(b_ms, 4), b_vjp_calls=nx, c_simulate_step_derivatives_bare_ms=round(c_ms, 4), c_kernel=c_kernel,
                a_over_b=round(a_ms / b_ms, 4), a_minus_c_ms=round(a_ms - c_ms, 4), a_vs_b_max_rel_diff=agree, runs=1, iters=iters, warmup=warmup,
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="f64:4096,f64:65536,f32:65536")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bare = rbd.load_flat_model(os.path.join(ROOT, "tests", "golden", "models", "atlas_floating.json"))
    for c in a.cases.split(","):
        dt, B = c.split(":")
        res = case(bare, torch.float64 if dt == "f64" else torch.float32, int(B), a.iters, a.warmup, a.dt)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
