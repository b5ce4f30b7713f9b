"""Times the step Jacobians of `simulate` (rbd_simulate_step_derivatives: ∂x⁺/∂x and ∂x⁺/∂τ, x = (q; v)) on Atlas with a floating base against what a user
has without them: central finite differences through rbd_simulate, i.e. ONE rbd_simulate step of the B·2(nq + 2nv) perturbed states (the cheapest form),
and one plain rbd_simulate step of the B states.  Also reports the ratio to rbd_dynamics_derivatives at the same batch (the cost model of DESIGN §3.8).
HIP events around `--iters` calls after `--warmup`; one JSON line per (dtype, batch) on stdout, and with --out the lines appended to that file.
  python scripts/bench_simulate_derivatives.py [--cases f64:4096,f64:65536,f32:65536] [--iters 5] [--warmup 2] [--out profiles/simulate_derivatives_bench.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rbd_amd as rbd  # noqa: E402

DT = 1e-3


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def state(model, q, v, dtype):
    s = rbd.MechanismState(model, q.shape[0], dtype=dtype)
    rbd.set_configuration_(s, q)
    rbd.set_velocity_(s, v)
    return s


def case(model, dtype, B, iters, warmup):
    nq, nv = model.nq, model.nv
    nx = nq + nv
    rng = np.random.default_rng(0)
    q = rbd.rand_configuration(model, B, rng)
    v = rbd.rand_velocity(model, B, rng)
    tau = rng.standard_normal((B, nv))
    td = dict(dtype=dtype, device="cuda")
    t = torch.as_tensor(tau, **td)
    # (a) the step Jacobians (each call advances the state: the timing is that of a rollout's linearisation)
    s = state(model, q, v, dtype)
    A, Bt = torch.empty((B, nx * nx), **td), torch.empty((B, nx * nv), **td)
    a_ms = timed(lambda: rbd.simulate_step_derivatives_(s, DT, torques=t, dx_dx=A, dx_dtau=Bt), iters, warmup)
    kernel = rbd.last_kernel(s)
    # the dynamics! Jacobians at the same batch: the issue's cost model (4 stages × (nq + 2nv)/(nq + nv))
    s2 = state(model, q, v, dtype)
    Aq, Av, Ai = torch.empty((B, nv * nq), **td), torch.empty((B, nv * nv), **td), torch.empty((B, nv * nv), **td)
    d_ms = timed(lambda: rbd.dynamics_derivatives_(s2, t, Aq, Av, Ai), iters, warmup)
    del s2, Aq, Av, Ai
    # (b) central finite differences: every state perturbed by ±h along the nq + nv coordinates of x and the nv of τ, one rbd_simulate step for all
    per = 2 * (nq + 2 * nv)
    nfd = B * per
    sf = state(model, np.repeat(q, per, axis=0), np.repeat(v, per, axis=0), dtype)
    tf = torch.as_tensor(np.repeat(tau, per, axis=0), **td)
    b_ms = timed(lambda: rbd.simulate_(sf, DT / 2, dt=DT, torques=tf), iters, warmup)
    fd_kernel = rbd.last_kernel(sf)
    del sf, tf
    # (c) one plain step
    s3 = state(model, q, v, dtype)
    c_ms = timed(lambda: rbd.simulate_(s3, DT / 2, dt=DT, torques=t), iters, warmup)
    return dict(metric="simulate_step_derivatives", mechanism="atlas_floating", dtype=str(dtype).replace("torch.", ""), B=B, nq=nq, nv=nv,
                a_step_jacobians_ms=round(a_ms, 4), a_kernel=kernel, b_fd_simulate_ms=round(b_ms, 4), b_states=nfd, b_kernel=fd_kernel,
                c_simulate_ms=round(c_ms, 4), c_kernel=rbd.last_kernel(s3), a_over_b=round(a_ms / b_ms, 3),
                dynamics_derivatives_ms=round(d_ms, 4), a_over_dynamics_derivatives=round(a_ms / d_ms, 2), device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="f64:4096,f64:65536,f32:65536")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
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
