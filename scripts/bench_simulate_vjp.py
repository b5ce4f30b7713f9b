"""Times reverse mode through `simulate` steps (rbd_simulate_vjp) on Atlas with a floating base: the gradient of ⟨w, x⁺⟩ in (q, v, τ), x = (q; v), against
what a user has without it — the step Jacobians [A B] of rbd_simulate_step_derivatives followed by [A B]ᵀw — at the same batch, and for `--nsteps` steps
against as many one-step VJPs (the checkpoints fitting).  HIP events around `--iters` calls after `--warmup`; one JSON line per (dtype, batch) on stdout,
and with --out the lines appended to that file.  --no-jacobians skips the comparison (for a kernel-trace run of the VJP alone).
  python scripts/bench_simulate_vjp.py [--cases f64:4096,f64:65536,f32:65536] [--nsteps 10] [--iters 5] [--warmup 2] [--out profiles/simulate_vjp_bench.jsonl]"""
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


def case(model, dtype, B, nsteps, iters, warmup, jacobians):
    nq, nv = model.nq, model.nv
    nx = nq + nv
    rng = np.random.default_rng(0)
    q = rbd.rand_configuration(model, B, rng)
    v = rbd.rand_velocity(model, B, rng)
    td = dict(dtype=dtype, device="cuda")
    t = torch.as_tensor(rng.standard_normal((B, nv)), **td)
    w = torch.as_tensor(rng.standard_normal((B, nx)), **td)
    wq, wv = w[:, :nq].contiguous(), w[:, nq:].contiguous()
    qb, vb, tb = torch.empty_like(wq), torch.empty_like(wv), torch.empty((B, nv), **td)

    def vjp(s, n):
        qb.copy_(wq)
        vb.copy_(wv)
        rbd.simulate_vjp_(qb, vb, s, DT, n, torques=t, tau_bar=tb)

    # (a) one step's VJP (each call advances the state, as a rollout's would)
    s = state(model, q, v, dtype)
    a_ms = timed(lambda: vjp(s, 1), iters, warmup)
    kernel = rbd.last_kernel(s)
    # (c) nsteps steps in one call against nsteps one-step calls
    s = state(model, q, v, dtype)
    c_ms = timed(lambda: vjp(s, nsteps), iters, warmup)
    res = dict(metric="simulate_vjp", mechanism="atlas_floating", dtype=str(dtype).replace("torch.", ""), B=B, nq=nq, nv=nv,
               a_vjp_one_step_ms=round(a_ms, 4), a_kernel=kernel, c_nsteps=nsteps, c_vjp_nsteps_ms=round(c_ms, 4),
               c_over_nsteps_one_step=round(c_ms / (nsteps * a_ms), 3))
    if jacobians:
        # (b) the step Jacobians and [A B]ᵀ w
        s = state(model, q, v, dtype)
        A, Bt = torch.empty((B, nx * nx), **td), torch.empty((B, nx * nv), **td)

        def jac():
            rbd.simulate_step_derivatives_(s, DT, torques=t, dx_dx=A, dx_dtau=Bt)
            torch.bmm(w.unsqueeze(1), rbd.jacobian_view(A, s, nx, nx))
            torch.bmm(w.unsqueeze(1), rbd.jacobian_view(Bt, s, nx, nv))

        b_ms = timed(jac, iters, warmup)
        del A, Bt
        res.update(b_step_jacobians_and_product_ms=round(b_ms, 4), a_over_b=round(a_ms / b_ms, 4))
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="f64:4096,f64:65536,f32:65536")
    ap.add_argument("--nsteps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-jacobians", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    model = rbd.load_flat_model(os.path.join(ROOT, "tests", "golden", "models", "atlas_floating.json"))
    for c in a.cases.split(","):
        dt, B = c.split(":")
        res = case(model, torch.float64 if dt == "f64" else torch.float32, int(B), a.nsteps, a.iters, a.warmup, not a.no_jacobians)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
