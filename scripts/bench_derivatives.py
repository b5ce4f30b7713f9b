"""Times the full Jacobians of dynamics! (rbd_dynamics_derivatives: ∂v̇/∂q, ∂v̇/∂v, ∂v̇/∂τ) on Atlas with a floating base against what a user has without
them: central finite differences through rbd_dynamics, i.e. ONE rbd_dynamics call on the B·2(nq + nv) perturbed states (the cheapest form), and plain
rbd_dynamics on the B states.  HIP events around `--iters` calls after `--warmup`; one JSON line per (dtype, batch) on stdout, and with --out the lines
appended to that file.
  python scripts/bench_derivatives.py [--cases f64:4096,f64:65536,f32:65536] [--iters 10] [--warmup 3] [--out profiles/derivatives_bench.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rbd_amd as rbd  # noqa: E402


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


def case(model, dtype, B, iters, warmup):
    nq, nv = model.nq, model.nv
    rng = np.random.default_rng(0)
    q = rbd.rand_configuration(model, B, rng)
    v = rbd.rand_velocity(model, B, rng)
    tau = rng.standard_normal((B, nv))
    td = dict(dtype=dtype, device="cuda")
    s = rbd.MechanismState(model, B, dtype=dtype)
    rbd.set_configuration_(s, q)
    rbd.set_velocity_(s, v)
    t = torch.as_tensor(tau, **td)
    Aq, Av, Ai = torch.empty((B, nv * nq), **td), torch.empty((B, nv * nv), **td), torch.empty((B, nv * nv), **td)
    vd = torch.empty((B, nv), **td)
    a_ms = timed(lambda: rbd.dynamics_derivatives_(s, t, Aq, Av, Ai, vdout=vd), iters, warmup)
    kernel = rbd.last_kernel(s)
    # (b) the finite-difference alternative: every state perturbed by ±h along each of the nq + nv coordinates of (q, v) — ∂v̇/∂τ = M⁻¹ would need nv more
    #     pairs, or a solve; left out, in (b)'s favour
    nfd = B * 2 * (nq + nv)
    sf = rbd.MechanismState(model, nfd, dtype=dtype)
    rf = rbd.DynamicsResult(model, nfd, dtype=dtype)
    rbd.set_configuration_(sf, np.repeat(q, 2 * (nq + nv), axis=0))
    rbd.set_velocity_(sf, np.repeat(v, 2 * (nq + nv), axis=0))
    tf = torch.as_tensor(np.repeat(tau, 2 * (nq + nv), axis=0), **td)
    b_ms = timed(lambda: rbd.dynamics_(rf, sf, tf), iters, warmup)
    fd_kernel = rbd.last_kernel(sf)
    del sf, rf, tf
    r = rbd.DynamicsResult(model, B, dtype=dtype)
    c_ms = timed(lambda: rbd.dynamics_(r, s, t), iters, warmup)
    return dict(metric="dynamics_derivatives", mechanism="atlas_floating", dtype=str(dtype).replace("torch.", ""), B=B, nq=nq, nv=nv,
                a_derivatives_ms=round(a_ms, 4), a_kernel=kernel, b_fd_dynamics_ms=round(b_ms, 4), b_states=nfd, b_kernel=fd_kernel,
                c_dynamics_ms=round(c_ms, 4), c_kernel=rbd.last_kernel(s), a_over_b=round(a_ms / b_ms, 3), device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="f64:4096,f64:65536,f32:65536")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
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
