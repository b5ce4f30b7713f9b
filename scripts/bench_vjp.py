"""Times the gradient of a scalar loss through dynamics! on Atlas with a floating base, ⟨w, v̇(q, v, τ)⟩ with respect to q, v and τ, three ways:
  (a) rbd_dynamics_vjp (reverse mode: the value route, one solve pair against the kept factor, one adjoint RNEA pass);
  (b) rbd_dynamics_derivatives (the full Jacobians ∂v̇/∂q, ∂v̇/∂v, ∂v̇/∂τ) followed by the Jᵀw products in torch;
  (c) plain rbd_dynamics on the same states (the value alone, for scale).
HIP events around `--iters` calls after `--warmup`; one JSON line per (dtype, batch) on stdout, and with --out the lines appended to that file.
  python scripts/bench_vjp.py [--cases f64:4096,f64:65536,f32:65536] [--iters 10] [--warmup 3] [--out profiles/vjp_bench.jsonl]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import rbd_amd as rbd  # noqa: E402
from bench_derivatives import timed  # noqa: E402


def case(model, dtype, B, iters, warmup):
    nq, nv = model.nq, model.nv
    rng = np.random.default_rng(0)
    q = rbd.rand_configuration(model, B, rng)
    v = rbd.rand_velocity(model, B, rng)
    td = dict(dtype=dtype, device="cuda")
    s = rbd.MechanismState(model, B, dtype=dtype)
    rbd.set_configuration_(s, q)
    rbd.set_velocity_(s, v)
    t = torch.as_tensor(rng.standard_normal((B, nv)), **td)
    w = torch.as_tensor(rng.standard_normal((B, nv)), **td)
    vd = torch.empty((B, nv), **td)
    # (a) reverse mode
    qb, vb, tb = torch.empty((B, nq), **td), torch.empty((B, nv), **td), torch.empty((B, nv), **td)
    a_ms = timed(lambda: rbd.dynamics_vjp_(s, w, t, qb, vb, tb, vdout=vd), iters, warmup)
    a_kernel = rbd.last_kernel(s)
    # (b) the full Jacobians, then Jᵀw per state (bmm on the column-major views)
    Aq, Av, Ai = torch.empty((B, nv * nq), **td), torch.empty((B, nv * nv), **td), torch.empty((B, nv * nv), **td)
    wc = w.unsqueeze(1)

    def jac():
        rbd.dynamics_derivatives_(s, t, Aq, Av, Ai, vdout=vd)
        return [torch.bmm(wc, rbd.jacobian_view(X, s, nv, n)).squeeze(1) for X, n in ((Aq, nq), (Av, nv), (Ai, nv))]
    b_ms = timed(jac, iters, warmup)
    b_kernel = rbd.last_kernel(s)
    gq, gv, gt = jac()
    torch.cuda.synchronize()
    scale = max(float(x.abs().max()) for x in (gq, gv, gt))
    agree = max(float((x - y).abs().max()) for x, y in ((qb, gq), (vb, gv), (tb, gt))) / scale
    # (c) the value alone
    r = rbd.DynamicsResult(model, B, dtype=dtype)
    c_ms = timed(lambda: rbd.dynamics_(r, s, t), iters, warmup)
    return dict(metric="dynamics_vjp", mechanism="atlas_floating", dtype=str(dtype).replace("torch.", ""), B=B, nq=nq, nv=nv,
                a_vjp_ms=round(a_ms, 4), a_kernel=a_kernel, b_jacobians_jtw_ms=round(b_ms, 4), b_kernel=b_kernel, c_dynamics_ms=round(c_ms, 4),
                c_kernel=rbd.last_kernel(s), a_over_b=round(a_ms / b_ms, 3), a_b_rel_diff=float("%.3g" % agree), device=torch.cuda.get_device_name(0))


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
