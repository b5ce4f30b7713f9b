"""Times reverse mode through `simulate` steps with soft contact on Atlas with a floating base, four contact points per foot and one floor (the set-up of
scripts/bench_contact_vjp.py), per step of a `--steps`-step call, three ways in one run:
  (a) rbd_simulate_contact_vjp: the cotangent of the final (q, v, s) -> (q̄, v̄, s̄, τ̄, f̄ext) in one call;
  (b) what a caller could compose before: the Munthe-Kaas RK4 step written in torch (tests/simulate_contact_ref.py) around autograd.dynamics_contact,
      forward and backward() together, as (a) also runs the forward pass;
  (c) rbd_simulate_vjp on the model without contact points: the floor of (a); (a) − (c) is what contact costs.
Every call starts from the same state (copied in before the call, inside the timed region of all three).  HIP events around `--iters` calls after `--warmup`;
one JSON line per (dtype, batch) on stdout, and with --out the lines appended to that file.
  python scripts/bench_simulate_contact_vjp.py [--cases f64:4096,f64:65536,f32:65536] [--steps 10] [--iters 20] [--warmup 5]
                                               [--out profiles/simulate_contact_vjp_bench.jsonl]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rbd_amd as rbd  # noqa: E402
from bench_contact_vjp import with_contact  # noqa: E402
from bench_derivatives import timed  # noqa: E402
import simulate_contact_ref as sr  # noqa: E402

DT = 1e-3


def case(bare, dtype, B, steps, iters, warmup):
    flat = with_contact(bare)
    nq, nv, nb, ns, P = flat.nq, flat.nv, flat.n_bodies, flat.ns, len(flat.contact_points)
    rng = np.random.default_rng(0)
    td = dict(dtype=dtype, device="cuda")
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), **td)
    sb = rbd.MechanismState(bare, B, dtype=dtype)  # the model without contact points: (c), and the contact points' positions below
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
    cot = [T(rng.standard_normal((B, n))) for n in (nq, nv, ns)]
    # (a)
    sc = rbd.MechanismState(flat, B, dtype=dtype)
    work = [torch.empty_like(x) for x in (q, v, s)]
    bars = [torch.empty_like(x) for x in cot]
    tb, fb = torch.empty((B, nv), **td), torch.empty((B, 6 * nb), **td)

    def fused():
        for w, x in zip(work + bars, [q, v, s] + cot):
            w.copy_(x)
        rbd.simulate_contact_vjp_(*bars, sc, DT, steps, torques=tau, externalwrenches=fext, tau_bar=tb, fext_bar=fb, q=work[0], v=work[1], s=work[2])
    a_ms = timed(fused, iters, warmup)
    a_kernel = rbd.last_kernel(sc)
    a_out = [x.clone() for x in bars + [tb, fb]]
    # (b)
    leaves = [x.clone().requires_grad_(True) for x in (q, v, s, tau, fext)]

    def composed():
        for x in leaves:
            x.grad = None
        qq, vv, ss, tt, ff = leaves
        q1, v1, s1, _ = sr.rollout(flat, qq, vv, ss, DT, steps, lambda x, y, z: rbd.autograd.dynamics_contact(sc, x, y, z, tt, ff)[:2] + (None,))
        ((q1 * cot[0]).sum() + (v1 * cot[1]).sum() + (s1 * cot[2]).sum()).backward()
    b_ms = timed(composed, iters, warmup)
    agree = max(float((x.grad - o).abs().max() / (1 + x.grad.abs().max())) for x, o in zip(leaves, a_out))
    # (c)
    def floor():
        for w, x in zip(work[:2] + bars[:2], [q, v] + cot[:2]):
            w.copy_(x)
        rbd.simulate_vjp_(bars[0], bars[1], sb, DT, steps, torques=tau, externalwrenches=fext, tau_bar=tb, fext_bar=fb, q=work[0], v=work[1])
    c_ms = timed(floor, iters, warmup)
    c_kernel = rbd.last_kernel(sb)
    per = lambda ms: round(ms / steps, 4)
    return dict(metric="simulate_contact_vjp", mechanism="atlas_floating", contact_points=P, halfspaces=1, dtype=str(dtype).replace("torch.", ""), B=B, nq=nq,
                nv=nv, ns=ns, steps=steps, dt=DT, a_simulate_contact_vjp_ms_per_step=per(a_ms), a_kernel=a_kernel, b_composed_ms_per_step=per(b_ms),
                c_simulate_vjp_bare_ms_per_step=per(c_ms), c_kernel=c_kernel, a_over_b=round(a_ms / b_ms, 3), a_minus_c_ms_per_step=per(a_ms - c_ms),
                a_vs_b_max_rel_diff=agree, device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="f64:4096,f64:65536,f32:65536")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bare = rbd.load_flat_model(os.path.join(ROOT, "tests", "golden", "models", "atlas_floating.json"))
    for c in a.cases.split(","):
        dt, B = c.split(":")
        res = case(bare, torch.float64 if dt == "f64" else torch.float32, int(B), a.steps, a.iters, a.warmup)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
