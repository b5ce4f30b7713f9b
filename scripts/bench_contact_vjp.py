"""Times reverse mode through dynamics! with soft contact on Atlas with a floating base, four contact points per foot and one floor, three ways in one run:
  (a) rbd_dynamics_contact_vjp: (v̇̄, ṡ̄, s̄_out) -> (q̄, v̄, s̄, τ̄, f̄ext) in one call;
  (b) what a caller could compose before: autograd.point_kinematics on the model WITHOUT its contact points (the points set with set_points_), the pair model
      written in torch (tests/contact_model_ref.py), autograd.dynamics at fext + contactwrenches, and backward() — forward and backward together, as (a)
      also evaluates the forward pass;
  (c) rbd_dynamics_vjp on the model without contact points: the floor of (a); (a) − (c) is what contact costs.
HIP events around `--iters` calls after `--warmup`; one JSON line per (dtype, batch) on stdout, and with --out the lines appended to that file.
  python scripts/bench_contact_vjp.py [--cases f64:4096,f64:65536,f32:65536] [--iters 20] [--warmup 5] [--out profiles/contact_vjp_bench.jsonl]"""
import argparse
import copy
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
from bench_derivatives import timed  # noqa: E402
import contact_model_ref as cm  # noqa: E402

FEET = ("l_foot", "r_foot")
SOLE = [(x, y, -0.08) for x in (0.17, -0.08) for y in (0.06, -0.06)]


def with_contact(bare):
    hc = rbd.hunt_crossley_hertz()
    par = dict(hc_k=hc.k, hc_lambda=hc.lam, hc_n=hc.n, mu=0.8, k=20e3, b=100.0)
    m = copy.copy(bare)
    m.contact_points = [dict(par, body=list(bare.body_names).index(f), location=np.array(r)) for f in FEET for r in SOLE]
    m.halfspaces = [dict(point=np.zeros(3), outward_normal=np.array([0.0, 0.0, 1.0]))]
    m.ns = 3 * len(m.contact_points) * len(m.halfspaces)
    m._c = None
    m.__dict__.pop("_rbd_model", None)  # (the library's model cached on the copied object is the one without contact points)
    return m


def case(bare, dtype, B, iters, warmup):
    flat = with_contact(bare)
    nq, nv, nb, ns, P = flat.nq, flat.nv, flat.n_bodies, flat.ns, len(flat.contact_points)
    rng = np.random.default_rng(0)
    td = dict(dtype=dtype, device="cuda")
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), **td)
    sb = rbd.MechanismState(bare, B, dtype=dtype)  # the model without contact points, the contact points set as points: (b) and (c)
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
    a, b, c = T(rng.standard_normal((B, nv))), T(rng.standard_normal((B, ns))), T(rng.standard_normal((B, ns)))
    # (a)
    sc = rbd.MechanismState(flat, B, dtype=dtype)
    out = [torch.empty((B, n), **td) for n in (nq, nv, ns, nv, 6 * nb)]
    a_ms = timed(lambda: rbd.dynamics_contact_vjp_(sc, a, b, c, tau, fext, *out, q=q, v=v, s=s), iters, warmup)
    a_kernel = rbd.last_kernel(sc)
    # (b)
    tab = cm.tables(flat, dtype, "cuda")
    leaves = [x.clone().requires_grad_(True) for x in (q, v, s, tau, fext)]

    def composed():
        for x in leaves:
            x.grad = None
        qq, vv, ss, tt, ff = leaves
        p, w = rbd.autograd.point_kinematics(sb, qq, vv)
        cw, sd, s_out, info = cm.contact_model(flat, p, w, ss, tab)
        vd = rbd.autograd.dynamics(sb, qq, vv, tt, ff + cw)
        ((vd * a).sum() + (sd * b).sum() + (s_out * c).sum()).backward()
    b_ms = timed(composed, iters, warmup)
    inside = float(cm.contact_model(flat, *rbd.autograd.point_kinematics(sb, q, v), s, tab)[3]["inside"].double().mean())
    agree = max(float((x.grad - o).abs().max() / (1 + x.grad.abs().max())) for x, o in zip(leaves, out))
    # (c)
    c_ms = timed(lambda: rbd.dynamics_vjp_(sb, a, tau, out[0], out[1], out[3], externalwrenches=fext, fext_bar=out[4], q=q, v=v), iters, warmup)
    c_kernel = rbd.last_kernel(sb)
    return dict(metric="dynamics_contact_vjp", mechanism="atlas_floating", contact_points=P, halfspaces=1, pairs_inside=round(inside, 3),
                dtype=str(dtype).replace("torch.", ""), B=B, nq=nq, nv=nv, a_dynamics_contact_vjp_ms=round(a_ms, 4), a_kernel=a_kernel,
                b_composed_ms=round(b_ms, 4), c_dynamics_vjp_bare_ms=round(c_ms, 4), c_kernel=c_kernel, a_over_b=round(a_ms / b_ms, 3),
                a_minus_c_ms=round(a_ms - c_ms, 4), a_vs_b_max_rel_diff=agree, device=torch.cuda.get_device_name(0))


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
