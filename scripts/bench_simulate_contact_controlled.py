"""Times `simulate` with soft contact under a device-side controller on Atlas with a floating base, four contact points per foot and one floor (the set-up of
scripts/bench_contact_vjp.py), per step of a `--steps`-step call, four ways in one run — and (e) one rbd_dynamics_contact call on the same inputs, per call:
  (a) rbd_simulate_contact_controlled with RBD_CONTROL_CONSTANT: the stage of contact_head_kernel + contact_sim_kernel;
  (b) the same with RBD_CONTROL_PD (feed-forward, q_des, small gains on every 1-dof joint);
  (c) rbd_simulate_contact on the same inputs: the constant kind of (a) behind its own entry point, so the same stage — it ran a stage of its own
      (a kernel for s + rnea_kernel + contact_kernel) until the two were folded; the leg stays as the measurement of rbd_simulate_contact against a library
      built from an earlier commit (RBD_LIB);
  (d) rbd_simulate of the mechanism without contact points: what contact costs on top.
Every call starts from the same state (copied in before the call, inside the timed region of all four).  HIP events around `--iters` calls after `--warmup`;
the four are timed in turn, `--repeats` rounds, and the median with the lowest and highest round is recorded: a difference inside that spread is not one.
One JSON line per (dtype, batch) on stdout, and with --out the lines appended to that file.
  python scripts/bench_simulate_contact_controlled.py [--cases f64:4096,f64:65536,f32:65536] [--steps 10] [--iters 20] [--warmup 5] [--repeats 5]
                                                      [--out profiles/simulate_contact_controlled_bench.jsonl]"""
import argparse
import ctypes
import json
import os
import statistics
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

DT = 1e-3


def case(bare, dtype, B, steps, iters, warmup, repeats):
    flat = with_contact(bare)
    nq, nv, nb, ns, P = flat.nq, flat.nv, flat.n_bodies, flat.ns, len(flat.contact_points)
    rng = np.random.default_rng(0)
    td = dict(dtype=dtype, device="cuda")
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), **td)
    sb = rbd.MechanismState(bare, B, dtype=dtype)  # the model without contact points: (d), and the contact points' positions below
    rbd.set_points_(sb, [c["body"] for c in flat.contact_points], [c["location"] for c in flat.contact_points])
    q, v = rbd.rand_configuration(bare, B, rng), rbd.rand_velocity(bare, B, rng)
    # the pelvis height puts the lowest sole point of each state between 3 cm under and 1 cm over the floor
    q[:, 4:7] = 0
    pos = torch.empty((B, 3 * P), **td)
    rbd.point_kinematics_(sb, pos, q=T(q), v=T(v))
    low = pos.double().cpu().numpy().reshape(B, P, 3)[:, :, 2].min(axis=1)
    q[:, 4:7] = (rng.uniform(-0.03, 0.01, B) - low)[:, None] * (bare.pred_rot[0].T @ np.array([0.0, 0.0, 1.0]))
    q_des = T(q + 0.3 * rng.standard_normal((B, nq)))
    q, v, s = T(q), T(v), T(1e-3 * rng.standard_normal((B, ns)))
    tau, fext = T(rng.standard_normal((B, nv))), T(rng.standard_normal((B, 6 * nb)))
    kp, kd = T(2 * rng.random(nv)), T(0.02 * rng.random(nv))  # (the gains of the tests: the wrist links have 4e-4 kg m² about their axes)
    sc = rbd.MechanismState(flat, B, dtype=dtype)
    work = [torch.empty_like(x) for x in (q, v, s)]
    L, C = rbd._capi.lib(), rbd._capi
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    const, pd = C.Control(), C.Control()
    const.kind, const.tau = C.CONTROL_CONSTANT, tau.data_ptr()
    pd.kind, pd.tau, pd.q_des, pd.kp, pd.kd = C.CONTROL_PD, tau.data_ptr(), q_des.data_ptr(), kp.data_ptr(), kd.data_ptr()
    oc, ob = sc._opts(), sb._opts()
    sc.ws.use_current_stream(); sb.ws.use_current_stream()

    def start(n):
        for w, x in zip(work[:n], (q, v, s)):
            w.copy_(x)

    def controlled(ctl):
        def f():
            start(3)
            C.check(L.rbd_simulate_contact_controlled(sc.ws.handle, B, p(work[0]), p(work[1]), p(work[2]), ctypes.byref(ctl), p(fext), ctypes.c_double(DT), steps,
                                                      ctypes.byref(oc)), "rbd_simulate_contact_controlled")
        return f

    def contact():
        start(3)
        C.check(L.rbd_simulate_contact(sc.ws.handle, B, p(work[0]), p(work[1]), p(work[2]), p(tau), p(fext), ctypes.c_double(DT), steps, ctypes.byref(oc)),
                "rbd_simulate_contact")

    def bare_sim():
        start(2)
        C.check(L.rbd_simulate(sb.ws.handle, B, p(work[0]), p(work[1]), p(tau), p(fext), ctypes.c_double(DT), steps, ctypes.byref(ob)), "rbd_simulate")

    vd, sd = torch.empty_like(v), torch.empty_like(s)

    def dynamics_contact():
        start(3)
        C.check(L.rbd_dynamics_contact(sc.ws.handle, B, p(work[0]), p(work[1]), p(work[2]), p(tau), p(fext), p(vd), None, p(sd), None, None, ctypes.byref(oc)),
                "rbd_dynamics_contact")

    legs = dict(a=controlled(const), b=controlled(pd), c=contact, d=bare_sim, e=dynamics_contact)
    state_of = lambda: [x.clone() for x in work]
    legs["a"](); a_out, a_kernel = state_of(), rbd.last_kernel(sc)
    legs["b"](); b_kernel = rbd.last_kernel(sc)
    legs["c"](); c_out, c_kernel = state_of(), rbd.last_kernel(sc)
    legs["d"](); d_kernel = rbd.last_kernel(sb)
    agree = max(float((x - y).abs().max() / (1 + y.abs().max())) for x, y in zip(a_out, c_out))
    ms = {k: [] for k in legs}
    for r in range(repeats):
        for k in legs:
            ms[k].append(timed(legs[k], iters, warmup if r == 0 else 1) / (1 if k == "e" else steps))
    fig = lambda k: dict(median=round(statistics.median(ms[k]), 4), low=round(min(ms[k]), 4), high=round(max(ms[k]), 4))
    names = dict(a="a_controlled_constant", b="b_controlled_pd", c="c_simulate_contact", d="d_simulate_bare", e="e_dynamics_contact")
    out = dict(metric="simulate_contact_controlled", mechanism="atlas_floating", contact_points=P, halfspaces=1, dtype=str(dtype).replace("torch.", ""), B=B, nq=nq,
               nv=nv, ns=ns, steps=steps, dt=DT, iters=iters, repeats=repeats)
    for k in legs:
        out[names[k] + ("_ms_per_call" if k == "e" else "_ms_per_step")] = fig(k)
    med = lambda k: statistics.median(ms[k])
    out.update(a_kernel=a_kernel, b_kernel=b_kernel, c_kernel=c_kernel, d_kernel=d_kernel, a_over_c=round(med("a") / med("c"), 3), b_over_c=round(med("b") / med("c"), 3),
               a_minus_d_ms_per_step=round(med("a") - med("d"), 4), a_vs_c_max_rel_diff=agree, device=torch.cuda.get_device_name(0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="f64:4096,f64:65536,f32:65536")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bare = rbd.load_flat_model(os.path.join(ROOT, "tests", "golden", "models", "atlas_floating.json"))
    for c in a.cases.split(","):
        dt, B = c.split(":")
        res = case(bare, torch.float64 if dt == "f64" else torch.float32, int(B), a.steps, a.iters, a.warmup, a.repeats)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
