"""Writes tests/golden/vectors/simulate_contact_parent.npz — what rbd_simulate_contact and rbd_dynamics_contact computed BEFORE rbd_simulate_contact was folded
into the stage of rbd_simulate_contact_controlled and the contact kinematics moved from rnea_kernel's export to contact_head_kernel's.

Run by hand on a GPU, never by a test, against a library built from the commit before the fold (commit 35d23ba), handed in through RBD_LIB:
    OUT=librbd_hip_parent.so rigidbodydynamics.jl_amd/csrc/build.sh          (in a checkout of that commit)
    RBD_LIB=<that .so> python tests/golden/make_simulate_contact_parent.py
tests/test_simulate_contact_controlled_gpu.py then holds the folded code to these results: the old stage (contact_stage_kernel + rnea_kernel + contact_kernel)
stays the yardstick although it is gone from the tree.

Inputs: simulate_contact_controlled_ref.walker_case (B = 130, 3 steps, dt = 1e-3); layout AOS; the kernels built with the library (RBD_JIT=0, as the tests run).
Recorded: every second state (65 of 130); fp32 results as float32; a SHA-256 of the input arrays' bytes instead of the inputs (input_hash below — the tests
assert it before they compare, so a change to walker_case cannot silently compare different problems).
  sim_f64_{q,v,s}          final state of rbd_simulate_contact, fp64, fext given
  sim_f32_{q,v,s}          the same in fp32
  sim_f32_nofext_{q,v,s}   fp32 without fext
  dyn_f64_{vdot,sdot}      one rbd_dynamics_contact call on the same (q, v, s, tau, fext), fp64
  dyn_f32_{vdot,sdot}      the same in fp32
"""
import ctypes
import hashlib
import os
import sys

os.environ["RBD_JIT"] = "0"

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
OUT = os.path.join(HERE, "vectors", "simulate_contact_parent.npz")
EVERY = 2  # the recorded states: [::EVERY]
INPUTS = ("q", "v", "s", "tau", "fext")


def input_hash(w):
    """SHA-256 over the bytes of the walker's input arrays (C-contiguous float64, in the order of INPUTS)"""
    h = hashlib.sha256()
    for k in INPUTS:
        h.update(np.ascontiguousarray(w[k], dtype=np.float64).tobytes())
    return h.hexdigest()


def main():
    import torch
    import rbd_amd as rbd
    import simulate_contact_controlled_ref as ref
    assert os.environ.get("RBD_LIB"), "RBD_LIB: the library built from the commit before the fold"
    w = ref.walker_case(rbd)
    flat, B = w["flat"], w["B"]
    L = rbd._capi.lib()
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    out = dict(input_hash=np.array(input_hash(w)), every=np.array(EVERY), library=np.array("rbd_simulate_contact / rbd_dynamics_contact of commit 35d23ba"),
               device=np.array(torch.cuda.get_device_name(0)))
    for name, dtype, fext in (("f64", torch.float64, True), ("f32", torch.float32, True), ("f32_nofext", torch.float32, False)):
        D = lambda k: torch.as_tensor(w[k], dtype=dtype).cuda()
        st = rbd.MechanismState(flat, B, dtype=dtype)
        q, v, s, tau, fe = D("q"), D("v"), D("s"), D("tau"), D("fext") if fext else None
        assert L.rbd_simulate_contact(st.ws.handle, B, ptr(q), ptr(v), ptr(s), ptr(tau), ptr(fe), ctypes.c_double(ref.DT), w["nsteps"], ctypes.byref(st._opts())) == 0
        assert rbd.sync(st) == 0
        print("sim_" + name, rbd.last_kernel(st))
        for k, x in zip("qvs", (q, v, s)):
            out["sim_%s_%s" % (name, k)] = x.cpu().numpy()[::EVERY]
        if fext:
            q, v, s = D("q"), D("v"), D("s")
            vd, sd = torch.empty_like(v), torch.empty_like(s)
            assert L.rbd_dynamics_contact(st.ws.handle, B, ptr(q), ptr(v), ptr(s), ptr(tau), ptr(fe), ptr(vd), None, ptr(sd), None, None, ctypes.byref(st._opts())) == 0
            assert rbd.sync(st) == 0
            print("dyn_" + name, rbd.last_kernel(st))
            out["dyn_%s_vdot" % name], out["dyn_%s_sdot" % name] = vd.cpu().numpy()[::EVERY], sd.cpu().numpy()[::EVERY]
    assert all(np.isfinite(x).all() for x in out.values() if x.dtype.kind == "f")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
