"""Point kinematics on the GPU (rbd_workspace_set_points, rbd_point_kinematics, rbd_point_kinematics_vjp, autograd.point_kinematics): positions, velocities,
accelerations and point Jacobians against the numpy/oracle reference (tests/point_kinematics_ref.py), the reference's own identities
(test/test_mechanism_algorithms.jl:359-369), fp32 against the oracle's own fp32 error, the pullback against Jpᵀ·vel_bar, a 4-point central difference and the
host-compiled routine, gradcheck, and the calls' edge cases."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rand_inputs
from point_kinematics_ref import off_path, pick_points, pos_vel_fd, reference
from test_derivatives_gpu import close, dev, host, make_state, model
from test_point_kinematics_cpu import Emu, build_harness

pytestmark = pytest.mark.gpu

MODELS = ["atlas_floating", "mixed20", "inner_floating", "tree20", "chain70"]  # (chain70: more than 64 bodies)
BATCHES = [67, 1]  # a partial wavefront; a single state
_cache = {}


def case(rbd, oracle, models, name, B):
    """Model, points, inputs and the fp64 reference of one (model, batch): computed once, shared, never modified."""
    key = (name, B)
    if key not in _cache:
        flat = model(rbd, models, name)
        bodies, r = pick_points(flat)
        q, v, _ = rand_inputs(rbd, flat, B, 151)
        vd = np.random.default_rng(15).standard_normal((B, flat.nv))
        ref = reference(oracle, flat, q, v, vd, bodies, r)
        bias = reference(oracle, flat, q, v, None, bodies, r, jac=False)[2]
        for a in ref + (bias,):
            a.setflags(write=False)
        _cache[key] = dict(flat=flat, bodies=bodies, r=r, q=q, v=v, vd=vd, ref=ref, bias=bias)
    return _cache[key]


def nan(s, n):
    shape = (s.batch, n) if s.layout == "aos" else (n, s.batch)
    return torch.full(shape, float("nan"), dtype=s.dtype, device="cuda")


def forward(rbd, s, flat, P, vd=None, which=("pos", "vel", "acc", "jac")):
    """The call with NaN-prefilled outputs; (pos, vel, acc) as (B, P, 3), jac as (B, P, 3, nv), None where not asked for."""
    out = {k: nan(s, 3 * P * (flat.nv if k == "jac" else 1)) if k in which else None for k in ("pos", "vel", "acc", "jac")}
    rbd.point_kinematics_(s, out["pos"], out["vel"], out["acc"], out["jac"], vd=vd)
    res = [None if out[k] is None else host(out[k], s).reshape(s.batch, P, 3) for k in ("pos", "vel", "acc")]
    res.append(None if out["jac"] is None else rbd.point_jacobian_view(out["jac"], s, P, flat.nv).double().cpu().numpy())
    return res


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", MODELS)
def test_fp64_values_and_identities(rbd, oracle, models, name, B, layout):
    c = case(rbd, oracle, models, name, B)
    flat, P = c["flat"], len(c["bodies"])
    s = make_state(rbd, flat, c["q"], c["v"], layout=layout)
    rbd.set_points_(s, c["bodies"], c["r"])
    got = forward(rbd, s, flat, P, vd=dev(c["vd"], s))
    assert rbd.last_kernel(s) == "point_kin_kernel"
    for what, g, x in zip(("pos", "vel", "acc", "jac"), got, c["ref"]):
        assert np.isfinite(g).all(), what  # (NaN-prefilled: fully overwritten)
        close(g, x, 1e-10, what)
    pos, vel, acc, jac = got
    off = off_path(flat, c["bodies"])
    assert (c["ref"][3].transpose(0, 1, 3, 2)[:, off] == 0).all() and (jac.transpose(0, 1, 3, 2)[:, off] == 0).all()  # columns off the path: exactly zero
    bias = forward(rbd, s, flat, P, which=("acc",))[2]
    close(bias, c["bias"], 1e-10, "acc with v̇ = 0")
    # the reference's identities: vel = Jp v, acc(v̇) − acc(0) = Jp v̇
    close(vel, np.einsum("bpiv,bv->bpi", jac, c["v"]), 1e-10, "vel = Jp v")
    close(acc - bias, np.einsum("bpiv,bv->bpi", jac, c["vd"]), 1e-10, "acc(v̇) − acc(0) = Jp v̇")


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_each_output_alone(rbd, oracle, models, layout):
    c = case(rbd, oracle, models, "mixed20", 67)
    flat, P = c["flat"], len(c["bodies"])
    s = make_state(rbd, flat, c["q"], c["v"], layout=layout)
    rbd.set_points_(s, c["bodies"], c["r"])
    full = forward(rbd, s, flat, P, vd=dev(c["vd"], s))
    for k, what in enumerate(("pos", "vel", "acc", "jac")):
        one = forward(rbd, s, flat, P, vd=dev(c["vd"], s), which=(what,))
        assert [x is not None for x in one] == [j == k for j in range(4)]
        assert np.array_equal(one[k], full[k]), what


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("name", MODELS)
def test_fp32_against_the_oracle_in_fp32(rbd, oracle, models, name, layout):
    """No fixed number: the GPU's fp32 error against the fp64 oracle is at most 4 × the error of the oracle run in fp32 on the same (fp32-rounded) inputs, plus
    1e-6 — the factor covers a different summation order."""
    flat = model(rbd, models, name)
    B = 67
    bodies, r = pick_points(flat)
    q, v, _ = rand_inputs(rbd, flat, B, 161)
    vd = np.random.default_rng(16).standard_normal((B, flat.nv))
    q, v, vd, r = (a.astype(np.float32).astype(np.float64) for a in (q, v, vd, r))
    ref64 = reference(oracle, flat, q, v, vd, bodies, r)
    ref32 = reference(oracle, flat, q, v, vd, bodies, r, dtype=np.float32)
    s = make_state(rbd, flat, q, v, dtype=torch.float32, layout=layout)
    rbd.set_points_(s, bodies, r)
    got = forward(rbd, s, flat, len(bodies), vd=dev(vd, s))
    for what, g, x64, x32 in zip(("pos", "vel", "acc", "jac"), got, ref64, ref32):
        e_gpu, e_or = np.abs(g - x64).max(), np.abs(x32.astype(np.float64) - x64).max()
        assert e_gpu <= 4 * e_or + 1e-6, "%s %s %s: GPU fp32 error %.3e, oracle fp32 error %.3e, ratio %.2f" % (name, layout, what, e_gpu, e_or, e_gpu / max(e_or, 1e-30))
        print("fp32 %s %s %s: GPU %.3e oracle %.3e ratio %.2f" % (name, layout, what, e_gpu, e_or, e_gpu / max(e_or, 1e-30)))


@pytest.fixture(scope="module")
def harness():
    return build_harness()


@pytest.mark.parametrize("layout", ["aos", "soa"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", MODELS)
def test_vjp(rbd, oracle, models, harness, name, B, layout):
    """v̄ against Jpᵀ·vel_bar (Jp from the oracle) at 1e-10, q̄ against the 4-point central difference of the numpy/oracle reference along every raw coordinate
    at 1e-8 (two states), and (q̄, v̄) against the host-compiled routine at 1e-12."""
    c = case(rbd, oracle, models, name, B)
    flat, P, q, v = c["flat"], len(c["bodies"]), c["q"], c["v"]
    rng = np.random.default_rng(17)
    pb, wb = rng.standard_normal((B, P, 3)), rng.standard_normal((B, P, 3))
    s = make_state(rbd, flat, q, v, layout=layout)
    rbd.set_points_(s, c["bodies"], c["r"])
    qb, vb = nan(s, flat.nq), nan(s, flat.nv)
    rbd.point_kinematics_vjp_(s, dev(pb.reshape(B, -1), s), dev(wb.reshape(B, -1), s), qb, vb)
    assert rbd.last_kernel(s) == "point_adjoint_kernel"
    qb, vb = host(qb, s), host(vb, s)
    assert np.isfinite(qb).all() and np.isfinite(vb).all()
    close(vb, np.einsum("bpiv,bpi->bv", c["ref"][3], wb), 1e-10, "v̄ = Jpᵀ vel_bar")
    n = min(B, 2)
    bar = np.concatenate([pb.reshape(B, -1), wb.reshape(B, -1)], axis=1)[:n]
    fd = np.zeros((n, flat.nq))
    for j in range(flat.nq):
        dq = np.zeros((n, flat.nq))
        dq[:, j] = 1
        fd[:, j] = np.sum(bar * pos_vel_fd(oracle, flat, q[:n], v[:n], c["bodies"], c["r"], dq, np.zeros((n, flat.nv))), axis=1)
    close(qb[:n], fd, 1e-8, "q̄ against central differences")
    hq, hv = Emu(harness, flat, c["bodies"], c["r"]).vjp(q, v, pb, wb)
    close(qb, hq, 1e-12, "q̄ against the host routine")
    close(vb, hv, 1e-12, "v̄ against the host routine")
    # one cotangent alone: linear in the cotangents
    q1, q2 = nan(s, flat.nq), nan(s, flat.nq)
    rbd.point_kinematics_vjp_(s, dev(pb.reshape(B, -1), s), None, q1)
    rbd.point_kinematics_vjp_(s, None, dev(wb.reshape(B, -1), s), q2)
    close(host(q1, s) + host(q2, s), qb, 1e-12, "q̄ from each cotangent alone")


def test_gradcheck(rbd, models):
    flat = models["mixed20"]
    B = 3
    q, v, _ = rand_inputs(rbd, flat, B, 171)
    s = rbd.MechanismState(flat, B)
    rbd.set_points_(s, *pick_points(flat))
    g = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda *a: rbd.autograd.point_kinematics(s, *a), (g(q), g(v)))


def test_errors_and_empty_batch(rbd, models):
    flat = models["mixed20"]
    B = 8
    q, v, _ = rand_inputs(rbd, flat, B, 181)
    s = make_state(rbd, flat, q, v)
    p = lambda x: rbd.state._ptr(x)
    L, opts = rbd._capi.lib(), s._opts()
    bodies, r = pick_points(flat)
    P = len(bodies)
    pos, qb = nan(s, 3 * P), nan(s, flat.nq)
    # no points set
    assert L.rbd_point_kinematics(s.ws.handle, B, p(s.q), p(s.v), None, p(pos), None, None, None, ctypes.byref(opts)) == 1
    assert L.rbd_point_kinematics_vjp(s.ws.handle, B, p(s.q), p(s.v), p(pos), None, p(qb), None, ctypes.byref(opts)) == 1
    # a body out of range
    for bad in (-1, flat.n_bodies):
        with pytest.raises(ValueError):
            rbd.set_points_(s, [0, bad], np.zeros((2, 3)))
    rbd.set_points_(s, bodies, r)
    # NULL q; vel without v; both cotangents NULL
    assert L.rbd_point_kinematics(s.ws.handle, B, None, p(s.v), None, p(pos), None, None, None, ctypes.byref(opts)) == 1
    assert L.rbd_point_kinematics(s.ws.handle, B, p(s.q), None, None, None, p(pos), None, None, ctypes.byref(opts)) == 1
    assert L.rbd_point_kinematics_vjp(s.ws.handle, B, None, p(s.v), p(pos), None, p(qb), None, ctypes.byref(opts)) == 1
    assert L.rbd_point_kinematics_vjp(s.ws.handle, B, p(s.q), p(s.v), None, None, p(qb), None, ctypes.byref(opts)) == 1
    # the VJP takes device pointers only
    hopts = rbd._capi.Opts(rbd._capi.LAYOUT_AOS, rbd._capi.MEM_HOST, 0, 1)
    assert L.rbd_point_kinematics_vjp(s.ws.handle, B, p(s.q), p(s.v), p(pos), None, p(qb), None, ctypes.byref(hopts)) == 3
    # B == 0: a successful no-op
    assert L.rbd_point_kinematics(s.ws.handle, 0, p(s.q), p(s.v), None, p(pos), None, None, None, ctypes.byref(opts)) == 0
    assert L.rbd_point_kinematics_vjp(s.ws.handle, 0, p(s.q), p(s.v), p(pos), None, p(qb), None, ctypes.byref(opts)) == 0
    torch.cuda.synchronize()
    assert torch.isnan(pos).all() and torch.isnan(qb).all()
    with pytest.raises(rbd.DimensionMismatch):  # shapes are checked before any launch
        rbd.point_kinematics_(s, pos=torch.zeros((B, 3 * P + 1), dtype=torch.float64, device="cuda"))
    # cleared points
    rbd.set_points_(s, [], np.zeros((0, 3)))
    assert L.rbd_point_kinematics(s.ws.handle, B, p(s.q), p(s.v), None, p(pos), None, None, None, ctypes.byref(opts)) == 1
    # loop joints
    fb = models["four_bar"]
    s4 = make_state(rbd, fb, *rand_inputs(rbd, fb, 2, 182)[:2])
    with pytest.raises(RuntimeError, match="tree Mechanisms"):
        rbd.set_points_(s4, [0], np.zeros((1, 3)))


def test_host_memory(rbd, oracle, models):
    """RBD_MEM_HOST as rbd_geometric_jacobian: host arrays in, host arrays out after rbd_sync."""
    c = case(rbd, oracle, models, "mixed20", 67)
    flat, P, B = c["flat"], len(c["bodies"]), 67
    s = rbd.MechanismState(flat, B)
    rbd.set_points_(s, c["bodies"], c["r"])
    hopts = rbd._capi.Opts(rbd._capi.LAYOUT_AOS, rbd._capi.MEM_HOST, 0, 1)
    q, v = np.ascontiguousarray(c["q"]), np.ascontiguousarray(c["v"])
    pos, jac = np.full((B, P, 3), np.nan), np.full((B, P, flat.nv, 3), np.nan)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert rbd._capi.lib().rbd_point_kinematics(s.ws.handle, B, hp(q), hp(v), None, hp(pos), None, None, hp(jac), ctypes.byref(hopts)) == 0
    assert rbd.sync(s) == 0
    close(pos, c["ref"][0], 1e-10, "pos")
    close(jac.transpose(0, 1, 3, 2), c["ref"][3], 1e-10, "jac")


def test_later_calls_allocate_nothing_and_points_can_be_replaced(rbd, oracle, models):
    c = case(rbd, oracle, models, "atlas_floating", 67)
    flat, B = c["flat"], 67
    s = make_state(rbd, flat, c["q"], c["v"])
    bodies, r = c["bodies"], c["r"]
    P = len(bodies)
    rbd.set_points_(s, bodies, r)
    outs = [nan(s, 3 * P), nan(s, 3 * P), nan(s, 3 * P), nan(s, 3 * P * flat.nv)]
    qb, vb, bar, vd = nan(s, flat.nq), nan(s, flat.nv), torch.ones_like(outs[0]), torch.zeros_like(s.v)  # (every tensor of the test made before the measurement)
    rbd.point_kinematics_(s, *outs, vd=vd)
    rbd.point_kinematics_vjp_(s, bar, bar, qb, vb)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(2):
        rbd.point_kinematics_(s, *outs, vd=vd)
        rbd.point_kinematics_vjp_(s, bar, bar, qb, vb)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0
    # other points, another P
    rbd.set_points_(s, bodies[:2], r[:2])
    got = forward(rbd, s, flat, 2, vd=dev(c["vd"], s))
    for what, g, x in zip(("pos", "vel", "acc", "jac"), got, c["ref"]):
        close(g, x[:, :2], 1e-10, what)
    rbd.point_kinematics_vjp_(s, bar[:, :6].contiguous(), None, qb, vb)
    assert torch.isfinite(qb).all()


@pytest.mark.parametrize("layout", ["aos", "soa"])
def test_batch_isolation(rbd, oracle, models, layout):
    """One NaN state leaves every other state's outputs bitwise unchanged."""
    c = case(rbd, oracle, models, "atlas_floating", 67)
    flat, B, P = c["flat"], 67, len(c["bodies"])
    rng = np.random.default_rng(19)
    bar = rng.standard_normal((B, 3 * P))

    def run(q):
        s = make_state(rbd, flat, q, c["v"], layout=layout)
        rbd.set_points_(s, c["bodies"], c["r"])
        out = forward(rbd, s, flat, P, vd=dev(c["vd"], s))
        qb, vb = nan(s, flat.nq), nan(s, flat.nv)
        rbd.point_kinematics_vjp_(s, dev(bar, s), dev(bar, s), qb, vb)
        return out + [host(qb, s), host(vb, s)]

    clean = run(c["q"])
    bad = c["q"].copy()
    bad[5] = np.nan
    dirty = run(bad)
    keep = np.arange(B) != 5
    for a, b in zip(clean, dirty):
        assert np.array_equal(a[keep], b[keep])
    assert all(np.isnan(b[5]).any() for b in dirty[:4])
