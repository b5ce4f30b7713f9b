"""Point kinematics without a GPU (rbd_workspace_set_points, rbd_point_kinematics, rbd_point_kinematics_vjp): the three calls are declared and exported; the
per-(point, state) routine of the forward kernel and the per-state routine of the pullback's kernel (csrc/rbd_point.hpp point_kin_state, point_adjoint_state),
compiled as plain C++ for the host as tests/test_vjp_cpu.py does, against the numpy/oracle reference (tests/point_kinematics_ref.py); the pullback against J·d
from the Dual<double, 1> instantiation of the forward routine; that instantiation against a 4-point central difference of the reference in raw q; and the path
and union tables of rbd_workspace_set_points (csrc/rbd_point_plan.hpp)."""
import ctypes
import os

import numpy as np
import pytest

from host_harness import CLANG, ROOT, build
from point_kinematics_ref import off_path, pick_points, pos_vel_fd, reference
from test_derivatives_cpu import tables

NEW = ("rbd_workspace_set_points", "rbd_point_kinematics", "rbd_point_kinematics_vjp")
MODELS = ["randmech1", "randmech2", "randmech3", "inner_floating", "mixed20", "double_pendulum"]

HARNESS = r"""
#include <hip/hip_runtime.h>
#include "rbd_point.hpp"
#include "rbd_point_plan.hpp"
thread_local EmuDim3 threadIdx, blockIdx, blockDim, gridDim;
int emu_unreachable(const char*) { __builtin_trap(); return 0; }
using namespace rbd;
// sizes first (out == nullptr), then the tables back to back: poff (np + 1), path, uni, ubeg (nu + 1), upts (np)
extern "C" void emu_point_plan(int nb, const int* parent, int np, const int* body, int* npath, int* nu, int* out) {
  const PointPlanTables T = point_plan(nb, parent, np, body);
  *npath = (int)T.path.size(); *nu = (int)T.uni.size();
  if (!out) return;
  for (const std::vector<int32_t>* v : {&T.poff, &T.path, &T.uni, &T.ubeg, &T.upts})
    for (int32_t x : *v) *out++ = x;
}
// state-major (AOS) buffers, one (point, state) after the other
extern "C" void emu_point_kin(int nb, int nq, int nv, const int* tbl, const double* rb, long B, int np, const int* poff, const int* path, const double* r,
                              const double* q, const double* v, const double* vd, double* pos, double* vel, double* acc, double* jac) {
  BigModel M{nb, nq, nv, 0, tbl, rb, {0, 0, 0}};
  for (int pt = 0; pt < np; ++pt)
    for (long st = 0; st < B; ++st) {
      double* J = jac + (st * np + pt) * 3 * nv;
      for (int e = 0; e < 3 * nv; ++e) J[e] = 0;
      double* o = pos + (st * np + pt) * 3;
      point_kin_state<double>(M, path + poff[pt], poff[pt + 1] - poff[pt], r + 3 * pt, true, true, [&](int k) { return q[st * nq + k]; },
                              [&](int k) { return v[st * nv + k]; }, [&](int k) { return vd ? vd[st * nv + k] : 0.0; },
                              [&](int col, int c, double x) { J[3 * col + c] = x; }, o, vel + (o - pos), acc + (o - pos));
    }
}
// J·d of (pos, vel) for one direction (dq, dv) per state: the Dual<double, 1> instantiation of the same routine
extern "C" void emu_point_jvp(int nb, int nq, int nv, const int* tbl, const double* rb, long B, int np, const int* poff, const int* path, const double* r,
                              const double* q, const double* v, const double* dq, const double* dv, double* dpos, double* dvel) {
  using D = Dual<double, 1>;
  BigModel M{nb, nq, nv, 0, tbl, rb, {0, 0, 0}};
  auto dual = [](double x, double d) { D y(x); y.d[0] = d; return y; };
  for (int pt = 0; pt < np; ++pt)
    for (long st = 0; st < B; ++st) {
      const D rr[3] = {D(r[3 * pt]), D(r[3 * pt + 1]), D(r[3 * pt + 2])};
      D pos[3], vel[3], acc[3];
      point_kin_state<D>(M, path + poff[pt], poff[pt + 1] - poff[pt], rr, true, false, [&](int k) { return dual(q[st * nq + k], dq[st * nq + k]); },
                         [&](int k) { return dual(v[st * nv + k], dv[st * nv + k]); }, [&](int k) { return D(0.0); }, [&](int, int, D) {}, pos, vel, acc);
      for (int k = 0; k < 3; ++k) { dpos[(st * np + pt) * 3 + k] = pos[k].d[0]; dvel[(st * np + pt) * 3 + k] = vel[k].d[0]; }
    }
}
extern "C" void emu_point_vjp(int nb, int nq, int nv, const int* tbl, const double* rb, long B, int np, int nu, const int* poff, const int* path, const int* uni,
                              const int* ubeg, const int* upts, const double* r, const double* q, const double* v, const double* pos_bar, const double* vel_bar,
                              double* qbar, double* vbar) {
  BigModel M{nb, nq, nv, 0, tbl, rb, {0, 0, 0}};
  PointPlan P{np, nu, poff, path, uni, ubeg, upts, r};
  AdjArgs<double> A{};
  A.B = B; A.q = q; A.v = v; A.Lq = Layout{1, nq}; A.Lv = A.Llam = Layout{1, nv}; A.Lf = Layout{1, 6L * nb};
  A.qbar = qbar; A.vbar = vbar; A.sign = 1.0;
  PointAdjArgs<double> C{pos_bar, vel_bar, Layout{1, 3L * np}};
  double* sc = new double[(size_t)ADJ_FIELDS * nb];
  for (long st = 0; st < B; ++st) {
    for (size_t k = 0; k < (size_t)ADJ_FIELDS * nb; ++k) sc[k] = __builtin_nan("");  // (what the routine does not write it must not use)
    point_adjoint_state<double>(M, P, A, C, st, sc, 1, 0);
  }
  delete[] sc;
}
"""


def build_harness():
    return build(HARNESS, "rbd_point_emu")


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(CLANG):
        pytest.skip("no ROCm clang")
    return build_harness()


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def plan(lib, flat, bodies):
    """(poff, path, uni, ubeg, upts) of the library's plan routine."""
    parent = np.ascontiguousarray(flat.parent, dtype=np.int32)
    bodies = np.ascontiguousarray(bodies, dtype=np.int32)
    npath, nu = ctypes.c_int(), ctypes.c_int()
    head = (ctypes.c_int(flat.n_bodies), _p(parent), ctypes.c_int(len(bodies)), _p(bodies), ctypes.byref(npath), ctypes.byref(nu))
    lib.emu_point_plan(*head, None)
    P = len(bodies)
    out = np.full(P + 1 + npath.value + nu.value + nu.value + 1 + P, -7, dtype=np.int32)
    lib.emu_point_plan(*head, _p(out))
    cuts = np.cumsum([P + 1, npath.value, nu.value, nu.value + 1])
    return [np.ascontiguousarray(x) for x in np.split(out, cuts)]


class Emu:
    def __init__(self, lib, flat, bodies, r):
        self.lib, self.flat, self.P = lib, flat, len(bodies)
        self.tbl, self.rb = tables(flat)
        self.poff, self.path, self.uni, self.ubeg, self.upts = plan(lib, flat, bodies)
        self.r = _c(np.asarray(r).reshape(-1))
        self.head = [ctypes.c_int(flat.n_bodies), ctypes.c_int(flat.nq), ctypes.c_int(flat.nv), _p(self.tbl), _p(self.rb)]

    def forward(self, q, v, vd):
        B, P, nv = q.shape[0], self.P, self.flat.nv
        q, v, vd = _c(q), _c(v), _c(vd)
        pos, vel, acc, jac = np.full((B, P, 3), np.nan), np.full((B, P, 3), np.nan), np.full((B, P, 3), np.nan), np.full((B, P, nv, 3), np.nan)
        self.lib.emu_point_kin(*self.head, ctypes.c_long(B), ctypes.c_int(P), _p(self.poff), _p(self.path), _p(self.r), _p(q), _p(v), _p(vd),
                               _p(pos), _p(vel), _p(acc), _p(jac))
        return pos, vel, acc, jac.transpose(0, 1, 3, 2)

    def jvp(self, q, v, dq, dv):
        B, P = q.shape[0], self.P
        q, v, dq, dv = _c(q), _c(v), _c(dq), _c(dv)
        dpos, dvel = np.full((B, P, 3), np.nan), np.full((B, P, 3), np.nan)
        self.lib.emu_point_jvp(*self.head, ctypes.c_long(B), ctypes.c_int(P), _p(self.poff), _p(self.path), _p(self.r), _p(q), _p(v), _p(dq), _p(dv),
                               _p(dpos), _p(dvel))
        return dpos, dvel

    def vjp(self, q, v, pos_bar, vel_bar):
        B, P, f = q.shape[0], self.P, self.flat
        q, v, pos_bar, vel_bar = _c(q), _c(v), _c(pos_bar), _c(vel_bar)
        qb, vb = np.full((B, f.nq), np.nan), np.full((B, f.nv), np.nan)
        self.lib.emu_point_vjp(*self.head, ctypes.c_long(B), ctypes.c_int(P), ctypes.c_int(len(self.uni)), _p(self.poff), _p(self.path), _p(self.uni),
                               _p(self.ubeg), _p(self.upts), _p(self.r), _p(q), _p(v), _p(pos_bar), _p(vel_bar), _p(qb), _p(vb))
        return qb, vb


def inputs(rbd, flat, B, seed):
    rng = np.random.default_rng(seed)
    return rng, rbd.rand_configuration(flat, B, rng), rbd.rand_velocity(flat, B, rng), rng.standard_normal((B, flat.nv))


def test_symbols_declared_and_exported(rbd):
    header = open(os.path.join(ROOT, "include", "rbd_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in rbd._capi.SYMBOLS, name
    lib = ctypes.CDLL(rbd._capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("name", MODELS)
def test_values_against_the_oracle(harness, models, oracle, rbd, name):
    """pos, vel, acc (with v̇ and with v̇ = 0) and the point Jacobians at 1e-12·(1 + |ref|); Jacobian columns off the path exactly zero."""
    flat = models[name]
    B = 4
    bodies, r = pick_points(flat)
    rng, q, v, vd = inputs(rbd, flat, B, 31)
    emu = Emu(harness, flat, bodies, r)
    for a in (vd, None):
        got = emu.forward(q, v, a)
        ref = reference(oracle, flat, q, v, a, bodies, r)
        for what, g, x in zip(("pos", "vel", "acc", "jac"), got, ref):
            assert np.abs(g - x).max() <= 1e-12 * (1 + np.abs(x).max()), (name, what, np.abs(g - x).max())
        assert (got[3].transpose(0, 1, 3, 2)[:, off_path(flat, bodies)] == 0).all()


@pytest.mark.parametrize("name", MODELS)
def test_adjoint_is_the_transpose_of_the_dual_forward(harness, models, rbd, name):
    """⟨(pos_bar, vel_bar), J d⟩ = ⟨q̄, dq⟩ + ⟨v̄, dv⟩ per state to 1e-12 of the terms' magnitude; dq is not projected on any quaternion's sphere; each
    cotangent alone (the other NULL) too."""
    flat = models[name]
    B = 5
    bodies, r = pick_points(flat)
    rng, q, v, _ = inputs(rbd, flat, B, 37)
    emu = Emu(harness, flat, bodies, r)
    P = len(bodies)
    pb, wb = rng.standard_normal((B, P, 3)), rng.standard_normal((B, P, 3))
    for pbar, vbar in ((pb, wb), (pb, None), (None, wb)):
        qb, vb = emu.vjp(q, v, pbar, vbar)
        assert np.isfinite(qb).all() and np.isfinite(vb).all()
        for trial in range(3):
            dq, dv = rng.standard_normal((B, flat.nq)), rng.standard_normal((B, flat.nv))
            if trial == 1:
                dv[:] = 0
            if trial == 2:
                dq[:] = 0
            dpos, dvel = emu.jvp(q, v, dq, dv)
            left = [t for t in ((None if pbar is None else pbar * dpos), (None if vbar is None else vbar * dvel)) if t is not None]
            terms = [qb * dq, vb * dv]
            lhs = sum(t.reshape(B, -1).sum(axis=1) for t in left)
            rhs = sum(t.sum(axis=1) for t in terms)
            mag = sum(np.abs(t).reshape(B, -1).sum(axis=1) for t in left + terms) + 1e-300
            assert (np.abs(lhs - rhs) <= 1e-12 * mag).all(), (name, trial, np.abs(lhs - rhs) / mag)


@pytest.mark.parametrize("name", MODELS)
def test_dual_forward_against_central_differences(harness, models, oracle, rbd, name):
    """J·d from the Dual instantiation against the 4-point central difference (h = 1e-3) of the numpy/oracle reference in raw q, at 1e-8·(1 + |ref|): rounding
    is about eps/h ≈ 1e-13, truncation about h⁴/30."""
    flat = models[name]
    B = 3
    bodies, r = pick_points(flat)
    rng, q, v, _ = inputs(rbd, flat, B, 41)
    emu = Emu(harness, flat, bodies, r)
    for trial in range(2):
        dq, dv = rng.standard_normal((B, flat.nq)), rng.standard_normal((B, flat.nv))
        dpos, dvel = emu.jvp(q, v, dq, dv)
        got = np.concatenate([dpos.reshape(B, -1), dvel.reshape(B, -1)], axis=1)
        ref = pos_vel_fd(oracle, flat, q, v, bodies, r, dq, dv)
        assert np.abs(got - ref).max() <= 1e-8 * (1 + np.abs(ref).max()), (name, trial, np.abs(got - ref).max())


def test_plan_tables(harness, models):
    """Points on a leaf, on a child of the world, on a body below an inner floating joint, and two points on one body."""
    flat = models["inner_floating"]  # a chain: Revolute, Prismatic, QuaternionFloating, Revolute, QuaternionSpherical, Planar, QuaternionFloating, Revolute
    parent = [int(p) for p in flat.parent]
    n = flat.n_bodies
    leaf = [b for b in range(n) if b not in parent][0]
    top = parent.index(-1)
    below = 3  # the body of the revolute joint under the first inner floating joint
    bodies = [leaf, top, below, below]
    poff, path, uni, ubeg, upts = plan(harness, flat, bodies)
    chain = lambda b: ([] if b < 0 else chain(parent[b]) + [b])
    want = [chain(b) for b in bodies]
    assert list(poff) == list(np.cumsum([0] + [len(c) for c in want]))
    assert list(path) == sum(want, [])
    assert list(uni) == sorted(set(sum(want, [])))
    assert all(parent[b] < 0 or list(uni).index(parent[b]) < k for k, b in enumerate(uni))  # parents first
    pts = {b: [k for k, x in enumerate(bodies) if x == b] for b in uni}
    assert [list(upts[ubeg[k]:ubeg[k + 1]]) for k in range(len(uni))] == [pts[b] for b in uni]
    assert pts[below] == [2, 3] and len(upts) == len(bodies)
    # a branching tree: the union is shared between paths, bodies off every path are left out
    tree = models["randmech1"]
    tp = [int(p) for p in tree.parent]
    b2 = [tree.n_bodies - 1, tp.index(-1)]
    poff, path, uni, ubeg, upts = plan(harness, tree, b2)
    on = set()
    for b in b2:
        while b >= 0:
            on.add(b)
            b = tp[b]
    assert list(uni) == sorted(on) and list(path[poff[1]:poff[2]]) == [b2[1]]
