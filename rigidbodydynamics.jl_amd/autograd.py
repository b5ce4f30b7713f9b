"""torch.autograd through the library: `tau = inverse_dynamics(state, q, v, vd, fext)`, `vd = dynamics(state, q, v, tau, fext)` and
`q1, v1 = simulate(state, q, v, tau, fext, dt=, nsteps=)`, and, reverse mode only, `pos, vel = point_kinematics(state, q, v)` and
`vd, sd, s_out = dynamics_contact(state, q, v, s, tau, fext)` and `q1, v1, s1 = simulate_contact(state, q, v, s, tau, fext, dt=, nsteps=)` (a mechanism with
contact points) are differentiable functions of their tensor arguments, so `loss.backward()` (reverse mode) and `torch.func.jvp` / `torch.autograd.forward_ad` (forward mode) work through
them.

  - `state` (a MechanismState) supplies the workspace, the batch, the dtype and the layout; q, v, … are tensors of that layout ((B, n) with "aos",
    (n, B) with "soa"); `state.q` / `state.v` are neither read nor written.
  - The forward pass is the library's normal call (rbd_inverse_dynamics / rbd_dynamics), so the value stays on the fast routes.
  - backward is one vector-Jacobian product per call (rbd_inverse_dynamics_vjp / rbd_dynamics_vjp / rbd_simulate_vjp) on the current torch stream;
    forward-mode AD is one JVP with one direction (rbd_inverse_dynamics_jvp / rbd_dynamics_jvp / rbd_simulate_jvp).
  - The derivatives are those of the raw coordinates q (a quaternion joint's unnormalised rotation formula; a SinCosRevolute's (s, c) as two
    coordinates), as every derivative entry point of the library.
  - Double backward is not supported (once_differentiable)."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _capi
from .state import (MechanismState, _ptr, _raise, dynamics_contact_vjp_, dynamics_vjp_, inverse_dynamics_vjp_, point_kinematics_, point_kinematics_vjp_,
                    simulate_contact_vjp_, simulate_vjp_)


def _prep(state: MechanismState, t: Optional[torch.Tensor], n: int, what: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = t.detach().contiguous()
    state._check(t, n, what)
    return t


def _empty(state: MechanismState, n: int, need: bool = True) -> Optional[torch.Tensor]:
    if not need:
        return None
    shape = (state.batch, n) if state.layout == "aos" else (n, state.batch)
    return torch.empty(shape, dtype=state.dtype, device=state.device)


class _InverseDynamics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, q, v, vd, fext):
        f = state.flat
        q, v, vd = _prep(state, q, f.nq, "q"), _prep(state, v, f.nv, "v"), _prep(state, vd, f.nv, "v̇")
        fext = _prep(state, fext, 6 * f.n_bodies, "externalwrenches")
        tau = _empty(state, f.nv)
        state.ws.use_current_stream()
        opts = state._opts()
        _raise(_capi.lib().rbd_inverse_dynamics(state.ws.handle, state.batch, _ptr(q), _ptr(v), _ptr(vd), _ptr(fext), _ptr(tau), ctypes.byref(opts)),
               "rbd_inverse_dynamics")
        ctx.state = state
        ctx.save_for_backward(q, v, vd, fext)
        ctx.save_for_forward(q, v, vd, fext)
        return tau

    @staticmethod
    @once_differentiable
    def backward(ctx, tau_bar):
        state, f = ctx.state, ctx.state.flat
        q, v, vd, fext = ctx.saved_tensors
        _, nq_, nv_, nvd_, nf_ = ctx.needs_input_grad
        out = (_empty(state, f.nq, nq_), _empty(state, f.nv, nv_), _empty(state, f.nv, nvd_), _empty(state, 6 * f.n_bodies, nf_ and fext is not None))
        if any(o is not None for o in out):
            inverse_dynamics_vjp_(state, vd, _prep(state, tau_bar, f.nv, "tau_bar"), *out[:3], externalwrenches=fext, fext_bar=out[3], q=q, v=v)
        return (None,) + out

    @staticmethod
    def jvp(ctx, _dstate, dq, dv, dvd, dfext):
        state, f = ctx.state, ctx.state.flat
        q, v, vd, fext = ctx.saved_tensors
        dq, dv, dvd = _prep(state, dq, f.nq, "dq"), _prep(state, dv, f.nv, "dv"), _prep(state, dvd, f.nv, "dv̇")
        dfext = _prep(state, dfext, 6 * f.n_bodies, "dexternalwrenches") if fext is not None else None
        dtau = _empty(state, f.nv)
        state.ws.use_current_stream()
        opts = state._opts()
        _raise(_capi.lib().rbd_inverse_dynamics_jvp(state.ws.handle, state.batch, 1, _ptr(q), _ptr(v), _ptr(vd), _ptr(fext), _ptr(dq), _ptr(dv), _ptr(dvd),
                                                    _ptr(dfext), None, _ptr(dtau), ctypes.byref(opts)), "rbd_inverse_dynamics_jvp")
        return dtau


class _Dynamics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, q, v, tau, fext, algorithm):
        f = state.flat
        q, v, tau = _prep(state, q, f.nq, "q"), _prep(state, v, f.nv, "v"), _prep(state, tau, f.nv, "torques")
        fext = _prep(state, fext, 6 * f.n_bodies, "externalwrenches")
        vd = _empty(state, f.nv)
        state.ws.use_current_stream()
        opts = state._opts({"aba": _capi.ALGO_ABA, "crba": _capi.ALGO_CRBA_CHOLESKY}[algorithm])
        _raise(_capi.lib().rbd_dynamics(state.ws.handle, state.batch, _ptr(q), _ptr(v), _ptr(tau), _ptr(fext), _ptr(vd), None, None, ctypes.byref(opts)),
               "rbd_dynamics")
        ctx.state = state
        ctx.save_for_backward(q, v, tau, fext)
        ctx.save_for_forward(q, v, tau, fext)
        return vd

    @staticmethod
    @once_differentiable
    def backward(ctx, vd_bar):
        state, f = ctx.state, ctx.state.flat
        q, v, tau, fext = ctx.saved_tensors
        _, nq_, nv_, nt_, nf_, _ = ctx.needs_input_grad
        out = (_empty(state, f.nq, nq_), _empty(state, f.nv, nv_), _empty(state, f.nv, nt_ and tau is not None), _empty(state, 6 * f.n_bodies, nf_ and fext is not None))
        if any(o is not None for o in out):
            dynamics_vjp_(state, _prep(state, vd_bar, f.nv, "vd_bar"), tau, out[0], out[1], out[2], externalwrenches=fext, fext_bar=out[3], q=q, v=v)
        return (None,) + out + (None,)

    @staticmethod
    def jvp(ctx, _dstate, dq, dv, dtau, dfext, _dalgorithm):
        state, f = ctx.state, ctx.state.flat
        q, v, tau, fext = ctx.saved_tensors
        dq, dv = _prep(state, dq, f.nq, "dq"), _prep(state, dv, f.nv, "dv")
        dtau = _prep(state, dtau, f.nv, "dτ") if tau is not None else None
        dfext = _prep(state, dfext, 6 * f.n_bodies, "dexternalwrenches") if fext is not None else None
        dvd = _empty(state, f.nv)
        state.ws.use_current_stream()
        opts = state._opts()
        _raise(_capi.lib().rbd_dynamics_jvp(state.ws.handle, state.batch, 1, _ptr(q), _ptr(v), _ptr(tau), _ptr(fext), _ptr(dq), _ptr(dv), _ptr(dtau),
                                            _ptr(dfext), None, _ptr(dvd), ctypes.byref(opts)), "rbd_dynamics_jvp")
        return dvd


class _Simulate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, q, v, tau, fext, dt, nsteps):
        f = state.flat
        q, v, tau = _prep(state, q, f.nq, "q"), _prep(state, v, f.nv, "v"), _prep(state, tau, f.nv, "torques")
        fext = _prep(state, fext, 6 * f.n_bodies, "externalwrenches")
        q1, v1 = q.clone(), v.clone()
        state.ws.use_current_stream()
        opts = state._opts()
        _raise(_capi.lib().rbd_simulate(state.ws.handle, state.batch, _ptr(q1), _ptr(v1), _ptr(tau), _ptr(fext), ctypes.c_double(dt), int(nsteps),
                                        ctypes.byref(opts)), "rbd_simulate")
        ctx.state, ctx.dt, ctx.nsteps = state, float(dt), int(nsteps)
        ctx.save_for_backward(q, v, tau, fext)
        ctx.save_for_forward(q, v, tau, fext)
        return q1, v1

    @staticmethod
    @once_differentiable
    def backward(ctx, q1_bar, v1_bar):
        state, f = ctx.state, ctx.state.flat
        q, v, tau, fext = ctx.saved_tensors
        _, nq_, nv_, nt_, nf_, _, _ = ctx.needs_input_grad
        if not (nq_ or nv_ or nt_ or nf_):
            return (None,) * 7
        # (the steps run again from the saved inputs, on copies: the library advances q, v in place)
        qs, vs = q.clone(), v.clone()
        qb = _prep(state, q1_bar, f.nq, "q_bar").clone() if q1_bar is not None else torch.zeros_like(q)
        vb = _prep(state, v1_bar, f.nv, "v_bar").clone() if v1_bar is not None else torch.zeros_like(v)
        tb, fb = _empty(state, f.nv, nt_ and tau is not None), _empty(state, 6 * f.n_bodies, nf_ and fext is not None)
        simulate_vjp_(qb, vb, state, ctx.dt, ctx.nsteps, torques=tau, externalwrenches=fext, tau_bar=tb, fext_bar=fb, q=qs, v=vs)
        return None, qb if nq_ else None, vb if nv_ else None, tb, fb, None, None

    @staticmethod
    def jvp(ctx, _dstate, dq, dv, dtau, dfext, _ddt, _dnsteps):
        state, f = ctx.state, ctx.state.flat
        q, v, tau, fext = ctx.saved_tensors
        qs, vs = q.clone(), v.clone()
        dq = _prep(state, dq, f.nq, "dq").clone() if dq is not None else torch.zeros_like(q)
        dv = _prep(state, dv, f.nv, "dv").clone() if dv is not None else torch.zeros_like(v)
        dtau = _prep(state, dtau, f.nv, "dτ") if tau is not None else None
        dfext = _prep(state, dfext, 6 * f.n_bodies, "dexternalwrenches") if fext is not None else None
        state.ws.use_current_stream()
        opts = state._opts()
        _raise(_capi.lib().rbd_simulate_jvp(state.ws.handle, state.batch, 1, _ptr(qs), _ptr(vs), _ptr(tau), _ptr(fext), ctypes.c_double(ctx.dt), ctx.nsteps,
                                            _ptr(dq), _ptr(dv), _ptr(dtau), _ptr(dfext), ctypes.byref(opts)), "rbd_simulate_jvp")
        return dq, dv


class _PointKinematics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, q, v):
        f, P = state.flat, getattr(state, "npoints", 0)
        q, v = _prep(state, q, f.nq, "q"), _prep(state, v, f.nv, "v")
        pos, vel = _empty(state, 3 * P), _empty(state, 3 * P)
        point_kinematics_(state, pos, vel, q=q, v=v)
        ctx.state = state
        ctx.save_for_backward(q, v)
        return pos, vel

    @staticmethod
    @once_differentiable
    def backward(ctx, pos_bar, vel_bar):
        state, f, P = ctx.state, ctx.state.flat, ctx.state.npoints
        q, v = ctx.saved_tensors
        _, nq_, nv_ = ctx.needs_input_grad
        out = (_empty(state, f.nq, nq_), _empty(state, f.nv, nv_))
        if any(o is not None for o in out):
            point_kinematics_vjp_(state, _prep(state, pos_bar, 3 * P, "pos_bar"), _prep(state, vel_bar, 3 * P, "vel_bar"), out[0], out[1], q=q, v=v)
        return (None,) + out

    @staticmethod
    def jvp(ctx, *tangents):
        raise NotImplementedError("point_kinematics: forward-mode AD is not implemented (use the Jacobian output of point_kinematics_)")


class _DynamicsContact(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, q, v, s, tau, fext):
        f = state.flat
        q, v, s = _prep(state, q, f.nq, "q"), _prep(state, v, f.nv, "v"), _prep(state, s, f.ns, "s")
        tau, fext = _prep(state, tau, f.nv, "torques"), _prep(state, fext, 6 * f.n_bodies, "externalwrenches")
        vd, sd, s_out = _empty(state, f.nv), _empty(state, f.ns), s.clone()  # (rbd_dynamics_contact resets the friction state in place: on a copy)
        state.ws.use_current_stream()
        opts = state._opts()
        _raise(_capi.lib().rbd_dynamics_contact(state.ws.handle, state.batch, _ptr(q), _ptr(v), _ptr(s_out), _ptr(tau), _ptr(fext), _ptr(vd), None, _ptr(sd),
                                                None, None, ctypes.byref(opts)), "rbd_dynamics_contact")
        ctx.state = state
        ctx.save_for_backward(q, v, s, tau, fext)
        return vd, sd, s_out

    @staticmethod
    @once_differentiable
    def backward(ctx, vd_bar, sd_bar, s_out_bar):
        state, f = ctx.state, ctx.state.flat
        q, v, s, tau, fext = ctx.saved_tensors
        _, nq_, nv_, ns_, nt_, nf_ = ctx.needs_input_grad
        out = (_empty(state, f.nq, nq_), _empty(state, f.nv, nv_), _empty(state, f.ns, ns_), _empty(state, f.nv, nt_ and tau is not None),
               _empty(state, 6 * f.n_bodies, nf_ and fext is not None))
        if any(o is not None for o in out):
            dynamics_contact_vjp_(state, _prep(state, vd_bar, f.nv, "vd_bar"), _prep(state, sd_bar, f.ns, "sd_bar"), _prep(state, s_out_bar, f.ns, "s_out_bar"),
                                  tau, fext, *out, q=q, v=v, s=s)
        return (None,) + out


class _SimulateContact(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, q, v, s, tau, fext, dt, nsteps):
        f = state.flat
        q, v, s = _prep(state, q, f.nq, "q"), _prep(state, v, f.nv, "v"), _prep(state, s, f.ns, "s")
        tau, fext = _prep(state, tau, f.nv, "torques"), _prep(state, fext, 6 * f.n_bodies, "externalwrenches")
        q1, v1, s1 = q.clone(), v.clone(), s.clone()
        state.ws.use_current_stream()
        opts = state._opts()
        _raise(_capi.lib().rbd_simulate_contact(state.ws.handle, state.batch, _ptr(q1), _ptr(v1), _ptr(s1), _ptr(tau), _ptr(fext), ctypes.c_double(dt),
                                                int(nsteps), ctypes.byref(opts)), "rbd_simulate_contact")
        ctx.state, ctx.dt, ctx.nsteps = state, float(dt), int(nsteps)
        ctx.save_for_backward(q, v, s, tau, fext)
        return q1, v1, s1

    @staticmethod
    @once_differentiable
    def backward(ctx, q1_bar, v1_bar, s1_bar):
        state, f = ctx.state, ctx.state.flat
        q, v, s, tau, fext = ctx.saved_tensors
        _, nq_, nv_, ns_, nt_, nf_, _, _ = ctx.needs_input_grad
        if not (nq_ or nv_ or ns_ or nt_ or nf_):
            return (None,) * 8
        # (the steps run again from the saved inputs, on copies: the library advances q, v, s in place)
        qs, vs, ss = q.clone(), v.clone(), s.clone()
        qb = _prep(state, q1_bar, f.nq, "q_bar").clone() if q1_bar is not None else torch.zeros_like(q)
        vb = _prep(state, v1_bar, f.nv, "v_bar").clone() if v1_bar is not None else torch.zeros_like(v)
        sb = _prep(state, s1_bar, f.ns, "s_bar").clone() if s1_bar is not None else torch.zeros_like(s)
        tb, fb = _empty(state, f.nv, nt_ and tau is not None), _empty(state, 6 * f.n_bodies, nf_ and fext is not None)
        simulate_contact_vjp_(qb, vb, sb, state, ctx.dt, ctx.nsteps, torques=tau, externalwrenches=fext, tau_bar=tb, fext_bar=fb, q=qs, v=vs, s=ss)
        return None, qb if nq_ else None, vb if nv_ else None, sb if ns_ else None, tb, fb, None, None


def simulate_contact(state: MechanismState, q: torch.Tensor, v: torch.Tensor, s: torch.Tensor, tau: Optional[torch.Tensor] = None,
                     fext: Optional[torch.Tensor] = None, dt: float = 1e-3, nsteps: int = 1):
    """(q⁺, v⁺, s⁺) after `nsteps` Munthe-Kaas RK4 steps of `simulate` of a mechanism with contact points and an environment, with the torques `tau` and
    wrenches `fext` held (None: zero / none); `s` (B, ns) is the friction state.  Differentiable in q, v, s, tau and fext, reverse mode only.  The value is
    rbd_simulate_contact's (on copies: q, v and s are not modified); backward runs the steps again from the saved inputs through one
    rbd_simulate_contact_vjp, the derivative of the branch each (point, half-space) pair takes at each stage state, with dynamics! on the CRBA + Cholesky
    route (as `simulate`).  Per-step controls: call this once per step with that step's tau; torch's saved tensors are then the checkpoints."""
    if not float(dt) > 0:
        raise ValueError("dt must be positive")
    if int(nsteps) < 0:
        raise ValueError("nsteps must be non-negative")
    return _SimulateContact.apply(state, q, v, s, tau, fext, float(dt), int(nsteps))


def dynamics_contact(state: MechanismState, q: torch.Tensor, v: torch.Tensor, s: torch.Tensor, tau: Optional[torch.Tensor] = None,
                     fext: Optional[torch.Tensor] = None):
    """(v̇, ṡ, s_out) = dynamics! of a mechanism with contact points and an environment, the ODE form: `s` (B, ns) is the friction state, s_out the same
    after the resets of the points out of contact (`s` itself is not modified).  Differentiable in q, v, s, tau and fext, reverse mode only: backward through
    all three outputs is one rbd_dynamics_contact_vjp, the derivative of the branch each (point, half-space) pair takes (outside, clamped, sticking,
    slipping).  The value is rbd_dynamics_contact's; the derivatives are the CRBA + Cholesky route's, as `dynamics`."""
    return _DynamicsContact.apply(state, q, v, s, tau, fext)


def point_kinematics(state: MechanismState, q: torch.Tensor, v: torch.Tensor):
    """(pos, vel) of the points fixed with `set_points_(state, …)`, each (B, 3P) in the root frame, differentiable in q and v (reverse mode: one
    rbd_point_kinematics_vjp per backward; the points must not be replaced between forward and backward)."""
    return _PointKinematics.apply(state, q, v)


def inverse_dynamics(state: MechanismState, q: torch.Tensor, v: torch.Tensor, vd: torch.Tensor, fext: Optional[torch.Tensor] = None) -> torch.Tensor:
    """τ = inverse_dynamics!(q, v, v̇, f_ext), differentiable in q, v, vd and fext (None: no external wrenches)."""
    return _InverseDynamics.apply(state, q, v, vd, fext)


def dynamics(state: MechanismState, q: torch.Tensor, v: torch.Tensor, tau: Optional[torch.Tensor] = None, fext: Optional[torch.Tensor] = None,
             algorithm: str = "aba") -> torch.Tensor:
    """v̇ = dynamics!(q, v, τ, f_ext), differentiable in q, v, tau and fext (None: zero torques / no external wrenches).  The value is rbd_dynamics's
    (algorithm="aba": the articulated-body route the workspace picks; "crba": the reference's CRBA + Cholesky route).  The derivatives are those of the
    CRBA + Cholesky route of the same function (the implicit-function identity through M(q)), which equal the articulated-body value's to rounding.
    In the raw coordinates OFF the unit sphere of a quaternion (or circle of a SinCosRevolute's (s, c)) the two routes are different functions of q; the
    derivatives there are the CRBA route's, so finite differences of raw q off the sphere match algorithm="crba"."""
    return _Dynamics.apply(state, q, v, tau, fext, algorithm)


def simulate(state: MechanismState, q: torch.Tensor, v: torch.Tensor, tau: Optional[torch.Tensor] = None, fext: Optional[torch.Tensor] = None,
             dt: float = 1e-4, nsteps: int = 1):
    """(q⁺, v⁺) after `nsteps` Munthe-Kaas RK4 steps of `simulate` with the torques `tau` and wrenches `fext` held (None: zero / none), differentiable
    in q, v, tau and fext.  The value is rbd_simulate's (on copies: q and v are not modified); backward runs the steps again from the saved inputs
    through rbd_simulate_vjp, forward-mode AD is one rbd_simulate_jvp direction.  The derivatives are those of the steps with dynamics! on the CRBA +
    Cholesky route at every stage (as `dynamics(..., algorithm="crba")`), which equal the articulated-body value's to rounding on the unit sphere of
    each quaternion; off it, the two routes are different functions of the raw q and finite differences match the CRBA route.
    Per-step controls (backpropagation through time): call this once per step with that step's tau; torch's saved tensors are then the checkpoints."""
    if not float(dt) > 0:
        raise ValueError("dt must be positive")
    if int(nsteps) < 0:
        raise ValueError("nsteps must be non-negative")
    return _Simulate.apply(state, q, v, tau, fext, float(dt), int(nsteps))
