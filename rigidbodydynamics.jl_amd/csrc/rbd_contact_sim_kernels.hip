// rbd_contact_sim_kernels.hip — the per-body kinematics every contact route of a tree of at most 64 bodies reads, and the stage of `simulate` with contact
// points (rbd_simulate_contact, rbd_simulate_contact_controlled: src/simulate.jl:36-55 — control! runs before every stage's dynamics!, which begins with
// contact_dynamics!, src/mechanism_algorithms.jl:845-864).
//
// Between launch_mk_stage, which leaves the stage state in (q, v), and the forward-dynamics launch the stage needs three things: the controller's τ on the stage
// state, the per-body kinematics the contact model reads, and the friction state s taken through the Runge–Kutta tableau, evaluated and reset.  Two kernels:
//
// contact_head_kernel: one lane per (state, body) like rnea_kernel — the top-down kinematics sweep only (transforms to root and twists), exported as
//   [state][body][24] (R, p, twist; slots 18 … 23, where rnea_kernel's export has accelerations, are not written: contact_kernel, contact_sim_kernel and the
//   adjoint contact kernels read 0 … 17), and, for RBD_CONTROL_PD, pd_control_lane's law on the lane's joint into the τ buffer of the stage.  No accelerations,
//   no Newton–Euler wrench, no bottom-up sweep, no bias torque.  Besides the simulate stage it serves run_contact_kinematics (rbd_capi.hip) with
//   tau_out = nullptr: rbd_contact_dynamics, rbd_dynamics_contact and the forward contact launches of the contact derivative drivers.
// contact_sim_kernel: one thread per state like contact_kernel — the tableau for s folded into contact_kernel's walk over the (point, half-space) pairs:
//   each pair's three values of s are advanced from (s0, acc, the previous stage's ṡ), the pair model (rbd_contact.hpp contact_pair_wrench: contact_kernel's)
//   is evaluated on them, ṡ and the reset s are written and the wrench is added into totalwrenches = fext + contact.  Stage 4 only closes s.
//   The tableau (runge_kutta_4, src/ode_integrators.jl:48-55: a = 1/2, 1/2, 1; b = 1/6, 1/3, 1/3, 1/6), stage by stage like mk_stage_kernel does (q, v):
//     stage 0: s0 = s, acc = 0;  stage k = 1 … 3: acc += b_k ṡ_k, s = s0 + a_{k+1,k} dt ṡ_k;  stage 4: s = s0 + dt (acc + b_4 ṡ_4).
#include "rbd_device.hpp"
#include "rbd_internal.hpp"
#include "rbd_lane.hpp"
#include "rbd_contact.hpp"

namespace rbd {

template <typename T>
__global__ __launch_bounds__(256) void contact_head_kernel(DevModel M, long B, const T* __restrict__ q, const T* __restrict__ v, const T* __restrict__ tau_ff,
                                                          MkFuse F, T* __restrict__ tau_out, T* __restrict__ body_out, Layout Lq, Layout Lv) {
  Body<T> b;
  load_body(M, B, b);
  const T* rb = reinterpret_cast<const T*>(M.rb) + (b.sub < M.nb ? b.sub : 0) * RB_STRIDE;
  T qj[7], vj[6];
  load_joint_q(b, q, Lq, qj);
  load_joint_v(b, v, Lv, vj);
  if (tau_out != nullptr) {  // uniform: RBD_CONTROL_PD — the stage's τ for every velocity coordinate of the lane's joint (feed-forward, or zero without one)
    T tj[6];
    load_joint_v(b, tau_ff, Lv, tj);
    pd_control_lane(b, F, Lq, qj, vj, tj);
    store_joint_v(b, tau_out, Lv, tj);
  }
  T XR[9], Xp[3], R[9], p[3], tl[6], Tw[6], vJ[6];
  local_transform(b, rb, qj, XR, Xp);
  local_joint_motion(b, rb, vj, tl);
  sweep_kinematics<T, false>(M, b, XR, Xp, R, p, tl, Tw, vJ, nullptr, nullptr);
  if (b.valid) {
    T* o = body_out + (b.state * M.nb + b.orig) * 24;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[9 + k] = p[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) o[12 + k] = Tw[k];
  }
}

// stage 0 … 3: s0, acc, sdot in the call's layout Ls, like s; `sdot` holds the previous stage's ṡ on entry and this stage's on
// return.  stage 4: s = s0 + dt (acc + b_4 ṡ_4), one thread per VALUE of s; nothing else is touched (body, fext, tw are not read).
template <typename T>
__global__ __launch_bounds__(256) void contact_sim_kernel(ContactModel M, long B, int stage, T dt, const T* __restrict__ body, T* __restrict__ s,
                                                         T* __restrict__ sdot, T* __restrict__ s0, T* __restrict__ acc, const T* __restrict__ fext,
                                                         T* __restrict__ tw, Layout Ls, Layout Lf) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const T bk = (stage == 1 || stage == 4) ? T(1) / T(6) : T(1) / T(3);  // b of the stage whose ṡ comes in
  if (stage == 4) {  // uniform.  Element-wise over the ns·B values (the launcher sizes the grid for it): the four buffers share a layout
    if (b >= 3L * M.np * M.nh * B) return;
    const T a = acc[b] + bk * sdot[b];
    s[b] = s0[b] + dt * a;
    return;
  }
  if (b >= B) return;
  const T* cp = reinterpret_cast<const T*>(M.cp);
  const T* hs = reinterpret_cast<const T*>(M.hs);
  const long bs = b * Ls.sb;
  // totalwrenches = wext for every body; the points then add their wrenches (a thread owns its state's columns)
  for (int j = 0; j < 6 * M.nb; ++j) {
    const long o = (long)j * Lf.sk + b * Lf.sb;
    tw[o] = fext ? fext[o] : T(0);
  }
  for (int ip = 0; ip < M.np; ++ip) {
    const int body_i = M.cbody[ip];
    const T* k = body + (b * M.nb + body_i) * 24;
    const T* c = cp + (long)ip * CP_STRIDE;
    T w[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    T pt[3], vel[3];
    contact_point_in_root(k, c, pt, vel);
    for (int h = 0; h < M.nh; ++h) {
      const long so = (long)(ip * M.nh + h) * 3;
      T x[3], xd[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const long o = (so + j) * Ls.sk + bs;
        if (stage == 0) {  // the snapshot is the step's start as it came in: before this stage's reset
          x[j] = s[o];
          s0[o] = x[j];
          acc[o] = T(0);
        } else {
          const T sd = sdot[o];
          acc[o] = acc[o] + bk * sd;
          x[j] = s0[o] + (stage == 3 ? T(1) : T(0.5)) * dt * sd;
        }
      }
      const bool inside = contact_pair_wrench<T>(pt, vel, x, c, hs + (long)h * 6, xd, w);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const long o = (so + j) * Ls.sk + bs;
        s[o] = inside ? x[j] : T(0);  // the stage state, reset where the point is outside
        sdot[o] = xd[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) tw[(long)(6 * body_i + j) * Lf.sk + b * Lf.sb] += w[j];
  }
}

template <typename T>
hipError_t launch_contact_head(const DevModel& M, long B, const void* q, const void* v, const void* tau_ff, const void* qdes, const void* kp, const void* kd,
                               void* tau_out, void* body_out, Layout Lq, Layout Lv, hipStream_t st) {
  MkFuse F{};
  F.stage = -1;
  if (tau_out) { F.pd_kp = kp; F.pd_kd = kd; F.pd_qdes = qdes; }
  // one lane per (state, body), M.lps lanes per state: rnea_kernel's grid
  const long spw = 64 / M.lps, waves = (B + spw - 1) / spw;
  contact_head_kernel<T><<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(M, B, (const T*)q, (const T*)v, (const T*)tau_ff, F, (T*)tau_out, (T*)body_out, Lq, Lv);
  return hipGetLastError();
}
template <typename T>
hipError_t launch_contact_sim(const ContactModel& M, long B, int stage, double dt, const void* body, void* s, void* sdot, void* s0, void* acc, const void* fext,
                              void* tw, Layout Ls, Layout Lf, hipStream_t st) {
  const long n = stage == 4 ? 3L * M.np * M.nh * B : B;  // threads: one per state, at the closing stage one per value of s
  contact_sim_kernel<T><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(M, B, stage, (T)dt, (const T*)body, (T*)s, (T*)sdot, (T*)s0, (T*)acc, (const T*)fext, (T*)tw,
                                                                     Ls, Lf);
  return hipGetLastError();
}
template hipError_t launch_contact_head<double>(const DevModel&, long, const void*, const void*, const void*, const void*, const void*, const void*, void*, void*, Layout,
                                                Layout, hipStream_t);
template hipError_t launch_contact_head<float>(const DevModel&, long, const void*, const void*, const void*, const void*, const void*, const void*, void*, void*, Layout,
                                               Layout, hipStream_t);
template hipError_t launch_contact_sim<double>(const ContactModel&, long, int, double, const void*, void*, void*, void*, void*, const void*, void*, Layout, Layout,
                                               hipStream_t);
template hipError_t launch_contact_sim<float>(const ContactModel&, long, int, double, const void*, void*, void*, void*, void*, const void*, void*, Layout, Layout,
                                              hipStream_t);

}  // namespace rbd
