// rbd_contact_kernels.hip — soft contact on the device: contact_dynamics! (src/mechanism_algorithms.jl:680-723) with the reference's
// default models (src/contact.jl: HuntCrossleyModel :98-119, ViscoelasticCoulombModel :122-178, HalfSpace3D :202-228), and the
// Runge–Kutta bookkeeping of the additional state for the derivatives of `simulate` (src/ode_integrators.jl:233-299; `simulate`
// itself: rbd_contact_sim_kernels.hip).
//
// contact_kernel: one thread per state.  Body transforms and twists come from the exported per-body kinematics ([state][body][24]:
// R, p, twist in slots 0 … 17 — contact_head_kernel's export, or the any-size kernels' on trees of more than 64 bodies); the thread
// walks the contact points in the order of the additional state, tests each
// against every half-space and adds its wrench to its body's; it writes contactwrenches and totalwrenches = wext + contactwrenches
// (mechanism_algorithms.jl:851-856) for EVERY body, so the forward-dynamics launch that follows reads one wrench buffer.
// No contact configuration is on a BASELINE hot path: clarity over speed here.
//
// contact_adjoint_kernel: the pullback of contact_kernel (rbd_contact.hpp contact_pair_adjoint), one thread per state between the adjoint RNEA pass, whose
// f̄ext is the cotangent of the wrenches it reads, and point_adjoint_kernel, which reads the per-point cotangents it writes.
//
// contact_stage_value_kernel, contact_stage_adjoint_kernel: the friction state through the Runge–Kutta tableau in value form and one stage of its backward
// pass with the contact model's pullback folded in (rbd_simulate_contact_vjp).
#include "rbd_device.hpp"
#include "rbd_internal.hpp"
#include "rbd_contact.hpp"

namespace rbd {

template <typename T>
__global__ __launch_bounds__(256) void contact_kernel(ContactModel M, long B, const T* __restrict__ body, T* __restrict__ s, T* __restrict__ sdot,
                                                     const T* __restrict__ fext, T* __restrict__ cw, T* __restrict__ tw, Layout Ls, Layout Lf) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const T* cp = reinterpret_cast<const T*>(M.cp);
  const T* hs = reinterpret_cast<const T*>(M.hs);
  // contactwrenches = 0, totalwrenches = wext for every body; the points then add their wrenches (a thread owns its state's columns)
  for (int j = 0; j < 6 * M.nb; ++j) {
    const long o = (long)j * Lf.sk + b * Lf.sb;
    if (cw) cw[o] = T(0);
    if (tw) tw[o] = fext ? fext[o] : T(0);
  }
  T* sx = s + b * Ls.sb;
  T* sd = sdot ? sdot + b * Ls.sb : nullptr;
  for (int ip = 0; ip < M.np; ++ip) {
    const int body_i = M.cbody[ip];
    const T* k = body + (b * M.nb + body_i) * 24;
    const T* c = cp + (long)ip * CP_STRIDE;
    T w[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    // point = body_to_root * location; velocity = point_velocity(twist, point) = ω × point + v   (:697-699)
    T pt[3], vel[3];
    contact_point_in_root(k, c, pt, vel);
    for (int h = 0; h < M.nh; ++h) {
      const long so = (long)(ip * M.nh + h) * 3;
      T x[3], xd[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) x[j] = sx[(so + j) * Ls.sk];
      const bool inside = contact_pair_wrench<T>(pt, vel, x, c, hs + (long)h * 6, xd, w);  // the pair model (rbd_contact.hpp)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (!inside) sx[(so + j) * Ls.sk] = T(0);  // reset! the state (:714-715); ẋ is zero there
        if (sd) sd[(so + j) * Ls.sk] = xd[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const long o = (long)(6 * body_i + j) * Lf.sk + b * Lf.sb;
      if (cw) cw[o] += w[j];
      if (tw) tw[o] += w[j];
    }
  }
}

// For every contact point: pos and vel again from the exported per-body kinematics, the cotangent (τ̄q; f̄) of its body's wrench (wbar, nullable: zero), the
// cotangents of ṡ and of s after the resets (sdbar, sobar, nullable) per half-space -> s_bar (nullable) and the point's pos_bar, vel_bar summed over the
// half-spaces (3 np values per state each, layout L3: what point_adjoint_kernel reads).  Every output element is written.
template <typename T>
__global__ __launch_bounds__(256) void contact_adjoint_kernel(ContactModel M, long B, const T* __restrict__ body, const T* __restrict__ s,
                                                             const T* __restrict__ wbar, const T* __restrict__ sdbar, const T* __restrict__ sobar,
                                                             T* __restrict__ sbar, T* __restrict__ pbar, T* __restrict__ vbar, Layout Ls, Layout Lf, Layout L3) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const T* cp = reinterpret_cast<const T*>(M.cp);
  const T* hs = reinterpret_cast<const T*>(M.hs);
  const long bs = b * Ls.sb, bf = b * Lf.sb, b3 = b * L3.sb;
  for (int ip = 0; ip < M.np; ++ip) {
    const int body_i = M.cbody[ip];
    const T* k = body + (b * M.nb + body_i) * 24;
    const T* c = cp + (long)ip * CP_STRIDE;
    T pt[3], vel[3], wb[6], pb[3] = {T(0), T(0), T(0)}, vb[3] = {T(0), T(0), T(0)};
    contact_point_in_root(k, c, pt, vel);
#pragma unroll
    for (int j = 0; j < 6; ++j) wb[j] = wbar ? wbar[(long)(6 * body_i + j) * Lf.sk + bf] : T(0);
    for (int h = 0; h < M.nh; ++h) {
      const long so = (long)(ip * M.nh + h) * 3;
      T x[3], xdb[3], xob[3], p1[3], v1[3], xb[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const long o = (so + j) * Ls.sk + bs;
        x[j] = s[o];
        xdb[j] = sdbar ? sdbar[o] : T(0);
        xob[j] = sobar ? sobar[o] : T(0);
      }
      contact_pair_adjoint<T>(pt, vel, x, c, hs + (long)h * 6, wb + 3, wb, xdb, xob, p1, v1, xb);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        pb[j] += p1[j];
        vb[j] += v1[j];
        if (sbar) sbar[(so + j) * Ls.sk + bs] = xb[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const long o = (long)(3 * ip + j) * L3.sk + b3;
      pbar[o] = pb[j];
      vbar[o] = vb[j];
    }
  }
}

// The additional state through a Runge–Kutta step in value form for rbd_simulate_contact_vjp (rbd_contact.hpp contact_stage_value), elementwise over the ns·B
// values like value_mk_stage_kernel over the joints: stage 0 … 3, the stage states and the sum in buffers of their own (sn may be s0 itself at stage 3).
template <typename T>
__global__ __launch_bounds__(256) void contact_stage_value_kernel(long n, int stage, T dt, const T* s0, const T* __restrict__ sdot, T* __restrict__ acc, T* sn) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T a = stage == 0 ? T(0) : acc[i], o;
  contact_stage_value<T>(stage, dt, s0[i], sdot[i], a, o);
  if (stage < 3) acc[i] = a;
  sn[i] = o;
}

// One stage of rbd_simulate_contact_vjp's backward pass for the friction state and the contact model, one thread per state like contact_adjoint_kernel, after
// the adjoint RNEA pass of the stage has written THIS stage's cotangent of the total wrenches to wbar (not a sum over stages):
//   - the tableau's pullback per value of s (contact_stage_adjoint): sbar holds the cotangent of the stage's output on entry; ṡ̄_k stays in registers, the
//     cotangents of s0 and of the running sum live in s0b, accb (written at stage 3, read at 2 … 0);
//   - contact_pair_adjoint per (point, half-space) pair at the exported per-body kinematics and the stage state s, with ṡ̄_k and wbar (the cotangent of s
//     after the resets is zero: the resets never reach the state after the step);
//   - sbar on return: the stage state's cotangent — the pair's x̄, at stage 0 with the cotangent of s0 collected over the four stages added;
//   - fbar (nullable) += wbar for every body: the caller's f̄ext is the sum over the stages;
//   - the per-point pos_bar, vel_bar summed over the half-spaces, in the layout point_adjoint_kernel reads.
template <typename T>
__global__ __launch_bounds__(256) void contact_stage_adjoint_kernel(ContactModel M, long B, int stage, T dt, const T* __restrict__ body, const T* __restrict__ s,
                                                                   const T* __restrict__ wbar, T* __restrict__ fbar, T* __restrict__ sbar, T* __restrict__ s0b,
                                                                   T* __restrict__ accb, T* __restrict__ pbar, T* __restrict__ vbar, Layout Ls, Layout Lf,
                                                                   Layout L3) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const T* cp = reinterpret_cast<const T*>(M.cp);
  const T* hs = reinterpret_cast<const T*>(M.hs);
  const long bs = b * Ls.sb, bf = b * Lf.sb, b3 = b * L3.sb;
  if (fbar)
    for (int j = 0; j < 6 * M.nb; ++j) {
      const long o = (long)j * Lf.sk + bf;
      fbar[o] += wbar[o];
    }
  for (int ip = 0; ip < M.np; ++ip) {
    const int body_i = M.cbody[ip];
    const T* k = body + (b * M.nb + body_i) * 24;
    const T* c = cp + (long)ip * CP_STRIDE;
    T pt[3], vel[3], wb[6], pb[3] = {T(0), T(0), T(0)}, vb[3] = {T(0), T(0), T(0)};
    contact_point_in_root(k, c, pt, vel);
#pragma unroll
    for (int j = 0; j < 6; ++j) wb[j] = wbar[(long)(6 * body_i + j) * Lf.sk + bf];
    for (int h = 0; h < M.nh; ++h) {
      const long so = (long)(ip * M.nh + h) * 3;
      T x[3], xdb[3], s0c[3], p1[3], v1[3], xb[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const long o = (so + j) * Ls.sk + bs;
        x[j] = s[o];
        T ab = stage == 3 ? T(0) : accb[o];
        s0c[j] = stage == 3 ? T(0) : s0b[o];
        contact_stage_adjoint<T>(stage, dt, sbar[o], s0c[j], ab, xdb[j]);
        if (stage == 3) accb[o] = ab;
        if (stage > 0) s0b[o] = s0c[j];
      }
      contact_pair_adjoint<T>(pt, vel, x, c, hs + (long)h * 6, wb + 3, wb, xdb, (const T*)nullptr, p1, v1, xb);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        pb[j] += p1[j];
        vb[j] += v1[j];
        sbar[(so + j) * Ls.sk + bs] = stage == 0 ? s0c[j] + xb[j] : xb[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const long o = (long)(3 * ip + j) * L3.sk + b3;
      pbar[o] = pb[j];
      vbar[o] = vb[j];
    }
  }
}

template <typename T>
hipError_t launch_contact(const ContactModel& M, long B, const void* body, void* s, void* sdot, const void* fext, void* cw, void* tw, Layout Ls, Layout Lf,
                          hipStream_t st) {
  contact_kernel<T><<<(unsigned)((B + 255) / 256), 256, 0, st>>>(M, B, (const T*)body, (T*)s, (T*)sdot, (const T*)fext, (T*)cw, (T*)tw, Ls, Lf);
  return hipGetLastError();
}
template <typename T>
hipError_t launch_contact_adjoint(const ContactModel& M, long B, const void* body, const void* s, const void* wbar, const void* sdbar, const void* sobar, void* sbar,
                                  void* pbar, void* vbar, Layout Ls, Layout Lf, Layout L3, hipStream_t st) {
  contact_adjoint_kernel<T><<<(unsigned)((B + 255) / 256), 256, 0, st>>>(M, B, (const T*)body, (const T*)s, (const T*)wbar, (const T*)sdbar, (const T*)sobar, (T*)sbar,
                                                                         (T*)pbar, (T*)vbar, Ls, Lf, L3);
  return hipGetLastError();
}
template <typename T>
hipError_t launch_contact_stage_value(long n, int stage, double dt, const void* s0, const void* sdot, void* acc, void* sn, hipStream_t st) {
  contact_stage_value_kernel<T><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, stage, (T)dt, (const T*)s0, (const T*)sdot, (T*)acc, (T*)sn);
  return hipGetLastError();
}
template <typename T>
hipError_t launch_contact_stage_adjoint(const ContactModel& M, long B, int stage, double dt, const void* body, const void* s, const void* wbar, void* fbar, void* sbar,
                                        void* s0b, void* accb, void* pbar, void* vbar, Layout Ls, Layout Lf, Layout L3, hipStream_t st) {
  contact_stage_adjoint_kernel<T><<<(unsigned)((B + 255) / 256), 256, 0, st>>>(M, B, stage, (T)dt, (const T*)body, (const T*)s, (const T*)wbar, (T*)fbar, (T*)sbar,
                                                                               (T*)s0b, (T*)accb, (T*)pbar, (T*)vbar, Ls, Lf, L3);
  return hipGetLastError();
}
template hipError_t launch_contact<double>(const ContactModel&, long, const void*, void*, void*, const void*, void*, void*, Layout, Layout, hipStream_t);
template hipError_t launch_contact<float>(const ContactModel&, long, const void*, void*, void*, const void*, void*, void*, Layout, Layout, hipStream_t);
template hipError_t launch_contact_adjoint<double>(const ContactModel&, long, const void*, const void*, const void*, const void*, const void*, void*, void*, void*, Layout,
                                                  Layout, Layout, hipStream_t);
template hipError_t launch_contact_adjoint<float>(const ContactModel&, long, const void*, const void*, const void*, const void*, const void*, void*, void*, void*, Layout,
                                                 Layout, Layout, hipStream_t);
template hipError_t launch_contact_stage_value<double>(long, int, double, const void*, const void*, void*, void*, hipStream_t);
template hipError_t launch_contact_stage_value<float>(long, int, double, const void*, const void*, void*, void*, hipStream_t);
template hipError_t launch_contact_stage_adjoint<double>(const ContactModel&, long, int, double, const void*, const void*, const void*, void*, void*, void*, void*, void*,
                                                        void*, Layout, Layout, Layout, hipStream_t);
template hipError_t launch_contact_stage_adjoint<float>(const ContactModel&, long, int, double, const void*, const void*, const void*, void*, void*, void*, void*, void*,
                                                       void*, Layout, Layout, Layout, hipStream_t);

}  // namespace rbd
