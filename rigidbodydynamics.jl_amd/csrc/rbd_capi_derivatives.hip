// rbd_capi_derivatives.hip — the derivative entry points of the C ABI (include/rbd_hip.h): forward mode (JVPs, Jacobians), reverse mode (VJPs), both through
// simulate steps and soft contact, and point kinematics.  The workspace and what every entry point starts with: rbd_capi_internal.hpp; the kernels:
// rbd_tangent_kernels.hip, rbd_point_kernels.hip, rbd_contact_kernels.hip.
#include "rbd_capi_internal.hpp"
#include "rbd_contact.hpp"

// ---- forward-mode derivatives of inverse_dynamics! and dynamics! (header 700; kernels: rbd_tangent_kernels.hip) --------------------------------------------
namespace {
enum : long { TAN_SCRATCH_CAP = 1L << 30 };  // bytes of tangent scratch at most: larger calls run in slabs of (state, chunk) threads

// the tree in the reference's order (BigModel tables) for every mechanism: built by the first derivative call or by rbd_workspace_set_points
int tan_tables(rbd_ws* w) {
  const rbd_model* m = w->model;
  int st;
  if (w->tan_tbl_ready) return RBD_OK;
  if (m->big) {
    w->tan = w->big;
  } else {  // the slot-ordered tables back in the reference's order (parents first: rbd_model_create checks it)
    const int nb = m->nb;
    std::vector<int32_t> tbl(4 * (size_t)nb);
    std::vector<double> rb((size_t)nb * RB_STRIDE);
    for (int i = 0; i < nb; ++i) {
      const int s = m->slot_of[i];
      const int32_t* ib = &m->ib[(size_t)s * IB_STRIDE];
      tbl[4 * i] = ib[IB_PARENT] < 0 ? -1 : m->order[ib[IB_PARENT]];
      tbl[4 * i + 1] = ib[IB_JTYPE]; tbl[4 * i + 2] = ib[IB_QOFF]; tbl[4 * i + 3] = ib[IB_VOFF];
      memcpy(&rb[(size_t)i * RB_STRIDE], &m->rb[(size_t)s * RB_STRIDE], sizeof(double) * RB_STRIDE);
    }
    if ((st = upload_real(w->d_tan_rb, rb, w->dtype))) return st;
    w->tan.nb = nb; w->tan.nq = m->nq; w->tan.nv = m->nv; w->tan.rb = w->d_tan_rb.p;
    memcpy(w->tan.gravity, m->gravity, sizeof w->tan.gravity);
    if ((st = upload(w->d_tan_tbl, tbl.data(), tbl.size() * sizeof(int32_t)))) return st;
    w->tan.tbl = (const int32_t*)w->d_tan_tbl.p;
  }
  w->tan_tbl_ready = true;
  return RBD_OK;
}

// the tables of np points (point k on reference body body[k] at r[3k … 3k + 2]) on the device: rbd_workspace_set_points, and the model's contact points for
// the contact VJPs.  d_i, d_r: the two buffers (what they held is freed)
int point_plan_upload(rbd_ws* w, int np, const int32_t* body, const double* r, DevBuf& d_i, DevBuf& d_r, PointPlan* out) {
  const rbd_model* m = w->model;
  int st;
  const PointPlanTables T = point_plan(m->nb, m->parent_ref.data(), np, body);
  const std::vector<int32_t>&poff = T.poff, &path = T.path, &uni = T.uni, &ubeg = T.ubeg, &upts = T.upts;
  std::vector<int32_t> all;
  const size_t o_path = poff.size(), o_uni = o_path + path.size(), o_ubeg = o_uni + uni.size(), o_upts = o_ubeg + ubeg.size();
  for (const std::vector<int32_t>* v : {&poff, &path, &uni, &ubeg, &upts}) all.insert(all.end(), v->begin(), v->end());
  if ((st = upload(d_i, all.data(), all.size() * sizeof(int32_t)))) return st;
  if ((st = upload_real(d_r, std::vector<double>(r, r + 3 * (size_t)np), w->dtype))) return st;
  const int32_t* d = (const int32_t*)d_i.p;
  *out = PointPlan{np, (int32_t)uni.size(), d, d + o_path, d + o_uni, d + o_ubeg, d + o_upts, d_r.p};
  return RBD_OK;
}

// what every derivative entry point shares, allocated by the first one: the tables in the reference's order, M, its factor, c and v̇
int tan_base(rbd_ws* w) {
  const rbd_model* m = w->model;
  const size_t es = esize(w);
  const long B = w->max_batch;
  int st;
  if (!w->tan_ready) {
    if ((st = tan_tables(w))) return st;
    if (m->big && (st = big_scratch(w, w->max_batch))) return st;
    const size_t nv = (size_t)m->nv;
    if ((st = ensure(w->d_tan_M, es * nv * nv * B)) || (st = ensure(w->d_tan_L, es * nv * nv * B)) ||
        (st = ensure(w->d_tan_c, es * nv * B)) || (st = ensure(w->d_tan_vd, es * nv * B)))
      return st;
    w->tan_ready = true;
  }
  return RBD_OK;
}

// the first derivative call of a workspace (and one with more directions than before) allocates; every later call only launches
int tan_ensure(rbd_ws* w, int ntan) {
  const rbd_model* m = w->model;
  const size_t es = esize(w);
  const long B = w->max_batch;
  int st;
  if ((st = tan_base(w))) return st;
  ntan = std::max(ntan, m->nq + m->nv);  // (the Jacobians' directions: a JVP call after a derivatives call allocates nothing)
  if (ntan > w->tan_ntan) {
    const int N = tangent_chunk((int)es);
    const size_t per = std::max<size_t>(1, tangent_scratch_elems_per_thread(w->tan, (int)es) * es);
    const long want = B * ((ntan + N - 1) / N);
    // RBD_TUNE tan_scratch_threads=<k>: room for k (state, chunk) threads instead of the byte cap (tests reach the several-slabs path at small sizes)
    bool has;
    const long knob = tune("tan_scratch_threads", 0, &has);
    const long cap = has ? std::max(1L, knob) : std::max<long>(64, (long)(TAN_SCRATCH_CAP / per) / 64 * 64);
    const long threads = std::min(want, cap);
    if ((st = ensure(w->d_tan_scratch, per * threads))) return st;
    w->tan_threads = threads;
    if ((st = ensure(w->d_tan_rhs, es * std::max<size_t>(1, (size_t)m->nv * ntan * B)))) return st;
    if (chol_beyond_lanes(m->nv) && (st = ensure(w->d_tan_x, es * (size_t)m->nv * ntan * B))) return st;
    w->tan_ntan = ntan;
  }
  return RBD_OK;
}

// the checks every derivative call shares (every model size: the tangent kernels walk the tree in the reference's order, rbd_tangent_kernels.hip)
int tan_check(rbd_ws* w, int32_t B, const rbd_opts_t* opts, Opts* o) {
  if (int st = begin_call(w, B, opts, kAnySize, o)) return st;
  if (w->model->nloops > 0) return RBD_ERR_HAS_LOOPS;  // (inverse_dynamics!: src/mechanism_algorithms.jl:549)
  if (w->model->ncp > 0 && w->model->nhs > 0) return RBD_ERR_UNSUPPORTED;  // (as rbd_dynamics: the contact wrenches need the additional state)
  if (o->memory != RBD_MEM_DEVICE) return RBD_ERR_UNSUPPORTED;
  return RBD_OK;
}

template <typename T> TanArgs<T> tan_args(rbd_ws* w, int32_t B, int layout, int ntan, const void* q, const void* v, const void* vdot, const void* fext) {
  const rbd_model* m = w->model;
  TanArgs<T> A{};
  A.B = B; A.ntan = ntan; A.unit = 0; A.g0 = 0;
  A.q = (const T*)q; A.v = (const T*)v; A.vdot = (const T*)vdot; A.fext = (const T*)fext;
  A.Lq = layout_of(layout, m->nq, B); A.Lv = layout_of(layout, m->nv, B); A.Lf = layout_of(layout, 6L * m->nb, B);
  A.Ldq = layout_of(layout, (long)m->nq * ntan, B); A.Ldv = layout_of(layout, (long)m->nv * ntan, B); A.Ldf = layout_of(layout, 6L * m->nb * ntan, B);
  A.sign = T(1);
  A.out = ColOut<T>::single(nullptr, Layout{0, 0}, m->nv);
  return A;
}

// dynamics!'s value the reference's way (dynamics_solve! :764, :819): c = dynamics_bias!, M = mass_matrix!, L = chol(M) into the workspace, v̇ = L⁻ᵀ L⁻¹ (τ − c)
template <typename T> int tan_dynamics_value(rbd_ws* w, int32_t B, int layout, const void* q, const void* v, const void* tau, const void* fext, void* vd) {
  const rbd_model* m = w->model;
  const Layout Lq = layout_of(layout, m->nq, B), Lv = layout_of(layout, m->nv, B), Lf = layout_of(layout, 6L * m->nb, B), Lm{B, 1};
  if (m->big) {
    HIP_TRY(launch_big_rnea<T>(w->big, B, q, v, nullptr, fext, w->d_tan_c.p, nullptr, w->d_big_scratch.p, nullptr, nullptr, Lq, Lv, Lf, w->stream));
    HIP_TRY(launch_big_crba<T>(w->big, B, q, w->d_tan_M.p, w->d_big_scratch.p, Lq, Lm, w->stream));
  } else {
    HIP_TRY(launch_rnea<T>(w->dm, B, q, v, nullptr, fext, w->d_tan_c.p, nullptr, nullptr, Lq, Lv, Lf, w->stream));
    HIP_TRY(launch_crba<T>(w->dm, B, q, w->d_tan_M.p, Lq, Lm, 1, w->stream));
  }
  // the factor stays in d_tan_L (batch-innermost, as M) for the solves that follow
  return dense_solve(w, B, w->d_tan_M.p, tau, w->d_tan_c.p, vd, w->d_tan_L.p, Lm, Lv, w->d_tan_L);
}

template <typename T>
int tan_id_jvp(rbd_ws* w, int32_t B, int32_t ntan, int layout, const void* q, const void* v, const void* vdot, const void* fext, const void* dq, const void* dv,
               const void* dvdot, const void* dfext, void* tau_out, void* dtau_out) {
  TanArgs<T> A = tan_args<T>(w, B, layout, ntan, q, v, vdot, fext);
  A.dq = (const T*)dq; A.dv = (const T*)dv; A.dvdot = (const T*)dvdot; A.dfext = (const T*)dfext;
  A.tau = (T*)tau_out;
  A.out.a = (T*)dtau_out; A.out.La = A.Ldv;
  HIP_TRY(launch_tangent_rnea<T>(w->tan, A, w->d_tan_scratch.p, w->tan_threads, w->stream));
  return RBD_OK;
}

template <typename T>
int tan_dyn_jvp(rbd_ws* w, int32_t B, int32_t ntan, int layout, const void* q, const void* v, const void* tau, const void* fext, const void* dq, const void* dv,
                const void* dtau, const void* dfext, void* vdot_out, void* dvdot_out) {
  const rbd_model* m = w->model;
  void* vd = vdot_out ? vdot_out : w->d_tan_vd.p;
  int st;
  if ((st = tan_dynamics_value<T>(w, B, layout, q, v, tau, fext, vd))) return st;
  if (!dvdot_out) return RBD_OK;
  // M dv̇ = dτ − ∂ID(q, v, v̇)·(dq, dv, 0, dfext): the right-hand sides (batch-innermost) in one tangent pass, then ntan solves against the one factor
  TanArgs<T> A = tan_args<T>(w, B, layout, ntan, q, v, vd, fext);
  A.dq = (const T*)dq; A.dv = (const T*)dv; A.dfext = (const T*)dfext;
  A.out.a = (T*)w->d_tan_rhs.p; A.out.La = Layout{B, 1};
  A.sign = T(-1); A.dadd = (const T*)dtau;
  HIP_TRY(launch_tangent_rnea<T>(w->tan, A, w->d_tan_scratch.p, w->tan_threads, w->stream));
  const ColOut<T> out = ColOut<T>::single((T*)dvdot_out, A.Ldv, m->nv);
  HIP_TRY(launch_tangent_solve<T>(m->nv, B, 0, ntan, w->d_tan_L.p, Layout{B, 1}, w->d_tan_rhs.p, 0, out, w->d_tan_x.p, w->stream));
  return RBD_OK;
}

template <typename T>
int tan_id_derivs(rbd_ws* w, int32_t B, int layout, const void* q, const void* v, const void* vdot, const void* fext, void* tau_out, void* dtau_dq, void* dtau_dv,
                  void* M_out) {
  const rbd_model* m = w->model;
  // the directions asked for: the columns of ∂/∂q (e_0 … e_nq−1 of (q; v)), then those of ∂/∂v
  const int g0 = dtau_dq ? 0 : m->nq, g1 = dtau_dv ? m->nq + m->nv : m->nq;
  if (g1 > g0 || tau_out) {
    TanArgs<T> A = tan_args<T>(w, B, layout, std::max(1, g1 - g0), q, v, vdot, fext);
    A.unit = 1; A.g0 = g0;
    A.tau = (T*)tau_out;
    A.out = ColOut<T>{(T*)dtau_dq, layout_of(layout, (long)m->nv * m->nq, B), (T*)dtau_dv, layout_of(layout, (long)m->nv * m->nv, B), m->nq, m->nv};
    if (g1 <= g0) A.out.a = A.out.b = nullptr;  // (τ alone)
    HIP_TRY(launch_tangent_rnea<T>(w->tan, A, w->d_tan_scratch.p, w->tan_threads, w->stream));
  }
  if (M_out) {  // ∂τ/∂v̇ = M (mass_matrix! :248-272), the full square
    const Layout Lq = layout_of(layout, m->nq, B), Lm = layout_of(layout, (long)m->nv * m->nv, B);
    if (m->big) HIP_TRY(launch_big_crba<T>(w->big, B, q, M_out, w->d_big_scratch.p, Lq, Lm, w->stream));
    else HIP_TRY(launch_crba<T>(w->dm, B, q, M_out, Lq, Lm, 1, w->stream));
    HIP_TRY(launch_symmetrize<T>(m->nv, B, M_out, Lm, w->stream));
  }
  return RBD_OK;
}

template <typename T>
int tan_dyn_derivs(rbd_ws* w, int32_t B, int layout, const void* q, const void* v, const void* tau, const void* fext, void* vdot_out, void* dvdot_dq, void* dvdot_dv,
                   void* dvdot_dtau) {
  const rbd_model* m = w->model;
  void* vd = vdot_out ? vdot_out : w->d_tan_vd.p;
  int st;
  if ((st = tan_dynamics_value<T>(w, B, layout, q, v, tau, fext, vd))) return st;
  const int g0 = dvdot_dq ? 0 : m->nq, g1 = dvdot_dv ? m->nq + m->nv : m->nq;
  if (g1 > g0) {  // −∂ID/∂(q, v) at the computed v̇, column g of the right-hand sides at g; then M⁻¹ of each
    TanArgs<T> A = tan_args<T>(w, B, layout, g1 - g0, q, v, vd, fext);
    A.unit = 1; A.g0 = g0;
    A.out.a = (T*)w->d_tan_rhs.p; A.out.La = Layout{B, 1};
    A.sign = T(-1);
    HIP_TRY(launch_tangent_rnea<T>(w->tan, A, w->d_tan_scratch.p, w->tan_threads, w->stream));
    const ColOut<T> out{(T*)dvdot_dq, layout_of(layout, (long)m->nv * m->nq, B), (T*)dvdot_dv, layout_of(layout, (long)m->nv * m->nv, B), m->nq, m->nv};
    HIP_TRY(launch_tangent_solve<T>(m->nv, B, g0, g1 - g0, w->d_tan_L.p, Layout{B, 1}, w->d_tan_rhs.p, 0, out, w->d_tan_x.p, w->stream));
  }
  if (dvdot_dtau) {  // ∂v̇/∂τ = M⁻¹: the solve against the identity, generated in the kernel
    const ColOut<T> out = ColOut<T>::single((T*)dvdot_dtau, layout_of(layout, (long)m->nv * m->nv, B), m->nv);
    HIP_TRY(launch_tangent_solve<T>(m->nv, B, 0, m->nv, w->d_tan_L.p, Layout{B, 1}, nullptr, 1, out, w->d_tan_x.p, w->stream));
  }
  return RBD_OK;
}

// ---- reverse mode (header 700 additions): the adjoint RNEA, one thread per state -------------------------------------------------------------------------
enum : long { ADJ_SCRATCH_CAP = TAN_SCRATCH_CAP };  // bytes of adjoint scratch at most: larger calls run in slabs of states

// the adjoint scratch for max_batch states, in slabs beyond the cap (needs the tables of `tan`): also all that rbd_point_kinematics_vjp allocates
int adj_scratch_ensure(rbd_ws* w) {
  if (w->adj_states > 0) return RBD_OK;
  const size_t per = std::max<size_t>(1, adjoint_scratch_elems_per_state(w->tan) * esize(w));
  const long states = std::min<long>(w->max_batch, std::max<long>(64, (long)(ADJ_SCRATCH_CAP / per) / 64 * 64));
  if (int st = ensure(w->d_adj_scratch, per * std::max<long>(1, states))) return st;
  w->adj_states = std::max<long>(1, states);
  return RBD_OK;
}

// the first reverse-mode call of a workspace allocates (for max_batch states); every later call only launches
int adj_ensure(rbd_ws* w) {
  const rbd_model* m = w->model;
  const size_t es = esize(w), nv = (size_t)m->nv;
  const long B = w->max_batch;
  int st;
  if ((st = tan_base(w))) return st;
  if (w->adj_ready) return RBD_OK;
  if ((st = adj_scratch_ensure(w))) return st;
  if ((st = ensure(w->d_adj_rhs, es * std::max<size_t>(1, nv * B))) || (st = ensure(w->d_adj_lam, es * std::max<size_t>(1, nv * B))))
    return st;
  if (chol_beyond_lanes(m->nv) && (st = ensure(w->d_adj_x, es * nv * B))) return st;
  w->adj_ready = true;
  return RBD_OK;
}

template <typename T> AdjArgs<T> adj_args(rbd_ws* w, int32_t B, int layout, const void* q, const void* v, const void* vdot, const void* fext) {
  const rbd_model* m = w->model;
  AdjArgs<T> A{};
  A.B = B;
  A.q = (const T*)q; A.v = (const T*)v; A.vdot = (const T*)vdot; A.fext = (const T*)fext;
  A.Lq = layout_of(layout, m->nq, B); A.Lv = layout_of(layout, m->nv, B); A.Lf = layout_of(layout, 6L * m->nb, B); A.Llam = A.Lv;
  A.sign = T(1);
  return A;
}

template <typename T>
int adj_id_vjp(rbd_ws* w, int32_t B, int layout, const void* q, const void* v, const void* vdot, const void* fext, const void* tau_bar, void* tau_out,
               void* q_bar, void* v_bar, void* vdot_bar, void* fext_bar) {
  AdjArgs<T> A = adj_args<T>(w, B, layout, q, v, vdot, fext);
  A.lam = (const T*)tau_bar;
  A.tau = (T*)tau_out; A.qbar = (T*)q_bar; A.vbar = (T*)v_bar; A.vdbar = (T*)vdot_bar; A.fbar = (T*)fext_bar;
  HIP_TRY(launch_adjoint_rnea<T>(w->tan, A, w->d_adj_scratch.p, w->adj_states, w->stream));
  return RBD_OK;
}

// v̇ = M⁻¹(τ − c) the reference's way (as rbd_dynamics_jvp), λ = M⁻¹ v̇̄ against the same factor, τ̄ = λ, (q̄, v̄, f̄ext) = −(adjoint RNEA at (q, v, v̇), λ)
template <typename T>
int adj_dyn_vjp(rbd_ws* w, int32_t B, int layout, const void* q, const void* v, const void* tau, const void* fext, const void* vdot_bar, void* vdot_out,
                void* q_bar, void* v_bar, void* tau_bar, void* fext_bar) {
  const rbd_model* m = w->model;
  void* vd = vdot_out ? vdot_out : w->d_tan_vd.p;
  int st;
  if ((st = tan_dynamics_value<T>(w, B, layout, q, v, tau, fext, vd))) return st;
  if (!q_bar && !v_bar && !tau_bar && !fext_bar) return RBD_OK;
  const Layout Lv = layout_of(layout, m->nv, B), Li{B, 1};
  const void* rhs = vdot_bar;
  if (layout != RBD_LAYOUT_SOA) {  // (tri_solve_col reads its right-hand side batch-innermost: SOA as it stands)
    HIP_TRY(launch_stage_rows<T>(m->nv, B, vdot_bar, Lv, w->d_adj_rhs.p, w->stream));
    rhs = w->d_adj_rhs.p;
  }
  // λ straight into τ̄ when the caller asks for it (the adjoint pass reads it from there)
  const ColOut<T> lam = tau_bar ? ColOut<T>::single((T*)tau_bar, Lv, m->nv) : ColOut<T>::single((T*)w->d_adj_lam.p, Li, m->nv);
  HIP_TRY(launch_tangent_solve<T>(m->nv, B, 0, 1, w->d_tan_L.p, Li, rhs, 0, lam, w->d_adj_x.p, w->stream));
  if (!q_bar && !v_bar && !fext_bar) return RBD_OK;
  AdjArgs<T> A = adj_args<T>(w, B, layout, q, v, vd, fext);
  A.lam = lam.a; A.Llam = lam.La;
  A.qbar = (T*)q_bar; A.vbar = (T*)v_bar; A.fbar = (T*)fext_bar;
  A.sign = T(-1);
  HIP_TRY(launch_adjoint_rnea<T>(w->tan, A, w->d_adj_scratch.p, w->adj_states, w->stream));
  return RBD_OK;
}

// ---- reverse mode through soft contact (header 700 addition): rbd_contact_dynamics_vjp, rbd_dynamics_contact_vjp --------------------------------------------
// the first contact VJP of a workspace allocates, for max_batch states: what every reverse-mode call shares, the model's contact points as a PointPlan of
// their own, the per-point cotangents, the total wrenches and their cotangent, the copy of s, and what the forward contact launch writes; no later call does
int ct_ensure(rbd_ws* w) {
  const rbd_model* m = w->model;
  const size_t es = esize(w), B = (size_t)w->max_batch;
  int st;
  if ((st = adj_ensure(w))) return st;
  if (w->ct_ready) return RBD_OK;
  if (w->ct_pts.np == 0) {
    std::vector<double> r(3 * (size_t)m->ncp);
    for (int i = 0; i < m->ncp; ++i)
      for (int j = 0; j < 3; ++j) r[3 * (size_t)i + j] = m->cp_r[(size_t)i * CP_STRIDE + CP_LOC + j];
    if ((st = point_plan_upload(w, m->ncp, m->cp_body.data(), r.data(), w->d_ct_i, w->d_ct_r, &w->ct_pts))) return st;
  }
  if ((st = ensure(w->d_ct_pbar, es * 3 * m->ncp * B)) || (st = ensure(w->d_ct_vbar, es * 3 * m->ncp * B)) || (st = ensure(w->d_ct_wbar, es * 6 * m->nb * B)) ||
      (st = ensure(w->d_ct_s, es * 3 * m->ncp * m->nhs * B)) || (st = ensure(w->d_body, es * (size_t)m->nb * 24 * B)) ||
      (st = ensure(w->d_c, es * (size_t)m->nv * B)) || (st = ensure(w->d_tw, es * (size_t)6 * m->nb * B)))
    return st;
  w->ct_ready = true;
  return RBD_OK;
}

// contact_adjoint_kernel at the per-body kinematics in w->d_body, then point_adjoint_kernel over the contact points: the cotangents of the bodies' wrenches
// (wbar), of ṡ and of s after the resets -> s_bar and (q_bar, v_bar) — ADDED to what these hold with accum (the adjoint RNEA pass wrote its share before)
template <typename T>
int ct_adjoint(rbd_ws* w, int32_t B, int layout, const void* q, const void* v, const void* s, const void* wbar, const void* sdot_bar, const void* s_out_bar,
               void* q_bar, void* v_bar, void* s_bar, int accum) {
  const rbd_model* m = w->model;
  if (!q_bar && !v_bar && !s_bar) return RBD_OK;
  const Layout Ls = layout_of(layout, 3L * m->ncp * m->nhs, B), Lf = layout_of(layout, 6L * m->nb, B), L3 = layout_of(layout, 3L * m->ncp, B);
  HIP_TRY(launch_contact_adjoint<T>(w->ctm, B, w->d_body.p, s, wbar, sdot_bar, s_out_bar, s_bar, w->d_ct_pbar.p, w->d_ct_vbar.p, Ls, Lf, L3, w->stream));
  if (!q_bar && !v_bar) return RBD_OK;
  AdjArgs<T> A = adj_args<T>(w, B, layout, q, v, nullptr, nullptr);
  A.qbar = (T*)q_bar; A.vbar = (T*)v_bar; A.accum = accum;
  PointAdjArgs<T> C{(const T*)w->d_ct_pbar.p, (const T*)w->d_ct_vbar.p, L3};
  HIP_TRY(launch_point_adjoint<T>(w->tan, w->ct_pts, A, C, w->d_adj_scratch.p, w->adj_states, w->stream));
  return RBD_OK;
}

// ---- reverse mode through simulate steps (header 700 addition): rbd_simulate_vjp ----------------------------------------------------------------------
enum : long { SAV_CKPT_CAP = 1L << 30 };  // bytes of step starts kept while every step's fits; beyond that two-level (√n) checkpointing

// the first call of a workspace allocates the joint lists, one step's stage states and the backward pass's cotangents (for max_batch states)
int sav_ensure(rbd_ws* w) {
  const rbd_model* m = w->model;
  const size_t es = esize(w), B = (size_t)w->max_batch;
  int st;
  if ((st = adj_ensure(w))) return st;
  if (w->sav_ready) return RBD_OK;
  std::vector<int32_t> jl;  // the 1-coordinate joints first (adjoint_mk_stage_kernel<T, false>), then the rest
  int nn = 0, nw = 0;
  for (int wide = 0; wide < 2; ++wide)
    for (int i = 0; i < m->nb; ++i) {
      const int jt = m->jt_ref[i];
      if (jt == RBD_JOINT_FIXED || mk_narrow_joint(jt) == (wide == 1)) continue;
      jl.insert(jl.end(), {jt, m->qoff_ref[i], m->voff_ref[i]});
      ++(wide ? nw : nn);
    }
  if ((st = upload(w->d_sav_joints, jl.data(), jl.size() * sizeof(int32_t)))) return st;
  // stage states 1-3 (q, v), the running sums (2 nv), the base point's cotangent (nq + nv), v̇̄ and the sums' cotangents (3 nv)
  if ((st = ensure(w->d_sav, es * B * (4 * (size_t)m->nq + 9 * (size_t)m->nv)))) return st;
  w->sav_nn = nn; w->sav_nw = nw;
  w->sav_ready = true;
  return RBD_OK;
}

// which step starts are kept: all (S = 1, K = nsteps slots), or every S-th in slots 0 … K − 1 and one segment's others, recomputed, in K … K + S − 2.
// RBD_TUNE sim_vjp_ckpt_steps=<k>: room for k starts instead of the byte cap (tests reach the recompute path at small sizes).
struct SavPlan { int S, K, slots; };
SavPlan sav_plan(size_t slot_bytes, int nsteps) {
  bool has;
  const long knob = tune("sim_vjp_ckpt_steps", 0, &has);
  const long room = has ? std::max(1L, knob) : std::max<long>(1, (long)(SAV_CKPT_CAP / std::max<size_t>(1, slot_bytes)));
  if (nsteps <= room) return {1, nsteps, nsteps};
  const int S = (int)std::ceil(std::sqrt((double)nsteps)), K = (nsteps + S - 1) / S;
  return {S, K, K + S - 1};
}

template <typename T> struct SavBufs {
  T *qs[3], *vs[3], *accp, *accv, *q0b, *v0b, *vdb, *apb, *avb;
};
template <typename T> SavBufs<T> sav_bufs(rbd_ws* w) {
  const long nq = w->model->nq, nv = w->model->nv, Bm = w->max_batch;
  T* p = (T*)w->d_sav.p;
  SavBufs<T> b;
  for (int i = 0; i < 3; ++i) { b.qs[i] = p; p += nq * Bm; b.vs[i] = p; p += nv * Bm; }
  b.accp = p; p += nv * Bm; b.accv = p; p += nv * Bm;
  b.q0b = p; p += nq * Bm; b.v0b = p; p += nv * Bm;
  b.vdb = p; p += nv * Bm; b.apb = p; p += nv * Bm; b.avb = p;
  return b;
}

template <typename T> MkAdjArgs<T> sav_args(rbd_ws* w, int32_t B, int layout, double dt, int stage) {
  MkAdjArgs<T> A{};
  A.B = B; A.stage = stage; A.dt = (T)dt;
  A.Lq = layout_of(layout, w->model->nq, B); A.Lv = layout_of(layout, w->model->nv, B);
  A.Lqb = A.Lq; A.Lvb = A.Lv;
  return A;
}

// ---- the friction state beside (q, v) (rbd_simulate_contact_vjp): the optional contact argument of the sav_* templates -----------------------------------------
// the first call of a workspace allocates what rbd_simulate_vjp and the contact VJPs do, and the friction state's buffers (for max_batch states)
int sct_ensure(rbd_ws* w) {
  const rbd_model* m = w->model;
  int st;
  if ((st = sav_ensure(w)) || (st = ct_ensure(w))) return st;
  if (w->sct_ready) return RBD_OK;
  if ((st = ensure(w->d_sct, esize(w) * 7 * 3 * (size_t)m->ncp * m->nhs * w->max_batch))) return st;
  w->sct_ready = true;
  return RBD_OK;
}

template <typename T> struct SctBufs {
  T *ss[3], *acc, *sdot, *s0b, *accb;
};
template <typename T> SctBufs<T> sct_bufs(rbd_ws* w) {
  const long n = 3L * w->model->ncp * w->model->nhs * w->max_batch;
  T* p = (T*)w->d_sct.p;
  SctBufs<T> b;
  for (int i = 0; i < 3; ++i) { b.ss[i] = p; p += n; }
  b.acc = p; p += n; b.sdot = p; p += n; b.s0b = p; p += n; b.accb = p;
  return b;
}

// one step's friction state: s0 its start (a checkpoint slot or the caller's s: only read), sn the state after the step (the value pass; may be s0), s_bar
// the cotangent (the backward pass).  NULL for a mechanism without contact: rbd_simulate_vjp's launches as they were.
struct SavContact { const Opts* o; const void* s0; void* sn; void* s_bar; };

// the friction state at stage state `stage`: stage 0 a COPY of s0 (the forward contact launch resets the pairs outside — never a step's start), else the
// workspace's stage buffer
template <typename T> T* sct_stage_state(rbd_ws* w, int stage) { return stage == 0 ? (T*)w->d_ct_s.p : sct_bufs<T>(w).ss[stage - 1]; }

// contact_dynamics! at a stage state: the per-body kinematics into w->d_body, ṡ into the workspace, the total wrenches fext + contact into w->d_tw
template <typename T> int sct_contact(rbd_ws* w, int32_t B, const SavContact& C, int stage, const T* qs, const T* vs, const void* fext) {
  const rbd_model* m = w->model;
  T* ss = sct_stage_state<T>(w, stage);
  if (stage == 0) HIP_TRY(hipMemcpyAsync(ss, C.s0, sizeof(T) * 3 * m->ncp * m->nhs * B, hipMemcpyDeviceToDevice, w->stream));
  return run_contact(w, B, *C.o, qs, vs, ss, sct_bufs<T>(w).sdot, fext, nullptr, w->d_tw.p);
}

// the friction state's value stage map (contact_stage_value_kernel), after sct_contact left ṡ of the stage state
template <typename T> int sct_value_step(rbd_ws* w, int32_t B, const SavContact& C, int stage, double dt) {
  const rbd_model* m = w->model;
  const SctBufs<T> b = sct_bufs<T>(w);
  HIP_TRY(launch_contact_stage_value<T>(3L * m->ncp * m->nhs * B, stage, dt, C.s0, b.sdot, b.acc, stage == 3 ? C.sn : (void*)b.ss[stage], w->stream));
  return RBD_OK;
}

// the friction state's and the contact model's share of one stage pulled back, after the adjoint RNEA pass wrote THIS stage's cotangent of the total wrenches
// to w->d_ct_wbar: contact_stage_adjoint_kernel (the tableau, the pairs, s̄, f̄ext += the stage's, the per-point cotangents), then point_adjoint_kernel ADDING the
// contact points' kinematic pullback to the stage state's q̄, v̄
template <typename T>
int sct_backward_step(rbd_ws* w, int32_t B, int layout, const SavContact& C, int stage, double dt, const T* qs, const T* vs, void* q_bar, void* v_bar, void* fext_bar) {
  const rbd_model* m = w->model;
  const SctBufs<T> b = sct_bufs<T>(w);
  const Layout Ls = layout_of(layout, 3L * m->ncp * m->nhs, B), Lf = layout_of(layout, 6L * m->nb, B), L3 = layout_of(layout, 3L * m->ncp, B);
  HIP_TRY(launch_contact_stage_adjoint<T>(w->ctm, B, stage, dt, w->d_body.p, sct_stage_state<T>(w, stage), w->d_ct_wbar.p, fext_bar, C.s_bar, b.s0b, b.accb, w->d_ct_pbar.p,
                                          w->d_ct_vbar.p, Ls, Lf, L3, w->stream));
  AdjArgs<T> A = adj_args<T>(w, B, layout, qs, vs, nullptr, nullptr);
  A.qbar = (T*)q_bar; A.vbar = (T*)v_bar; A.accum = 1;
  PointAdjArgs<T> P{(const T*)w->d_ct_pbar.p, (const T*)w->d_ct_vbar.p, L3};
  HIP_TRY(launch_point_adjoint<T>(w->tan, w->ct_pts, A, P, w->d_adj_scratch.p, w->adj_states, w->stream));
  return RBD_OK;
}

// stages 0 … last of one step from (q0, v0), values only (the route of sim_tan_run: dynamics! by CRBA + Cholesky at every stage state, then the stage
// map): the stage states 1-3 and the running sums into the workspace, the state after the step (last = 3) into (qout, vout), which may be (q0, v0).
// With contact (C): dynamics! at the total wrenches of the stage state, and the friction state through the same tableau.
template <typename T>
int sav_value_step(rbd_ws* w, int32_t B, int layout, const T* q0, const T* v0, const void* tau, const void* fext, double dt, int last, T* qout, T* vout,
                   const SavContact* C = nullptr) {
  const SavBufs<T> b = sav_bufs<T>(w);
  const int32_t* jl = (const int32_t*)w->d_sav_joints.p;
  for (int stage = 0; stage <= last; ++stage) {
    const T* qs = stage == 0 ? q0 : b.qs[stage - 1];
    const T* vs = stage == 0 ? v0 : b.vs[stage - 1];
    int st;
    if (C && (st = sct_contact<T>(w, B, *C, stage, qs, vs, fext))) return st;
    if ((st = tan_dynamics_value<T>(w, B, layout, qs, vs, tau, C ? w->d_tw.p : fext, w->d_tan_vd.p))) return st;
    MkAdjArgs<T> A = sav_args<T>(w, B, layout, dt, stage);
    A.q0 = q0; A.v0 = v0; A.qs = qs; A.vs = vs; A.vd = (const T*)w->d_tan_vd.p; A.accp = b.accp; A.accv = b.accv;
    A.qn = stage == 3 ? qout : b.qs[stage]; A.vn = stage == 3 ? vout : b.vs[stage];
    HIP_TRY(launch_mk_stage_classes<T>(A, jl, w->sav_nn, jl + 3 * w->sav_nn, w->sav_nw, 0, w->stream));
    if (C && (st = sct_value_step<T>(w, B, *C, stage, dt))) return st;
  }
  return RBD_OK;
}

// One step pulled back: (q_bar, v_bar) hold the cotangent of the state after the step on entry and that of (q0, v0) on return; τ̄ and f̄ext accumulate.
// Stages 3 … 0: the stage map's pullback (v̇̄_i, the stage state's cotangent, the base point's), λ_i = M_i⁻¹ v̇̄_i, then the adjoint RNEA at the stage state
// with sign −1 ADDING −(∂ID)ᵀλ_i to the stage state's cotangent and f̄ext, and λ_i to τ̄.  `fresh`: the stage states, the sums and stage 3's factor and v̇
// are this step's already (the forward pass's last step).  With contact (C): the values at the stage's total wrenches, whose cotangent of THIS stage alone the
// adjoint RNEA pass writes to w->d_ct_wbar (f̄ext is a sum over stages; the contact pullback must not see the sum), then sct_backward_step.
template <typename T>
int sav_backward_step(rbd_ws* w, int32_t B, int layout, const T* q0, const T* v0, const void* tau, const void* fext, double dt, bool fresh, void* q_bar,
                      void* v_bar, void* tau_bar, void* fext_bar, const SavContact* C = nullptr) {
  const rbd_model* m = w->model;
  const SavBufs<T> b = sav_bufs<T>(w);
  const int32_t* jl = (const int32_t*)w->d_sav_joints.p;
  const Layout Li{B, 1};
  int st;
  if (!fresh && (st = sav_value_step<T>(w, B, layout, q0, v0, tau, fext, dt, 2, nullptr, nullptr, C))) return st;
  for (int stage = 3; stage >= 0; --stage) {
    const T* qs = stage == 0 ? q0 : b.qs[stage - 1];
    const T* vs = stage == 0 ? v0 : b.vs[stage - 1];
    if (C && !(fresh && stage == 3) && (st = sct_contact<T>(w, B, *C, stage, qs, vs, fext))) return st;
    if (!(fresh && stage == 3) && (st = tan_dynamics_value<T>(w, B, layout, qs, vs, tau, C ? w->d_tw.p : fext, w->d_tan_vd.p))) return st;
    MkAdjArgs<T> S = sav_args<T>(w, B, layout, dt, stage);
    S.q0 = q0; S.qs = qs; S.vs = vs; S.accp = b.accp;
    S.qsb = (T*)q_bar; S.vsb = (T*)v_bar; S.q0b = b.q0b; S.v0b = b.v0b; S.vdb = b.vdb; S.apb = b.apb; S.avb = b.avb;
    HIP_TRY(launch_mk_stage_classes<T>(S, jl, w->sav_nn, jl + 3 * w->sav_nn, w->sav_nw, 1, w->stream));
    const ColOut<T> lam = ColOut<T>::single((T*)w->d_adj_lam.p, Li, m->nv);
    HIP_TRY(launch_tangent_solve<T>(m->nv, B, 0, 1, w->d_tan_L.p, Li, b.vdb, 0, lam, w->d_adj_x.p, w->stream));
    AdjArgs<T> A = adj_args<T>(w, B, layout, qs, vs, w->d_tan_vd.p, C ? w->d_tw.p : fext);
    A.lam = lam.a; A.Llam = Li;
    A.qbar = (T*)q_bar; A.vbar = (T*)v_bar; A.fbar = (T*)(C ? w->d_ct_wbar.p : fext_bar); A.lbar = (T*)tau_bar;
    A.sign = T(-1); A.accum = 1; A.fset = C ? 1 : 0;
    HIP_TRY(launch_adjoint_rnea<T>(w->tan, A, w->d_adj_scratch.p, w->adj_states, w->stream));
    if (C && (st = sct_backward_step<T>(w, B, layout, *C, stage, dt, qs, vs, q_bar, v_bar, fext_bar))) return st;
  }
  return RBD_OK;
}

// τ̄ and f̄ext are sums over every stage of every step: zero first (all of them when nothing moves)
int sav_zero_sums(rbd_ws* w, int32_t B, void* tau_bar, void* fext_bar) {
  if (tau_bar) HIP_TRY(hipMemsetAsync(tau_bar, 0, esize(w) * w->model->nv * B, w->stream));
  if (fext_bar) HIP_TRY(hipMemsetAsync(fext_bar, 0, esize(w) * 6 * w->model->nb * B, w->stream));
  return RBD_OK;
}

// nsteps steps forward (the step starts kept as `P` says; q, v advanced in place), then backward from the last step to the first.  co: the options of a call with
// contact (rbd_simulate_contact_vjp), whose slots hold (q, v, s) and whose friction state sx and cotangent sx_bar travel beside (q, v); NULL without.
template <typename T>
int sav_run(rbd_ws* w, int32_t B, int layout, void* q, void* v, const void* tau, const void* fext, double dt, int nsteps, SavPlan P, void* q_bar, void* v_bar,
            void* tau_bar, void* fext_bar, const Opts* co = nullptr, void* sx = nullptr, void* sx_bar = nullptr) {
  const rbd_model* m = w->model;
  const long nq = m->nq, nv = m->nv, ns = co ? 3L * m->ncp * m->nhs : 0, slot = (nq + nv + ns) * B;
  const size_t es = sizeof(T);
  T* ck = (T*)w->d_sav_ckpt.p;
  auto cq = [&](int i) { return ck + i * slot; };
  auto cv = [&](int i) { return ck + i * slot + nq * B; };
  auto cs = [&](int i) { return ck + i * slot + (nq + nv) * B; };
  auto keep = [&](int i, const void* qf, const void* vf) -> hipError_t {
    hipError_t e = hipMemcpyAsync(cq(i), qf, es * nq * B, hipMemcpyDeviceToDevice, w->stream);
    if (e == hipSuccess && co) e = hipMemcpyAsync(cs(i), sx, es * ns * B, hipMemcpyDeviceToDevice, w->stream);
    return e != hipSuccess ? e : hipMemcpyAsync(cv(i), vf, es * nv * B, hipMemcpyDeviceToDevice, w->stream);
  };
  SavContact ct{co, nullptr, nullptr, sx_bar};
  auto contact = [&](const void* s0, void* sn) -> const SavContact* {  // (one step's friction state: from s0 to sn)
    if (!co) return nullptr;
    ct.s0 = s0; ct.sn = sn;
    return &ct;
  };
  int st;
  if (P.S == 1) {  // every start kept: step s from slot s into slot s + 1 (the last into (q, v))
    HIP_TRY(keep(0, q, v));
    for (int s = 0; s < nsteps; ++s) {
      const bool last = s == nsteps - 1;
      if ((st = sav_value_step<T>(w, B, layout, cq(s), cv(s), tau, fext, dt, 3, last ? (T*)q : cq(s + 1), last ? (T*)v : cv(s + 1),
                                  contact(cs(s), last ? (T*)sx : cs(s + 1)))))
        return st;
    }
  } else {  // every S-th start kept, (q, v) stepped in place
    for (int s = 0; s < nsteps; ++s) {
      if (s % P.S == 0) HIP_TRY(keep(s / P.S, q, v));
      if ((st = sav_value_step<T>(w, B, layout, (T*)q, (T*)v, tau, fext, dt, 3, (T*)q, (T*)v, contact(sx, sx)))) return st;
    }
  }
  bool fresh = P.S == 1;  // (the forward pass's last step left its stage states, sums and stage-3 factor)
  for (int g = P.K - 1; g >= 0; --g) {
    const int s0 = g * P.S, n = std::min(P.S, nsteps - s0);
    auto start = [&](int j) { return j == 0 ? g : P.K + j - 1; };  // (the slot of step s0 + j's start)
    for (int j = 1; j < n; ++j)  // the segment's starts recomputed from its kept one
      if ((st = sav_value_step<T>(w, B, layout, cq(start(j - 1)), cv(start(j - 1)), tau, fext, dt, 3, cq(start(j)), cv(start(j)),
                                  contact(cs(start(j - 1)), cs(start(j))))))
        return st;
    for (int j = n - 1; j >= 0; --j) {
      if ((st = sav_backward_step<T>(w, B, layout, cq(start(j)), cv(start(j)), tau, fext, dt, fresh, q_bar, v_bar, tau_bar, fext_bar, contact(cs(start(j)), nullptr))))
        return st;
      fresh = false;
    }
  }
  return RBD_OK;
}

// ---- forward mode through soft contact (header 700 addition): rbd_contact_dynamics_jvp, rbd_dynamics_contact_jvp, rbd_dynamics_contact_derivatives -------------
// the first call of a workspace allocates what tan_ensure and ct_ensure do, the right-hand sides for max(ntan, nq + nv + ns) directions (the Jacobians' columns:
// a JVP call after a derivatives call allocates nothing); a JVP call with more directions than any before allocates again
int ctj_ensure(rbd_ws* w, int ntan) {
  const rbd_model* m = w->model;
  if (int st = tan_ensure(w, std::max(ntan, m->nq + m->nv + 3 * m->ncp * m->nhs))) return st;
  return ct_ensure(w);
}

template <typename T> TanContactArgs<T> ctj_args(rbd_ws* w, int32_t B, int layout, int ntan, const void* s, const void* ds) {
  const rbd_model* m = w->model;
  const long ns = 3L * m->ncp * m->nhs;
  TanContactArgs<T> C{};
  C.C = w->ctm;
  C.s = (const T*)s; C.ds = (const T*)ds;
  C.Ls = layout_of(layout, ns, B); C.Lds = layout_of(layout, ns * ntan, B);
  C.gs0 = m->nq + m->nv;
  C.dcw = ColOut<T>::single(nullptr, Layout{0, 0}, 6 * m->nb);
  C.dsdot = C.dsout = ColOut<T>::single(nullptr, Layout{0, 0}, (int)ns);
  return C;
}

// the forward contact launches on a copy of s (the caller's is const; contact_kernel resets the pairs outside): the total wrenches fext + contact into
// w->d_tw, ṡ into sdot_out (nullable); then v̇ and the factor of M at those wrenches (tan_dynamics_value), when v̇ or a tangent of it is asked for
template <typename T>
int ctj_values(rbd_ws* w, int32_t B, const Opts& o, const void* q, const void* v, const void* s, const void* tau, const void* fext, void* sdot_out, void* vd) {
  const rbd_model* m = w->model;
  int st;
  HIP_TRY(hipMemcpyAsync(w->d_ct_s.p, s, sizeof(T) * 3 * m->ncp * m->nhs * B, hipMemcpyDeviceToDevice, w->stream));
  if ((st = run_contact(w, B, o, q, v, w->d_ct_s.p, sdot_out, fext, nullptr, w->d_tw.p))) return st;
  if (vd && m->nv > 0 && (st = tan_dynamics_value<T>(w, B, o.layout, q, v, tau, w->d_tw.p, vd))) return st;
  return RBD_OK;
}

template <typename T>
int ctj_dyn_jvp(rbd_ws* w, int32_t B, int32_t ntan, const Opts& o, const void* q, const void* v, const void* s, const void* tau, const void* fext, const void* dq,
                const void* dv, const void* ds, const void* dtau, const void* dfext, void* vdot_out, void* sdot_out, void* dvdot_out, void* dsdot_out,
                void* ds_out_out) {
  const rbd_model* m = w->model;
  const bool solve = dvdot_out && m->nv > 0;
  void* vd = vdot_out ? vdot_out : (solve ? w->d_tan_vd.p : nullptr);
  int st;
  if ((vd || sdot_out || solve) && (st = ctj_values<T>(w, B, o, q, v, s, tau, fext, sdot_out, vd))) return st;
  if (!solve && !dsdot_out && !ds_out_out) return RBD_OK;
  // M dv̇ = dτ − ∂ID(q, v, v̇)·(dq, dv, 0, d(total wrenches)): the pass at the TOTAL wrenches, the contact step adding the contact wrenches' tangents
  TanArgs<T> A = tan_args<T>(w, B, o.layout, ntan, q, v, solve ? vd : nullptr, solve ? w->d_tw.p : nullptr);
  A.dq = (const T*)dq; A.dv = (const T*)dv; A.dfext = solve ? (const T*)dfext : nullptr;
  A.sign = T(-1);
  if (solve) { A.out.a = (T*)w->d_tan_rhs.p; A.out.La = Layout{B, 1}; A.dadd = (const T*)dtau; }
  TanContactArgs<T> C = ctj_args<T>(w, B, o.layout, ntan, s, ds);
  C.dsdot.a = (T*)dsdot_out; C.dsdot.La = C.Lds;
  C.dsout.a = (T*)ds_out_out; C.dsout.La = C.Lds;
  C.forward_only = solve ? 0 : 1;
  HIP_TRY(launch_tangent_contact_rnea<T>(w->tan, A, C, w->d_tan_scratch.p, w->tan_threads, w->stream));
  if (solve) {
    const ColOut<T> out = ColOut<T>::single((T*)dvdot_out, A.Ldv, m->nv);
    HIP_TRY(launch_tangent_solve<T>(m->nv, B, 0, ntan, w->d_tan_L.p, Layout{B, 1}, w->d_tan_rhs.p, 0, out, w->d_tan_x.p, w->stream));
  }
  return RBD_OK;
}

// The columns of (q; v) in one pass (ColOut splits over two buffers), those of s in a second one with g0 = nq + nv; the right-hand sides of column g at g, so
// that each block's solve writes its own Jacobian.  A block none of whose outputs is asked for is not launched; no wrench sweep and no solve without dvdot_*.
template <typename T>
int ctj_dyn_derivs(rbd_ws* w, int32_t B, const Opts& o, const void* q, const void* v, const void* s, const void* tau, const void* fext, void* vdot_out,
                   void* sdot_out, void* dvdot_dq, void* dvdot_dv, void* dvdot_ds, void* dvdot_dtau, void* dsdot_dq, void* dsdot_dv, void* dsdot_ds) {
  const rbd_model* m = w->model;
  const int nq = m->nq, nv = m->nv, ns = 3 * m->ncp * m->nhs, layout = o.layout;
  const bool mv = nv > 0;
  const bool any_vd = mv && (dvdot_dq || dvdot_dv || dvdot_ds || dvdot_dtau);
  void* vd = vdot_out ? vdot_out : (any_vd ? w->d_tan_vd.p : nullptr);
  int st;
  if ((vd || sdot_out || any_vd) && (st = ctj_values<T>(w, B, o, q, v, s, tau, fext, sdot_out, vd))) return st;
  const Layout Li{B, 1};
  auto jac = [&](int rows, int cols) { return layout_of(layout, (long)rows * cols, B); };
  // one block of unit directions g0 … g1 − 1; out / dso: where the block's dv̇ and dṡ columns go
  auto block = [&](int g0, int g1, bool solve, const ColOut<T>& out, const ColOut<T>& dso) -> int {
    if (g1 <= g0) return RBD_OK;
    TanArgs<T> A = tan_args<T>(w, B, layout, g1 - g0, q, v, solve ? vd : nullptr, solve ? w->d_tw.p : nullptr);
    A.unit = 1; A.g0 = g0;
    A.sign = T(-1);
    if (solve) { A.out.a = (T*)w->d_tan_rhs.p; A.out.La = Li; }
    TanContactArgs<T> C = ctj_args<T>(w, B, layout, g1 - g0, s, nullptr);
    C.dsdot = dso;
    C.forward_only = solve ? 0 : 1;
    HIP_TRY(launch_tangent_contact_rnea<T>(w->tan, A, C, w->d_tan_scratch.p, w->tan_threads, w->stream));
    if (solve) HIP_TRY(launch_tangent_solve<T>(nv, B, g0, g1 - g0, w->d_tan_L.p, Li, w->d_tan_rhs.p, 0, out, w->d_tan_x.p, w->stream));
    return RBD_OK;
  };
  {
    const bool wq = (mv && dvdot_dq) || dsdot_dq, wv = (mv && dvdot_dv) || dsdot_dv;
    const ColOut<T> out{(T*)dvdot_dq, jac(nv, nq), (T*)dvdot_dv, jac(nv, nv), nq, nv};
    const ColOut<T> dso{(T*)dsdot_dq, jac(ns, nq), (T*)dsdot_dv, jac(ns, nv), nq, ns};
    if ((st = block(wq ? 0 : nq, wv ? nq + nv : nq, mv && (dvdot_dq || dvdot_dv), out, dso))) return st;
  }
  if ((mv && dvdot_ds) || dsdot_ds) {  // (columns < nq + nv do not occur in this block: the first buffer of its ColOuts is never asked for)
    const ColOut<T> out{nullptr, Layout{0, 0}, (T*)dvdot_ds, jac(nv, ns), nq + nv, nv};
    const ColOut<T> dso{nullptr, Layout{0, 0}, (T*)dsdot_ds, jac(ns, ns), nq + nv, ns};
    if ((st = block(nq + nv, nq + nv + ns, mv && dvdot_ds, out, dso))) return st;
  }
  if (mv && dvdot_dtau) {  // ∂v̇/∂τ = M⁻¹ (the contact wrenches do not depend on τ): the solve against the identity
    const ColOut<T> out = ColOut<T>::single((T*)dvdot_dtau, jac(nv, nv), nv);
    HIP_TRY(launch_tangent_solve<T>(nv, B, 0, nv, w->d_tan_L.p, Li, nullptr, 1, out, w->d_tan_x.p, w->stream));
  }
  return RBD_OK;
}

// ---- derivatives of simulate steps (header 700 additions) -----------------------------------------------------------------------------------------------
enum : long { SIM_TAN_CAP = 1L << 31 };  // bytes of the simulate tangent buffers at most: more directions run as several passes

// values of the friction state per state (0 without contact points or environment: the entry points with contact in their name refuse such a mechanism)
size_t sim_ns(const rbd_model* m) { return 3 * (size_t)m->ncp * (size_t)m->nhs; }
// tangents per (direction, state) of one pass: initial dq, dv, dτ; the stage state's dq, dv; the running sums' two; dv̇; with contact the step's ds₀, the
// stage state's ds, the running sum's tangent and dṡ
size_t sim_tan_per_dir(const rbd_model* m) { return 2 * (size_t)m->nq + 6 * (size_t)m->nv + 4 * sim_ns(m); }
// RBD_TUNE sim_tan_bytes=<n>: one pass's tangents in n bytes instead of the cap, at least one chunk of directions (tests reach the several-passes path at
// small sizes)
int sim_pass_width(rbd_ws* w, int ndir) {
  const long per = (long)(esize(w) * sim_tan_per_dir(w->model) * (size_t)w->max_batch);
  const int N = tangent_chunk((int)esize(w));
  bool has;
  const long knob = tune("sim_tan_bytes", 0, &has);
  const long cap = std::max<long>(N, (has ? std::max(0L, knob) : (long)SIM_TAN_CAP) / std::max<long>(1, per) / N * N);
  return (int)std::min<long>(ndir, cap);
}
// the first call of a workspace allocates, and one whose pass is wider than any before; nothing else allocates.  With contact: what rbd_simulate_contact_vjp's
// value route does too (sct_ensure), and the saved initial s beside the saved (q, v)
int sim_ensure(rbd_ws* w, int width, bool contact = false) {
  const rbd_model* m = w->model;
  const size_t es = esize(w), B = (size_t)w->max_batch;
  int st;
  if ((st = tan_ensure(w, width))) return st;
  if (contact && (st = sct_ensure(w))) return st;
  if ((st = ensure(w->d_sim_val, es * B * (4 * (size_t)m->nq + 6 * (size_t)m->nv + sim_ns(m))))) return st;
  if (width > w->sim_tan_w) {
    if ((st = ensure(w->d_sim_tan, es * B * sim_tan_per_dir(m) * (size_t)width))) return st;
    w->sim_tan_w = width;
  }
  return RBD_OK;
}

// nsteps steps of the RK4 integrator with ndir directions carried along, in passes of at most sim_tan_w directions.  JVP (jac == false): the caller's
// dq, dv (in/out), dτ, dfext, ndir directions in the call's layout.  Jacobians (jac): the columns g0 … g0 + ndir − 1 of [∂x⁺/∂x  ∂x⁺/∂τ], unit directions
// made on the device, written to dxdx (columns < nx) and dxdtau.  Each stage: dynamics! at the stage state (CRBA + Cholesky, the factor in the workspace),
// the tangent RNEA (sign −1, dadd = dτ), the solve for dv̇, the stage kernel.
// With contact (C; rbd_simulate_contact_jvp, rbd_simulate_contact_step_derivatives): x = (q; v; s), the friction state s (in/out) and its tangents ds (the
// JVP's, in/out) beside (q, v).  Each stage: the forward contact launch at the stage state (sct_contact: a copy of s₀ at stage 0, the total wrenches into
// w->d_tw, ṡ into the workspace), dynamics! at those wrenches, tangent_contact_rnea_kernel in place of the plain pass (the pass's ds in, dṡ out), the solve,
// the (q, v) stage kernel as it is, then tangent_contact_stage_kernel for s — values and tangents in one launch, where the value route has
// contact_stage_value_kernel.  Three launches more per stage than without (the contact launch's two, the friction state's stage kernel).  NULL: no launch differs.
struct SimTanContact { const Opts* o; void* s; void* ds; };
template <typename T>
int sim_tan_run(rbd_ws* w, int32_t B, int layout, void* q, void* v, const void* tau, const void* fext, double dt, int nsteps, int ndir, bool jac, int g0,
                void* dq, void* dv, const void* dtau, const void* dfext, void* dxdx, void* dxdtau, const SimTanContact* C = nullptr) {
  const rbd_model* m = w->model;
  const int nq = m->nq, nv = m->nv, ns = C ? (int)sim_ns(m) : 0, nx = nq + nv + ns, W = w->sim_tan_w;
  const long Bm = w->max_batch;
  const size_t es = sizeof(T);
  const Layout Lq = layout_of(layout, nq, B), Lv = layout_of(layout, nv, B), Ls = layout_of(layout, ns, B), Li{B, 1};
  const Layout Ldq = layout_of(layout, (long)nq * ndir, B), Ldv = layout_of(layout, (long)nv * ndir, B), Ldf = layout_of(layout, 6L * m->nb * ndir, B);
  const Layout Lds = layout_of(layout, (long)ns * ndir, B);
  // values (the call's layout): q0, the two stage-state buffers, the saved initial state; v0, two stage states, the running sum, the saved state
  T* val = (T*)w->d_sim_val.p;
  T *q0 = val, *qa = q0 + nq * Bm, *qb = qa + nq * Bm, *qi = qb + nq * Bm, *v0 = qi + nq * Bm, *va = v0 + nv * Bm, *vb = va + nv * Bm;
  T *accp = vb + nv * Bm, *accv = accp + nv * Bm, *vi = accv + nv * Bm, *si = vi + nv * Bm;
  // tangents of one pass, batch-innermost
  T* tb = (T*)w->d_sim_tan.p;
  const long tw = (long)W * Bm;
  T *dq0 = tb, *dv0 = dq0 + nq * tw, *dd0 = dv0 + nv * tw, *dqs = dd0 + nv * tw, *dvs = dqs + nq * tw, *dap = dvs + nv * tw, *dav = dap + nv * tw,
    *dvd = dav + nv * tw;
  T *ds0 = dvd + nv * tw, *dss = ds0 + ns * tw, *dsa = dss + ns * tw, *dsd = dsa + ns * tw;  // (with contact)
  auto col = [&](T* p, int n) { return ColOut<T>::single(p, Li, n); };
  auto user = [&](const void* p, Layout L, int n) { return ColOut<T>::single((T*)p, L, n); };
  const int npass = (ndir + W - 1) / W;
  if (npass > 1) {
    HIP_TRY(hipMemcpyAsync(qi, q, es * nq * B, hipMemcpyDeviceToDevice, w->stream));
    HIP_TRY(hipMemcpyAsync(vi, v, es * nv * B, hipMemcpyDeviceToDevice, w->stream));
    if (C) HIP_TRY(hipMemcpyAsync(si, C->s, es * ns * B, hipMemcpyDeviceToDevice, w->stream));
  }
  for (int p = 0; p < npass; ++p) {
    const int e0 = p * W, nw = std::min(W, ndir - e0);
    if (p > 0) {  // every pass starts from the caller's state (each one writes the same state after the step)
      HIP_TRY(hipMemcpyAsync(q, qi, es * nq * B, hipMemcpyDeviceToDevice, w->stream));
      HIP_TRY(hipMemcpyAsync(v, vi, es * nv * B, hipMemcpyDeviceToDevice, w->stream));
      if (C) HIP_TRY(hipMemcpyAsync(C->s, si, es * ns * B, hipMemcpyDeviceToDevice, w->stream));
    }
    // (the τ unit columns follow those of x: at nq + nv without contact, as before)
    HIP_TRY(launch_tangent_mk_load<T>(B, nw, nq, nv, jac ? g0 + e0 : e0, jac ? 1 : 0, nx, user(dq, Ldq, nq), user(dv, Ldv, nv), user(dtau, Ldv, nv),
                                      col(dq0, nq), col(dv0, nv), col(dd0, nv), w->stream));
    if (C) HIP_TRY(launch_tangent_contact_load<T>(B, nw, ns, jac ? g0 + e0 : e0, jac ? 1 : 0, nq + nv, user(C->ds, Lds, ns), col(ds0, ns), w->stream));
    for (int step = 0; step < nsteps; ++step) {
      HIP_TRY(hipMemcpyAsync(q0, q, es * nq * B, hipMemcpyDeviceToDevice, w->stream));
      HIP_TRY(hipMemcpyAsync(v0, v, es * nv * B, hipMemcpyDeviceToDevice, w->stream));
      for (int stage = 0; stage < 4; ++stage) {
        // the stage state: (q, v) at stage 0, then qa/va, qb/vb, qa/va; stage 3 writes the state after the step over (q, v)
        T* qs = stage == 0 ? (T*)q : (stage == 2 ? qb : qa);
        T* vs = stage == 0 ? (T*)v : (stage == 2 ? vb : va);
        int st;
        const SavContact sc{C ? C->o : nullptr, C ? C->s : nullptr, nullptr, nullptr};  // (sct_contact reads the options and the step's start)
        if (C && (st = sct_contact<T>(w, B, sc, stage, qs, vs, fext))) return st;
        const void* wr = C ? w->d_tw.p : fext;  // the wrenches dynamics! and the tangent pass see: with contact the total ones
        if ((st = tan_dynamics_value<T>(w, B, layout, qs, vs, tau, wr, w->d_tan_vd.p))) return st;
        TanArgs<T> A = tan_args<T>(w, B, layout, nw, qs, vs, w->d_tan_vd.p, wr);
        A.dq = stage == 0 ? dq0 : dqs; A.dv = stage == 0 ? dv0 : dvs; A.Ldq = Li; A.Ldv = Li;
        A.dfext = (!jac && dfext) ? (const T*)dfext + (long)e0 * 6 * m->nb * Ldf.sk : nullptr; A.Ldf = Ldf;
        A.out.a = (T*)w->d_tan_rhs.p; A.out.La = Li;
        A.sign = T(-1); A.dadd = dd0;
        if (C) {
          TanContactArgs<T> K = ctj_args<T>(w, B, layout, nw, sct_stage_state<T>(w, stage), stage == 0 ? ds0 : dss);
          K.Lds = Li;
          K.dsdot = col(dsd, ns);
          HIP_TRY(launch_tangent_contact_rnea<T>(w->tan, A, K, w->d_tan_scratch.p, w->tan_threads, w->stream));
        } else {
          HIP_TRY(launch_tangent_rnea<T>(w->tan, A, w->d_tan_scratch.p, w->tan_threads, w->stream));
        }
        HIP_TRY(launch_tangent_solve<T>(nv, B, 0, nw, w->d_tan_L.p, Li, w->d_tan_rhs.p, 0, col(dvd, nv), w->d_tan_x.p, w->stream));
        MkTanArgs<T> S{};
        S.B = B; S.ntan = nw; S.nb = w->tan.nb; S.stage = stage; S.dt = (T)dt; S.tbl = w->tan.tbl;
        S.q0 = q0; S.v0 = v0; S.qs = qs; S.vs = vs; S.vd = (const T*)w->d_tan_vd.p; S.accp = accp; S.accv = accv;
        S.qn = stage == 3 ? (T*)q : (stage == 1 ? qb : qa);
        S.vn = stage == 3 ? (T*)v : (stage == 1 ? vb : va);
        S.Lq = Lq; S.Lv = Lv;
        S.dq0 = col(dq0, nq); S.dv0 = col(dv0, nv); S.dqs = stage == 0 ? S.dq0 : col(dqs, nq); S.dvs = stage == 0 ? S.dv0 : col(dvs, nv);
        S.dvd = col(dvd, nv); S.daccp = col(dap, nv); S.daccv = col(dav, nv);
        S.ocol = 0; S.ovrow = 0;
        if (stage < 3) {
          S.oq = col(dqs, nq); S.ov = col(dvs, nv);
        } else if (step < nsteps - 1) {  // (the next step's base point, in place)
          S.oq = S.dq0; S.ov = S.dv0;
        } else if (jac) {
          S.oq = S.ov = ColOut<T>{(T*)dxdx, layout_of(layout, (long)nx * nx, B), (T*)dxdtau, layout_of(layout, (long)nx * nv, B), nx, nx};
          S.ocol = g0 + e0; S.ovrow = nq;
        } else {
          S.oq = user(dq, Ldq, nq); S.ov = user(dv, Ldv, nv); S.ocol = e0;
        }
        HIP_TRY(launch_tangent_mk_stage<T>(S, w->stream));
        if (!C) continue;
        const SctBufs<T> b = sct_bufs<T>(w);
        CtTanStageArgs<T> F{};
        F.B = B; F.ntan = nw; F.ns = ns; F.stage = stage; F.dt = (T)dt;
        F.s0 = (const T*)C->s; F.sd = b.sdot; F.acc = b.acc; F.sn = stage == 3 ? (T*)C->s : b.ss[stage];
        F.Ls = Ls;
        F.ds0 = col(ds0, ns); F.dsd = col(dsd, ns); F.dacc = col(dsa, ns);
        F.ocol = S.ocol; F.orow = 0;
        if (stage < 3) {
          F.os = col(dss, ns);
        } else if (step < nsteps - 1) {
          F.os = F.ds0;
        } else if (jac) {  // (rows nq + nv … of the columns the (q, v) stage kernel writes the rows above of)
          F.os = S.oq; F.orow = nq + nv;
        } else {
          F.os = user(C->ds, Lds, ns);
        }
        HIP_TRY(launch_tangent_contact_stage<T>(F, w->stream));
      }
    }
  }
  return RBD_OK;
}
}  // namespace

extern "C" {

int rbd_inverse_dynamics_jvp(rbd_ws_t* w, int32_t B, int32_t ntan, const void* q, const void* v, const void* vdot, const void* fext, const void* dq,
                             const void* dv, const void* dvdot, const void* dfext, void* tau_out, void* dtau_out, const rbd_opts_t* opts) {
  Opts o;
  int st = tan_check(w, B, opts, &o);
  if (st != RBD_OK) return st;
  const rbd_model* m = w->model;
  if (ntan <= 0 || missing(q, m->nq) || missing(v, m->nv) || missing(vdot, m->nv)) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0 || m->nv == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  if ((st = tan_ensure(w, ntan))) return st;
  Timed t(w);
  w->last_kernel = "tangent_rnea_kernel";
  return by_dtype(w->dtype, [&](auto t) { return tan_id_jvp<decltype(t)>(w, B, ntan, o.layout, q, v, vdot, fext, dq, dv, dvdot, dfext, tau_out, dtau_out); });
}

int rbd_dynamics_jvp(rbd_ws_t* w, int32_t B, int32_t ntan, const void* q, const void* v, const void* tau, const void* fext, const void* dq, const void* dv,
                     const void* dtau, const void* dfext, void* vdot_out, void* dvdot_out, const rbd_opts_t* opts) {
  Opts o;
  int st = tan_check(w, B, opts, &o);
  if (st != RBD_OK) return st;
  const rbd_model* m = w->model;
  if (ntan <= 0 || missing(q, m->nq) || missing(v, m->nv)) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0 || m->nv == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  if ((st = tan_ensure(w, ntan))) return st;
  Timed t(w);
  w->last_kernel = "tangent_rnea_kernel + tangent_solve_kernel";
  return by_dtype(w->dtype, [&](auto t) { return tan_dyn_jvp<decltype(t)>(w, B, ntan, o.layout, q, v, tau, fext, dq, dv, dtau, dfext, vdot_out, dvdot_out); });
}

int rbd_inverse_dynamics_derivatives(rbd_ws_t* w, int32_t B, const void* q, const void* v, const void* vdot, const void* fext, void* tau_out, void* dtau_dq,
                                     void* dtau_dv, void* M_out, const rbd_opts_t* opts) {
  Opts o;
  int st = tan_check(w, B, opts, &o);
  if (st != RBD_OK) return st;
  const rbd_model* m = w->model;
  if (missing(q, m->nq) || missing(v, m->nv) || missing(vdot, m->nv)) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0 || m->nv == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  if ((st = tan_ensure(w, m->nq + m->nv))) return st;
  Timed t(w);
  w->last_kernel = "tangent_rnea_kernel";
  return by_dtype(w->dtype, [&](auto t) { return tan_id_derivs<decltype(t)>(w, B, o.layout, q, v, vdot, fext, tau_out, dtau_dq, dtau_dv, M_out); });
}

int rbd_dynamics_derivatives(rbd_ws_t* w, int32_t B, const void* q, const void* v, const void* tau, const void* fext, void* vdot_out, void* dvdot_dq,
                             void* dvdot_dv, void* dvdot_dtau, const rbd_opts_t* opts) {
  Opts o;
  int st = tan_check(w, B, opts, &o);
  if (st != RBD_OK) return st;
  const rbd_model* m = w->model;
  if (missing(q, m->nq) || missing(v, m->nv)) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0 || m->nv == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  if ((st = tan_ensure(w, m->nq + m->nv))) return st;
  Timed t(w);
  w->last_kernel = "tangent_rnea_kernel + tangent_solve_kernel";
  return by_dtype(w->dtype, [&](auto t) { return tan_dyn_derivs<decltype(t)>(w, B, o.layout, q, v, tau, fext, vdot_out, dvdot_dq, dvdot_dv, dvdot_dtau); });
}

int rbd_simulate_jvp(rbd_ws_t* w, int32_t B, int32_t ntan, void* q, void* v, const void* tau, const void* fext, double dt, int32_t nsteps, void* dq,
                     void* dv, const void* dtau, const void* dfext, const rbd_opts_t* opts) {
  Opts o;
  int st = tan_check(w, B, opts, &o);
  if (st != RBD_OK) return st;
  if (ntan <= 0 || !(dt > 0) || nsteps < 0 || !q || !v || !dq || !dv) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0 || nsteps == 0 || w->model->nv == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  const int width = sim_pass_width(w, ntan);
  if ((st = sim_ensure(w, width))) return st;
  Timed t(w);
  w->last_kernel = "tangent_rnea_kernel + tangent_solve_kernel + tangent_mk_stage_kernel";
  return by_dtype(w->dtype, [&](auto t) {
    return sim_tan_run<decltype(t)>(w, B, o.layout, q, v, tau, fext, dt, nsteps, ntan, false, 0, dq, dv, dtau, dfext, nullptr, nullptr);
  });
}

int rbd_simulate_step_derivatives(rbd_ws_t* w, int32_t B, void* q, void* v, const void* tau, const void* fext, double dt, void* dx_dx, void* dx_dtau,
                                  const rbd_opts_t* opts) {
  Opts o;
  int st = tan_check(w, B, opts, &o);
  if (st != RBD_OK) return st;
  const rbd_model* m = w->model;
  if (!(dt > 0) || !q || !v) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0 || m->nv == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  // the columns asked for: those of ∂x⁺/∂x (0 … nx − 1), then those of ∂x⁺/∂τ (a pass of one column that writes nowhere when neither is)
  const int nx = m->nq + m->nv, g0 = dx_dx ? 0 : nx, g1 = dx_dtau ? nx + m->nv : nx, ncol = std::max(1, g1 - g0);
  const int width = sim_pass_width(w, std::max(ncol, nx + m->nv));  // (allocated for every column: a call with the other output allocates nothing)
  if ((st = sim_ensure(w, width))) return st;
  Timed t(w);
  w->last_kernel = "tangent_rnea_kernel + tangent_solve_kernel + tangent_mk_stage_kernel";
  return by_dtype(w->dtype, [&](auto t) {
    return sim_tan_run<decltype(t)>(w, B, o.layout, q, v, tau, fext, dt, 1, ncol, true, g0, nullptr, nullptr, nullptr, nullptr, dx_dx, dx_dtau);
  });
}

int rbd_inverse_dynamics_vjp(rbd_ws_t* w, int32_t B, const void* q, const void* v, const void* vdot, const void* fext, const void* tau_bar, void* tau_out,
                             void* q_bar, void* v_bar, void* vdot_bar, void* fext_bar, const rbd_opts_t* opts) {
  Opts o;
  int st = tan_check(w, B, opts, &o);
  if (st != RBD_OK) return st;
  const rbd_model* m = w->model;
  if (missing(q, m->nq) || missing(v, m->nv) || missing(vdot, m->nv) || missing(tau_bar, m->nv)) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0 || m->nv == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  if ((st = adj_ensure(w))) return st;
  Timed t(w);
  w->last_kernel = "adjoint_rnea_kernel";
  return by_dtype(w->dtype, [&](auto t) { return adj_id_vjp<decltype(t)>(w, B, o.layout, q, v, vdot, fext, tau_bar, tau_out, q_bar, v_bar, vdot_bar, fext_bar); });
}

int rbd_dynamics_vjp(rbd_ws_t* w, int32_t B, const void* q, const void* v, const void* tau, const void* fext, const void* vdot_bar, void* vdot_out,
                     void* q_bar, void* v_bar, void* tau_bar, void* fext_bar, const rbd_opts_t* opts) {
  Opts o;
  int st = tan_check(w, B, opts, &o);
  if (st != RBD_OK) return st;
  const rbd_model* m = w->model;
  if (missing(q, m->nq) || missing(v, m->nv) || missing(vdot_bar, m->nv)) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0 || m->nv == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  if ((st = adj_ensure(w))) return st;
  Timed t(w);
  w->last_kernel = "tangent_solve_kernel + adjoint_rnea_kernel";
  return by_dtype(w->dtype, [&](auto t) { return adj_dyn_vjp<decltype(t)>(w, B, o.layout, q, v, tau, fext, vdot_bar, vdot_out, q_bar, v_bar, tau_bar, fext_bar); });
}

int rbd_simulate_vjp(rbd_ws_t* w, int32_t B, void* q, void* v, const void* tau, const void* fext, double dt, int32_t nsteps, void* q_bar, void* v_bar,
                     void* tau_bar, void* fext_bar, const rbd_opts_t* opts) {
  Opts o;
  int st = tan_check(w, B, opts, &o);
  if (st != RBD_OK) return st;
  if (!(dt > 0) || nsteps < 0 || !q || !v || !q_bar || !v_bar) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0) return RBD_OK;
  const rbd_model* m = w->model;
  const size_t es = esize(w);
  HIP_TRY(hipSetDevice(w->device));
  if ((st = sav_zero_sums(w, B, tau_bar, fext_bar))) return st;
  if (nsteps == 0 || m->nv == 0) return RBD_OK;
  if ((st = sav_ensure(w))) return st;
  const size_t slot_bytes = es * (size_t)(m->nq + m->nv) * B;
  const SavPlan P = sav_plan(slot_bytes, nsteps);
  if ((st = ensure(w->d_sav_ckpt, slot_bytes * P.slots))) return st;  // (only a call that needs more room than any before)
  Timed t(w);
  w->last_kernel = "value_mk_stage_kernel + adjoint_mk_stage_kernel + tangent_solve_kernel + adjoint_rnea_kernel";
  return by_dtype(w->dtype, [&](auto t) { return sav_run<decltype(t)>(w, B, o.layout, q, v, tau, fext, dt, nsteps, P, q_bar, v_bar, tau_bar, fext_bar); });
}

// ---- point kinematics (rbd_point.hpp): rbd_workspace_set_points, rbd_point_kinematics, rbd_point_kinematics_vjp -------------------------------------------------
int rbd_workspace_set_points(rbd_ws_t* w, int32_t npoints, const int32_t* body, const double* r) {
  if (!w || npoints < 0 || (npoints > 0 && (!body || !r))) return RBD_ERR_INVALID_ARGUMENT;
  const rbd_model* m = w->model;
  if (m->nloops > 0) return RBD_ERR_HAS_LOOPS;
  for (int k = 0; k < npoints; ++k)
    if (body[k] < 0 || body[k] >= m->nb) return RBD_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(w->device));
  HIP_TRY(hipStreamSynchronize(w->stream));  // (a call still running reads the tables replaced here)
  w->d_pt_i.reset(); w->d_pt_r.reset();
  w->pts = PointPlan{};
  if (npoints == 0) return RBD_OK;
  int st;
  if ((st = tan_tables(w))) return st;
  return point_plan_upload(w, npoints, body, r, w->d_pt_i, w->d_pt_r, &w->pts);
}

int rbd_point_kinematics(rbd_ws_t* w, int32_t B, const void* q, const void* v, const void* vdot, void* pos, void* vel, void* acc, void* jac,
                         const rbd_opts_t* opts) {
  Opts o;
  int st = begin_call(w, B, opts, kAnySize, &o);
  if (st != RBD_OK) return st;
  const rbd_model* m = w->model;
  if (m->nloops > 0) return RBD_ERR_HAS_LOOPS;
  if (w->pts.np == 0 || !q || ((vel || acc) && missing(v, m->nv))) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  const long P = w->pts.np;
  const size_t row = esize(w) * B;
  HostIO io(w, o.memory);
  const void *dq, *dv, *dvd;
  void *dpos, *dvel, *dacc, *djac;
  if ((st = io.in(q, row * m->nq, &dq)) || (st = io.in(v, row * m->nv, &dv)) || (st = io.in(vdot, row * m->nv, &dvd)) || (st = io.out(pos, row * 3 * P, &dpos)) ||
      (st = io.out(vel, row * 3 * P, &dvel)) || (st = io.out(acc, row * 3 * P, &dacc)) || (st = io.out(jac, row * 3 * P * m->nv, &djac)))
    return st;
  w->last_kernel = "point_kin_kernel";
  {
    Timed t(w);
    HIP_TRY(by_dtype(w->dtype, [&](auto t) {
      using T = decltype(t);
      PointArgs<T> A{};
      A.B = B; A.q = (const T*)dq; A.v = (const T*)dv; A.vdot = (const T*)dvd;
      A.Lq = layout_of(o.layout, m->nq, B); A.Lv = layout_of(o.layout, m->nv, B); A.L3 = layout_of(o.layout, 3 * P, B); A.Lj = layout_of(o.layout, 3 * P * m->nv, B);
      A.pos = (T*)dpos; A.vel = (T*)dvel; A.acc = (T*)dacc; A.jac = (T*)djac;
      return launch_point_kin<T>(w->tan, w->pts, A, w->stream);
    }));
  }
  return io.finish();
}

int rbd_point_kinematics_vjp(rbd_ws_t* w, int32_t B, const void* q, const void* v, const void* pos_bar, const void* vel_bar, void* q_bar, void* v_bar,
                             const rbd_opts_t* opts) {
  Opts o;
  int st = tan_check(w, B, opts, &o);
  if (st != RBD_OK) return st;
  const rbd_model* m = w->model;
  if (w->pts.np == 0 || missing(q, m->nq) || missing(v, m->nv) || (!pos_bar && !vel_bar)) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0 || (!q_bar && !v_bar)) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  if ((st = adj_scratch_ensure(w))) return st;
  Timed t(w);
  w->last_kernel = "point_adjoint_kernel";
  HIP_TRY(by_dtype(w->dtype, [&](auto t) {
    using T = decltype(t);
    AdjArgs<T> A = adj_args<T>(w, B, o.layout, q, v, nullptr, nullptr);
    A.qbar = (T*)q_bar; A.vbar = (T*)v_bar;
    PointAdjArgs<T> C{(const T*)pos_bar, (const T*)vel_bar, layout_of(o.layout, 3L * w->pts.np, B)};
    return launch_point_adjoint<T>(w->tan, w->pts, A, C, w->d_adj_scratch.p, w->adj_states, w->stream);
  }));
  return RBD_OK;
}

// ---- reverse mode through soft contact (rbd_contact.hpp): rbd_contact_dynamics_vjp, rbd_dynamics_contact_vjp ----------------------------------------------------
static int contact_vjp_scope(rbd_ws* w, int32_t B, const rbd_opts_t* opts, Opts* o) {
  if (int st = begin_call(w, B, opts, kAnySize, o)) return st;
  if (w->model->nloops > 0) return RBD_ERR_HAS_LOOPS;
  if (w->model->ncp == 0 || w->model->nhs == 0) return RBD_ERR_INVALID_ARGUMENT;  // (as rbd_contact_dynamics: use rbd_dynamics_vjp)
  if (o->memory != RBD_MEM_DEVICE) return RBD_ERR_UNSUPPORTED;
  return RBD_OK;
}

int rbd_contact_dynamics_vjp(rbd_ws_t* w, int32_t B, const void* q, const void* v, const void* s, const void* cw_bar, const void* sdot_bar, const void* s_out_bar,
                             void* q_bar, void* v_bar, void* s_bar, const rbd_opts_t* opts) {
  Opts o;
  int st = contact_vjp_scope(w, B, opts, &o);
  if (st != RBD_OK) return st;
  if (!q || !v || !s || (!cw_bar && !sdot_bar && !s_out_bar)) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  if ((st = ct_ensure(w))) return st;
  Timed t(w);
  w->last_kernel = "contact_adjoint_kernel + point_adjoint_kernel";
  if ((st = run_contact_kinematics(w, B, o, q, v))) return st;
  return by_dtype(w->dtype, [&](auto t) { return ct_adjoint<decltype(t)>(w, B, o.layout, q, v, s, cw_bar, sdot_bar, s_out_bar, q_bar, v_bar, s_bar, 0); });
}

int rbd_dynamics_contact_vjp(rbd_ws_t* w, int32_t B, const void* q, const void* v, const void* s, const void* tau, const void* fext, const void* vdot_bar,
                             const void* sdot_bar, const void* s_out_bar, void* vdot_out, void* sdot_out, void* q_bar, void* v_bar, void* s_bar, void* tau_bar,
                             void* fext_bar, const rbd_opts_t* opts) {
  Opts o;
  int st = contact_vjp_scope(w, B, opts, &o);
  if (st != RBD_OK) return st;
  if (!q || !v || !s || (!vdot_bar && !sdot_bar && !s_out_bar)) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  if ((st = ct_ensure(w))) return st;
  const rbd_model* m = w->model;
  const size_t es = esize(w);
  Timed t(w);
  w->last_kernel = "tangent_solve_kernel + adjoint_rnea_kernel + contact_adjoint_kernel + point_adjoint_kernel";
  // the forward contact launch resets the friction state of the points outside: on a copy (s is the caller's, const); total wrenches into the workspace
  HIP_TRY(hipMemcpyAsync(w->d_ct_s.p, s, es * 3 * m->ncp * m->nhs * B, hipMemcpyDeviceToDevice, w->stream));
  if ((st = run_contact(w, B, o, q, v, w->d_ct_s.p, sdot_out, fext, nullptr, w->d_tw.p))) return st;
  return by_dtype(w->dtype, [&](auto t) -> int {
    using T = decltype(t);
    int st;
    const void* wbar = nullptr;
    if (vdot_bar) {
      // v̇ as a function of the total wrenches: its f̄ext is their cotangent — the caller's fext_bar (totalwrenches = fext + contactwrenches) and the contact
      // wrenches' — and q̄, v̄ are the dynamics' share, which the contact points' is added to
      void* wb = fext_bar ? fext_bar : ((q_bar || v_bar || s_bar) ? w->d_ct_wbar.p : nullptr);
      if ((st = adj_dyn_vjp<T>(w, B, o.layout, q, v, tau, w->d_tw.p, vdot_bar, vdot_out, q_bar, v_bar, tau_bar, wb))) return st;
      wbar = wb;
    } else {  // no cotangent of v̇: τ and fext reach ṡ and s_out through nothing
      if (vdot_out && (st = tan_dynamics_value<T>(w, B, o.layout, q, v, tau, w->d_tw.p, vdot_out))) return st;
      if (tau_bar) HIP_TRY(hipMemsetAsync(tau_bar, 0, es * m->nv * B, w->stream));
      if (fext_bar) HIP_TRY(hipMemsetAsync(fext_bar, 0, es * 6 * m->nb * B, w->stream));
    }
    return ct_adjoint<T>(w, B, o.layout, q, v, s, wbar, sdot_bar, s_out_bar, q_bar, v_bar, s_bar, vdot_bar ? 1 : 0);
  });
}

// ---- forward mode through soft contact: rbd_contact_dynamics_jvp, rbd_dynamics_contact_jvp, rbd_dynamics_contact_derivatives ------------------------------------
int rbd_contact_dynamics_jvp(rbd_ws_t* w, int32_t B, int32_t ntan, const void* q, const void* v, const void* s, const void* dq, const void* dv, const void* ds,
                             void* dcw_out, void* dsdot_out, void* ds_out_out, const rbd_opts_t* opts) {
  Opts o;
  int st = contact_vjp_scope(w, B, opts, &o);
  if (st != RBD_OK) return st;
  if (ntan <= 0 || !q || !v || !s) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  if ((st = ctj_ensure(w, ntan))) return st;
  Timed t(w);
  w->last_kernel = "tangent_contact_rnea_kernel";
  if (!dcw_out && !dsdot_out && !ds_out_out) return RBD_OK;
  return by_dtype(w->dtype, [&](auto t) -> int {
    using T = decltype(t);
    // the tangent pass in its forward-only mode: no v̇, no wrenches, no wrench sweep
    TanArgs<T> A = tan_args<T>(w, B, o.layout, ntan, q, v, nullptr, nullptr);
    A.dq = (const T*)dq; A.dv = (const T*)dv;
    TanContactArgs<T> C = ctj_args<T>(w, B, o.layout, ntan, s, ds);
    C.dcw.a = (T*)dcw_out; C.dcw.La = A.Ldf;
    C.dsdot.a = (T*)dsdot_out; C.dsdot.La = C.Lds;
    C.dsout.a = (T*)ds_out_out; C.dsout.La = C.Lds;
    C.forward_only = 1;
    HIP_TRY(launch_tangent_contact_rnea<T>(w->tan, A, C, w->d_tan_scratch.p, w->tan_threads, w->stream));
    return RBD_OK;
  });
}

int rbd_dynamics_contact_jvp(rbd_ws_t* w, int32_t B, int32_t ntan, const void* q, const void* v, const void* s, const void* tau, const void* fext, const void* dq,
                             const void* dv, const void* ds, const void* dtau, const void* dfext, void* vdot_out, void* sdot_out, void* dvdot_out,
                             void* dsdot_out, void* ds_out_out, const rbd_opts_t* opts) {
  Opts o;
  int st = contact_vjp_scope(w, B, opts, &o);
  if (st != RBD_OK) return st;
  if (ntan <= 0 || !q || !v || !s) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  if ((st = ctj_ensure(w, ntan))) return st;
  Timed t(w);
  w->last_kernel = "contact_kernel + tangent_contact_rnea_kernel + tangent_solve_kernel";
  return by_dtype(w->dtype, [&](auto t) {
    return ctj_dyn_jvp<decltype(t)>(w, B, ntan, o, q, v, s, tau, fext, dq, dv, ds, dtau, dfext, vdot_out, sdot_out, dvdot_out, dsdot_out, ds_out_out);
  });
}

int rbd_dynamics_contact_derivatives(rbd_ws_t* w, int32_t B, const void* q, const void* v, const void* s, const void* tau, const void* fext, void* vdot_out,
                                     void* sdot_out, void* dvdot_dq, void* dvdot_dv, void* dvdot_ds, void* dvdot_dtau, void* dsdot_dq, void* dsdot_dv,
                                     void* dsdot_ds, const rbd_opts_t* opts) {
  Opts o;
  int st = contact_vjp_scope(w, B, opts, &o);
  if (st != RBD_OK) return st;
  if (!q || !v || !s) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0) return RBD_OK;
  HIP_TRY(hipSetDevice(w->device));
  if ((st = ctj_ensure(w, 1))) return st;
  Timed t(w);
  w->last_kernel = "contact_kernel + tangent_contact_rnea_kernel + tangent_solve_kernel";
  return by_dtype(w->dtype, [&](auto t) {
    return ctj_dyn_derivs<decltype(t)>(w, B, o, q, v, s, tau, fext, vdot_out, sdot_out, dvdot_dq, dvdot_dv, dvdot_ds, dvdot_dtau, dsdot_dq, dsdot_dv, dsdot_ds);
  });
}

int rbd_simulate_contact_vjp(rbd_ws_t* w, int32_t B, void* q, void* v, void* s, const void* tau, const void* fext, double dt, int32_t nsteps, void* q_bar,
                             void* v_bar, void* s_bar, void* tau_bar, void* fext_bar, const rbd_opts_t* opts) {
  Opts o;
  int st = contact_vjp_scope(w, B, opts, &o);
  if (st != RBD_OK) return st;
  if (!(dt > 0) || nsteps < 0 || !q || !v || !s || !q_bar || !v_bar || !s_bar) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0) return RBD_OK;
  const rbd_model* m = w->model;
  if (m->nv == 0) return RBD_ERR_UNSUPPORTED;  // (contact points on a mechanism that cannot move: nothing to differentiate)
  const size_t es = esize(w);
  HIP_TRY(hipSetDevice(w->device));
  if ((st = sav_zero_sums(w, B, tau_bar, fext_bar))) return st;
  if (nsteps == 0) return RBD_OK;
  if ((st = sct_ensure(w))) return st;
  const size_t slot_bytes = es * (size_t)(m->nq + m->nv + 3 * m->ncp * m->nhs) * B;
  const SavPlan P = sav_plan(slot_bytes, nsteps);
  if ((st = ensure(w->d_sav_ckpt, slot_bytes * P.slots))) return st;  // (only a call that needs more room than any before)
  Timed t(w);
  w->last_kernel = "value_mk_stage_kernel + contact_kernel + contact_stage_value_kernel + adjoint_mk_stage_kernel + tangent_solve_kernel + adjoint_rnea_kernel + "
                   "contact_stage_adjoint_kernel + point_adjoint_kernel";
  return by_dtype(w->dtype, [&](auto t) {
    return sav_run<decltype(t)>(w, B, o.layout, q, v, tau, fext, dt, nsteps, P, q_bar, v_bar, tau_bar, fext_bar, &o, s, s_bar);
  });
}

// ---- forward mode through simulate steps with soft contact: rbd_simulate_contact_jvp, rbd_simulate_contact_step_derivatives -----------------------------------
static const char* const kSimContactTanKernels =
    "contact_kernel + tangent_contact_rnea_kernel + tangent_solve_kernel + tangent_mk_stage_kernel + tangent_contact_stage_kernel";

int rbd_simulate_contact_jvp(rbd_ws_t* w, int32_t B, int32_t ntan, void* q, void* v, void* s, const void* tau, const void* fext, double dt, int32_t nsteps,
                             void* dq, void* dv, void* ds, const void* dtau, const void* dfext, const rbd_opts_t* opts) {
  Opts o;
  int st = contact_vjp_scope(w, B, opts, &o);
  if (st != RBD_OK) return st;
  if (ntan <= 0 || !(dt > 0) || nsteps < 0 || !q || !v || !s || !dq || !dv || !ds) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0 || nsteps == 0) return RBD_OK;
  if (w->model->nv == 0) return RBD_ERR_UNSUPPORTED;  // (as rbd_simulate_contact_vjp: contact points on a mechanism that cannot move)
  HIP_TRY(hipSetDevice(w->device));
  const int width = sim_pass_width(w, ntan);
  if ((st = sim_ensure(w, width, true))) return st;
  Timed t(w);
  w->last_kernel = kSimContactTanKernels;
  const SimTanContact C{&o, s, ds};
  return by_dtype(w->dtype, [&](auto t) {
    return sim_tan_run<decltype(t)>(w, B, o.layout, q, v, tau, fext, dt, nsteps, ntan, false, 0, dq, dv, dtau, dfext, nullptr, nullptr, &C);
  });
}

int rbd_simulate_contact_step_derivatives(rbd_ws_t* w, int32_t B, void* q, void* v, void* s, const void* tau, const void* fext, double dt, void* dx_dx,
                                          void* dx_dtau, const rbd_opts_t* opts) {
  Opts o;
  int st = contact_vjp_scope(w, B, opts, &o);
  if (st != RBD_OK) return st;
  const rbd_model* m = w->model;
  if (!(dt > 0) || !q || !v || !s) return RBD_ERR_INVALID_ARGUMENT;
  if (B == 0) return RBD_OK;
  if (m->nv == 0) return RBD_ERR_UNSUPPORTED;
  HIP_TRY(hipSetDevice(w->device));
  // the columns asked for, as rbd_simulate_step_derivatives with nx = nq + nv + ns: those of ∂x⁺/∂x, then those of ∂x⁺/∂τ
  const int nx = m->nq + m->nv + (int)sim_ns(m), g0 = dx_dx ? 0 : nx, g1 = dx_dtau ? nx + m->nv : nx, ncol = std::max(1, g1 - g0);
  const int width = sim_pass_width(w, std::max(ncol, nx + m->nv));
  if ((st = sim_ensure(w, width, true))) return st;
  Timed t(w);
  w->last_kernel = kSimContactTanKernels;
  const SimTanContact C{&o, s, nullptr};
  return by_dtype(w->dtype, [&](auto t) {
    return sim_tan_run<decltype(t)>(w, B, o.layout, q, v, tau, fext, dt, 1, ncol, true, g0, nullptr, nullptr, nullptr, nullptr, dx_dx, dx_dtau, &C);
  });
}

}  // extern "C"
