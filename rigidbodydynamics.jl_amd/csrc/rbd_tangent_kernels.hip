// rbd_tangent_kernels.hip — the kernels of the derivative entry points (rbd_inverse_dynamics_jvp, rbd_dynamics_jvp, rbd_inverse_dynamics_derivatives,
// rbd_dynamics_derivatives, rbd_simulate_jvp, rbd_simulate_step_derivatives, rbd_inverse_dynamics_vjp, rbd_dynamics_vjp, rbd_simulate_vjp, rbd_point_kinematics_vjp, rbd_contact_dynamics_jvp, rbd_dynamics_contact_jvp,
// rbd_dynamics_contact_derivatives, rbd_simulate_contact_jvp, rbd_simulate_contact_step_derivatives): the tangent RNEA
// (rbd_tangent.hpp) with one thread per (state, chunk of TAN_CHUNK directions) and its variant with the soft-contact step between the sweeps (rbd_contact.hpp),
// the multi-right-hand-side triangular solve of dynamics! tangents against the
// Cholesky factor of M, the tangent of the integrator's stage map (rbd_tangent_mk.hpp) with one thread per (state, joint, chunk) and of the friction state's
// (rbd_contact.hpp contact_stage_value) with one thread per (state, value of s, chunk), the adjoint RNEA
// (rbd_adjoint.hpp) with one thread per state, and the stage map's values and pullback (rbd_adjoint_mk.hpp) with one thread per (state, joint) of a
// joint class.  Compiled with -ffinite-math-only -fno-signed-zeros (build.sh): the zero
// tangents of the mechanism's constants fold out of the products.
#include "rbd_tangent.hpp"
#include "rbd_adjoint.hpp"
#include "rbd_tangent_mk.hpp"
#include "rbd_adjoint_mk.hpp"
#include "rbd_point.hpp"
#include "rbd_contact.hpp"
#include "rbd_internal.hpp"

namespace rbd {

template <typename T> struct TanChunk;
template <> struct TanChunk<double> { enum { N = 2 }; };
template <> struct TanChunk<float> { enum { N = 4 }; };

size_t tangent_scratch_elems_per_thread(const BigModel& M, int es) {
  const int N = es == 8 ? (int)TanChunk<double>::N : (int)TanChunk<float>::N;
  return (size_t)TAN_FIELDS * (N + 1) * (size_t)M.nb;
}
int tangent_chunk(int es) { return es == 8 ? (int)TanChunk<double>::N : (int)TanChunk<float>::N; }

// `total` threads in slabs of the scratch's size (at most `max` each): launch(first, count) per slab
template <typename F> hipError_t launch_slabs(long total, long max, F launch) {
  for (long i0 = 0; i0 < total; i0 += max) {
    launch(i0, total - i0 < max ? total - i0 : max);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// threads t0 … t0 + nt − 1 of the B · nchunks (state, chunk) pairs; the scratch holds nt threads
template <typename T, int N>
__global__ __launch_bounds__(64) void tangent_rnea_kernel(BigModel M, TanArgs<T> A, long t0, long nt, T* __restrict__ scratch) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nt) return;
  const long t = t0 + slot;
  const int chunk = (int)(t / A.B);
  const long st = t - (long)chunk * A.B;
  tangent_rnea_state<T, N>(M, A, st, chunk, scratch, nt, slot);
}

template <typename T>
hipError_t launch_tangent_rnea(const BigModel& M, const TanArgs<T>& A, void* scratch, long max_threads, hipStream_t s) {
  constexpr int N = TanChunk<T>::N;
  const long nchunks = (A.ntan + N - 1) / N;
  return launch_slabs(nchunks * A.B, max_threads, [&](long t0, long nt) {
    hipLaunchKernelGGL((tangent_rnea_kernel<T, N>), dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, s, M, A, t0, nt, (T*)scratch);
  });
}

// the contact variant (rbd_contact.hpp tangent_contact_state; rbd_contact_dynamics_jvp, rbd_dynamics_contact_jvp, rbd_dynamics_contact_derivatives): the same
// threads, slabs and scratch; an instantiation of its own, so that tangent_rnea_kernel stays what it was
template <typename T, int N>
__global__ __launch_bounds__(64) void tangent_contact_rnea_kernel(BigModel M, TanArgs<T> A, TanContactArgs<T> C, long t0, long nt, T* __restrict__ scratch) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nt) return;
  const long t = t0 + slot;  // (the thread of the CALL, not of the slab: its chunk picks the directions whose dsdot / ds_out / dcw rows it writes)
  const int chunk = (int)(t / A.B);
  const long st = t - (long)chunk * A.B;
  tangent_contact_state<T, N>(M, A, C, st, chunk, scratch, nt, slot);
}

template <typename T>
hipError_t launch_tangent_contact_rnea(const BigModel& M, const TanArgs<T>& A, const TanContactArgs<T>& C, void* scratch, long max_threads, hipStream_t s) {
  constexpr int N = TanChunk<T>::N;
  const long nchunks = (A.ntan + N - 1) / N;
  return launch_slabs(nchunks * A.B, max_threads, [&](long t0, long nt) {
    hipLaunchKernelGGL((tangent_contact_rnea_kernel<T, N>), dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, s, M, A, C, t0, nt, (T*)scratch);
  });
}

// columns c0 … c0 + ncol − 1 of every state, thread = (c − c0) · B + state: x = M⁻¹ rhs_c (identity: e_c) with the factor L (layout Ll)
template <typename T, int NVP>
__global__ __launch_bounds__(64) void tangent_solve_kernel(int nv, long B, int c0, int ncol, const T* __restrict__ L, Layout Ll, const T* __restrict__ rhs,
                                                           int identity, ColOut<T> out, T* __restrict__ xmem) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)ncol * B) return;
  const int c = c0 + (int)(t / B);
  const long st = t % B;
  if (NVP > 0) {
    T x[NVP > 0 ? NVP : 1];
    tri_solve_col<NVP>(nv, L, Ll, st, c, rhs, B, identity, out, x);
  } else {  // (more than 64 coordinates: the solution vector in a scratch of its own, batch-innermost)
    struct Mem { T* p; long B; __device__ T& operator[](int i) const { return p[(long)i * B]; } } x{xmem + t, (long)ncol * B};
    tri_solve_col<0>(nv, L, Ll, st, c, rhs, B, identity, out, x);
  }
}

template <typename T>
hipError_t launch_tangent_solve(int nv, long B, int c0, int ncol, const void* L, Layout Ll, const void* rhs, int identity, const ColOut<T>& out, void* xmem,
                                hipStream_t s) {
  const long total = (long)ncol * B;
  if (total == 0) return hipSuccess;
  const dim3 grid((unsigned)((total + 63) / 64));
#define RBD_TSOLVE(NVP)                                                                                                                               \
  if (nv <= NVP) {                                                                                                                                    \
    hipLaunchKernelGGL((tangent_solve_kernel<T, NVP>), grid, dim3(64), 0, s, nv, B, c0, ncol, (const T*)L, Ll, (const T*)rhs, identity, out, (T*)nullptr); \
    return hipGetLastError();                                                                                                                         \
  }
  RBD_TSOLVE(8) RBD_TSOLVE(16) RBD_TSOLVE(32) RBD_TSOLVE(48) RBD_TSOLVE(64)
#undef RBD_TSOLVE
  if (!xmem) return hipErrorInvalidValue;
  hipLaunchKernelGGL((tangent_solve_kernel<T, 0>), grid, dim3(64), 0, s, nv, B, c0, ncol, (const T*)L, Ll, (const T*)rhs, identity, out, (T*)xmem);
  return hipGetLastError();
}

// ∂τ/∂v̇ = M as the full square: the upper triangle from the lower one CRBA wrote
template <typename T> __global__ __launch_bounds__(256) void symmetrize_kernel(int nv, long B, T* __restrict__ M, Layout Lm) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n2 = (long)nv * nv;
  if (e >= n2 * B) return;
  long st, k;
  if (Lm.sk == 1) { st = e / n2; k = e - st * n2; } else { k = e / B; st = e - k * B; }
  const int col = (int)(k / nv), row = (int)(k - (long)col * nv);
  if (row < col) M[k * Lm.sk + layout_base(Lm, st)] = M[((long)row * nv + col) * Lm.sk + layout_base(Lm, st)];
}
template <typename T> hipError_t launch_symmetrize(int nv, long B, void* M, Layout Lm, hipStream_t s) {
  const long total = (long)nv * nv * B;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(symmetrize_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, nv, B, (T*)M, Lm);
  return hipGetLastError();
}

// ---- simulate tangents: one thread per (state, joint, chunk of N directions), thread = (chunk · nb + joint) · B + state ----------------------------------
template <typename T, int N>
__global__ __launch_bounds__(64) void tangent_mk_stage_kernel(MkTanArgs<T> A) {
  using D = Dual<T, N>;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nchunks = (A.ntan + N - 1) / N;
  if (t >= nchunks * A.nb * A.B) return;
  const long st = t % A.B, r = t / A.B;
  const int i = (int)(r % A.nb), chunk = (int)(r / A.nb);
  const int jt = A.tbl[4 * i + 1], qoff = A.tbl[4 * i + 2], voff = A.tbl[4 * i + 3];
  const int nqi = joint_nq<T>(jt), nvi = joint_nv(jt);
  if (nvi == 0) return;
  const int e0 = chunk * N;
  // value of row `row` (nullable: not needed by this thread) and the tangents of the chunk's directions (zero past the pass's directions)
  auto load = [&](const T* val, Layout L, const ColOut<T>& tan, int row) {
    D x(val ? val[(long)row * L.sk + layout_base(L, st)] : T(0));
#pragma unroll
    for (int j = 0; j < N; ++j) x.d[j] = e0 + j < A.ntan ? *tan.at(e0 + j, row, st) : T(0);
    return x;
  };
  D q0[7], qs[7], v0[6], vs[6], vd[6], ap[6], av[6], qn[7], vn[6];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    q0[k] = k < nqi ? load(A.q0, A.Lq, A.dq0, qoff + k) : D(T(0));
    qs[k] = k < nqi ? load(A.qs, A.Lq, A.dqs, qoff + k) : D(T(0));
  }
  // (the running sums: only chunk 0 reads and writes their values before the last stage, which reads them everywhere)
  const bool accval = A.stage == 3 || chunk == 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const bool in = k < nvi;
    v0[k] = in ? load(A.v0, A.Lv, A.dv0, voff + k) : D(T(0));
    vs[k] = in ? load(A.vs, A.Lv, A.dvs, voff + k) : D(T(0));
    vd[k] = in ? load(A.vd, A.Lv, A.dvd, voff + k) : D(T(0));
    ap[k] = in && A.stage > 0 ? load(accval ? A.accp : nullptr, A.Lv, A.daccp, voff + k) : D(T(0));
    av[k] = in && A.stage > 0 ? load(accval ? A.accv : nullptr, A.Lv, A.daccv, voff + k) : D(T(0));
  }
  tan_mk_stage_joint<T, N>(jt, A.stage, A.dt, q0, v0, qs, vs, vd, ap, av, qn, vn);
  auto store = [&](T* val, Layout L, const ColOut<T>& tan, int col0, int row, int trow, const D& x) {
    if (chunk == 0 && val) val[(long)row * L.sk + layout_base(L, st)] = x.v;
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (e0 + j < A.ntan)
        if (T* o = tan.at(col0 + e0 + j, trow, st)) *o = x.d[j];
  };
#pragma unroll
  for (int k = 0; k < 7; ++k)
    if (k < nqi) store(A.qn, A.Lq, A.oq, A.ocol, qoff + k, qoff + k, qn[k]);
#pragma unroll
  for (int k = 0; k < 6; ++k)
    if (k < nvi) {
      store(A.vn, A.Lv, A.ov, A.ocol, voff + k, A.ovrow + voff + k, vn[k]);
      if (A.stage < 3) {
        store(A.accp, A.Lv, A.daccp, 0, voff + k, voff + k, ap[k]);
        store(A.accv, A.Lv, A.daccv, 0, voff + k, voff + k, av[k]);
      }
    }
}

template <typename T> hipError_t launch_tangent_mk_stage(const MkTanArgs<T>& A, hipStream_t s) {
  constexpr int N = TanChunk<T>::N;
  const long total = (long)((A.ntan + N - 1) / N) * A.nb * A.B;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL((tangent_mk_stage_kernel<T, N>), dim3((unsigned)((total + 63) / 64)), dim3(64), 0, s, A);
  return hipGetLastError();
}

// the initial tangents of a pass of ncol directions (thread = direction · B + state): columns col0 … of the caller's (dq, dv, dτ) (nullable: zero), or
// with `unit` the unit vectors of the step Jacobians' columns — column g is e_g of (q; v) for g < nq + nv, and e_{g − tau0} of τ for g ≥ tau0 (tau0 = nq + nv;
// with the friction state's columns between, nq + nv + ns)
template <typename T>
__global__ __launch_bounds__(256) void tangent_mk_load_kernel(long B, int ncol, int nq, int nv, int col0, int unit, int tau0, ColOut<T> sq, ColOut<T> sv,
                                                              ColOut<T> sd, ColOut<T> dq, ColOut<T> dv, ColOut<T> dd) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)ncol * B) return;
  const int e = (int)(t / B), g = col0 + e;
  const long st = t % B;
  auto src = [&](const ColOut<T>& s, int r) -> T { const T* p = s.at(g, r, st); return p ? *p : T(0); };
  for (int r = 0; r < nq; ++r) *dq.at(e, r, st) = unit ? T(g == r ? 1 : 0) : src(sq, r);
  for (int r = 0; r < nv; ++r) {
    *dv.at(e, r, st) = unit ? T(g == nq + r ? 1 : 0) : src(sv, r);
    *dd.at(e, r, st) = unit ? T(g == tau0 + r ? 1 : 0) : src(sd, r);
  }
}

template <typename T>
hipError_t launch_tangent_mk_load(long B, int ncol, int nq, int nv, int col0, int unit, int tau0, const ColOut<T>& sq, const ColOut<T>& sv,
                                  const ColOut<T>& sd, const ColOut<T>& dq, const ColOut<T>& dv, const ColOut<T>& dd, hipStream_t s) {
  const long total = (long)ncol * B;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(tangent_mk_load_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, B, ncol, nq, nv, col0, unit, tau0, sq, sv, sd, dq, dv, dd);
  return hipGetLastError();
}

// ---- simulate tangents with soft contact: the friction state through the tableau, one thread per (state, value of s, chunk of N directions), thread =
// (chunk · ns + row) · B + state.  contact_stage_value on Dual<T, N> (rbd_contact.hpp): values and tangents of a stage in one launch (it stands where
// contact_stage_value_kernel does on the value route).  Elementwise: every internal buffer is read and written contiguously over the state index.
template <typename T, int N>
__global__ __launch_bounds__(64) void tangent_contact_stage_kernel(CtTanStageArgs<T> A) {
  using D = Dual<T, N>;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nchunks = (A.ntan + N - 1) / N;
  if (t >= nchunks * A.ns * A.B) return;
  const long st = t % A.B, r = t / A.B;
  const int row = (int)(r % A.ns), chunk = (int)(r / A.ns);
  const int e0 = chunk * N;
  const long vo = (long)row * A.Ls.sk + layout_base(A.Ls, st);
  auto load = [&](const T* val, const ColOut<T>& tan) {
    D x(val ? val[vo] : T(0));
#pragma unroll
    for (int j = 0; j < N; ++j) x.d[j] = e0 + j < A.ntan ? *tan.at(e0 + j, row, st) : T(0);
    return x;
  };
  // (the tableau is linear: no tangent depends on a value, so only chunk 0, which writes the values, reads them — the other chunks must not, at stage 3,
  // where sn may be s0 itself; stage 0 reads neither the running sum's value nor its tangent)
  const bool rv = chunk == 0;
  const D s0 = load(rv ? A.s0 : nullptr, A.ds0), sd = load(rv ? A.sd : nullptr, A.dsd);
  D acc = A.stage > 0 ? load(rv ? A.acc : nullptr, A.dacc) : D(T(0)), sn;
  contact_stage_value<D>(A.stage, A.dt, s0, sd, acc, sn);
  auto store = [&](T* val, const ColOut<T>& tan, int col0, int trow, const D& x) {
    if (chunk == 0 && val) val[vo] = x.v;
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (e0 + j < A.ntan)
        if (T* o = tan.at(col0 + e0 + j, trow, st)) *o = x.d[j];
  };
  store(A.sn, A.os, A.ocol, A.orow + row, sn);
  if (A.stage < 3) store(A.acc, A.dacc, 0, row, acc);
}

template <typename T> hipError_t launch_tangent_contact_stage(const CtTanStageArgs<T>& A, hipStream_t s) {
  constexpr int N = TanChunk<T>::N;
  const long total = (long)((A.ntan + N - 1) / N) * A.ns * A.B;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL((tangent_contact_stage_kernel<T, N>), dim3((unsigned)((total + 63) / 64)), dim3(64), 0, s, A);
  return hipGetLastError();
}

// the friction state's initial tangents of a pass of ncol directions (thread = direction · B + state), beside tangent_mk_load_kernel's (dq, dv, dτ): columns
// col0 … of the caller's ds, or with `unit` the unit vectors — column g is e_{g − s0col} of s (s0col = nq + nv), zero for every other g
template <typename T>
__global__ __launch_bounds__(256) void tangent_contact_load_kernel(long B, int ncol, int ns, int col0, int unit, int s0col, ColOut<T> src, ColOut<T> ds) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)ncol * B) return;
  const int e = (int)(t / B), g = col0 + e;
  const long st = t % B;
  for (int r = 0; r < ns; ++r) *ds.at(e, r, st) = unit ? T(g == s0col + r ? 1 : 0) : *src.at(g, r, st);
}

template <typename T>
hipError_t launch_tangent_contact_load(long B, int ncol, int ns, int col0, int unit, int s0col, const ColOut<T>& src, const ColOut<T>& ds, hipStream_t s) {
  const long total = (long)ncol * B;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(tangent_contact_load_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, B, ncol, ns, col0, unit, s0col, src, ds);
  return hipGetLastError();
}

// ---- reverse mode: the adjoint RNEA, one thread per state ---------------------------------------------------------------------------------------------
size_t adjoint_scratch_elems_per_state(const BigModel& M) { return (size_t)ADJ_FIELDS * (size_t)M.nb; }

// states s0 … s0 + ns − 1; the scratch holds ns states
template <typename T>
__global__ __launch_bounds__(64) void adjoint_rnea_kernel(BigModel M, AdjArgs<T> A, long s0, long ns, T* __restrict__ scratch) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= ns) return;
  adjoint_rnea_state<T>(M, A, s0 + slot, scratch, ns, slot);
}

template <typename T> hipError_t launch_adjoint_rnea(const BigModel& M, const AdjArgs<T>& A, void* scratch, long max_states, hipStream_t s) {
  return launch_slabs(A.B, max_states, [&](long s0, long ns) {
    hipLaunchKernelGGL((adjoint_rnea_kernel<T>), dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, s, M, A, s0, ns, (T*)scratch);
  });
}

// the pullback of rbd_point_kinematics (rbd_point.hpp point_adjoint_state): one thread per state over the union of the points' paths, the same scratch and slabs
template <typename T>
__global__ __launch_bounds__(64) void point_adjoint_kernel(BigModel M, PointPlan P, AdjArgs<T> A, PointAdjArgs<T> C, long s0, long ns, T* __restrict__ scratch) {
  const long slot = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= ns) return;
  point_adjoint_state<T>(M, P, A, C, s0 + slot, scratch, ns, slot);
}

template <typename T>
hipError_t launch_point_adjoint(const BigModel& M, const PointPlan& P, const AdjArgs<T>& A, const PointAdjArgs<T>& C, void* scratch, long max_states, hipStream_t s) {
  return launch_slabs(A.B, max_states, [&](long s0, long ns) {
    hipLaunchKernelGGL((point_adjoint_kernel<T>), dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, s, M, P, A, C, s0, ns, (T*)scratch);
  });
}

// an n × B batch buffer of layout L copied batch-innermost (row r of state b at r B + b: the right-hand side tri_solve_col reads)
template <typename T> __global__ __launch_bounds__(256) void stage_rows_kernel(int n, long B, const T* __restrict__ x, Layout L, T* __restrict__ out) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)n * B) return;
  const long r = e / B, st = e - r * B;
  out[e] = x[r * L.sk + layout_base(L, st)];
}
template <typename T> hipError_t launch_stage_rows(int n, long B, const void* x, Layout L, void* out, hipStream_t s) {
  const long total = (long)n * B;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(stage_rows_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, n, B, (const T*)x, L, (T*)out);
  return hipGetLastError();
}

// ---- simulate VJPs: the stage map's values and its pullback, one thread per (joint of a class, state), thread = j · B + state ---------------------------
// Two instantiations per kernel: WIDE = false for the 1-coordinate joints (no Dual code: the registers of a revolute joint), WIDE = true for the planar and
// quaternion joints.  Values are read in the call's layout, the cotangents of the stage state in the caller's (Lqb, Lvb), the rest batch-innermost.
template <typename T, bool WIDE>
__global__ __launch_bounds__(64) void value_mk_stage_kernel(MkAdjArgs<T> A) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)A.nj * A.B) return;
  const long st = t % A.B;
  const int j = (int)(t / A.B);
  const int jt = A.jl[3 * j], qoff = A.jl[3 * j + 1], voff = A.jl[3 * j + 2];
  constexpr int KQ = WIDE ? 7 : 2, KV = WIDE ? 6 : 1;
  const int nqi = joint_nq<T>(jt), nvi = joint_nv(jt);
  auto at = [&](T* p, Layout L, int row) -> T& { return p[(long)row * L.sk + layout_base(L, st)]; };
  T q0[7], qs[7], qn[7], v0[6], vs[6], vd[6], ap[6], av[6], vn[6];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const bool in = k < KQ && k < nqi;
    q0[k] = in ? at((T*)A.q0, A.Lq, qoff + k) : T(0);
    qs[k] = in ? at((T*)A.qs, A.Lq, qoff + k) : T(0);
    qn[k] = T(0);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const bool in = k < KV && k < nvi;
    v0[k] = in ? at((T*)A.v0, A.Lv, voff + k) : T(0);
    vs[k] = in ? at((T*)A.vs, A.Lv, voff + k) : T(0);
    vd[k] = in ? at((T*)A.vd, A.Lv, voff + k) : T(0);
    ap[k] = in && A.stage > 0 ? at(A.accp, A.Lv, voff + k) : T(0);
    av[k] = in && A.stage > 0 ? at(A.accv, A.Lv, voff + k) : T(0);
    vn[k] = T(0);
  }
  mk_stage_value_joint<T, WIDE>(jt, A.stage, A.dt, q0, v0, qs, vs, vd, ap, av, qn, vn);
#pragma unroll
  for (int k = 0; k < KQ; ++k)
    if (k < nqi) at(A.qn, A.Lq, qoff + k) = qn[k];
#pragma unroll
  for (int k = 0; k < KV; ++k)
    if (k < nvi) {
      at(A.vn, A.Lv, voff + k) = vn[k];
      if (A.stage < 3) { at(A.accp, A.Lv, voff + k) = ap[k]; at(A.accv, A.Lv, voff + k) = av[k]; }
    }
}

template <typename T, bool WIDE>
__global__ __launch_bounds__(64) void adjoint_mk_stage_kernel(MkAdjArgs<T> A) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)A.nj * A.B) return;
  const long st = t % A.B;
  const int j = (int)(t / A.B);
  const int jt = A.jl[3 * j], qoff = A.jl[3 * j + 1], voff = A.jl[3 * j + 2];
  constexpr int KQ = WIDE ? 7 : 2, KV = WIDE ? 6 : 1;
  const int nqi = joint_nq<T>(jt), nvi = joint_nv(jt), stage = A.stage;
  auto at = [&](T* p, Layout L, int row) -> T& { return p[(long)row * L.sk + layout_base(L, st)]; };
  auto li = [&](T* p, int row) -> T& { return p[(long)row * A.B + st]; };
  T q0[7], qs[7], qnb[7], q0b[7], qsb[7], vs[6], ap[6], vnb[6], apb[6], avb[6], v0b[6], vsb[6], vdb[6];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const bool in = k < KQ && k < nqi;
    q0[k] = in ? at((T*)A.q0, A.Lq, qoff + k) : T(0);
    qs[k] = in ? at((T*)A.qs, A.Lq, qoff + k) : T(0);
    qnb[k] = in ? at(A.qsb, A.Lqb, qoff + k) : T(0);
    q0b[k] = in && stage < 3 ? li(A.q0b, qoff + k) : T(0);
    qsb[k] = T(0);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const bool in = k < KV && k < nvi;
    vs[k] = in ? at((T*)A.vs, A.Lv, voff + k) : T(0);
    ap[k] = in && stage == 3 ? at(A.accp, A.Lv, voff + k) : T(0);
    vnb[k] = in ? at(A.vsb, A.Lvb, voff + k) : T(0);
    apb[k] = in && stage < 3 ? li(A.apb, voff + k) : T(0);
    avb[k] = in && stage < 3 ? li(A.avb, voff + k) : T(0);
    v0b[k] = in && stage < 3 ? li(A.v0b, voff + k) : T(0);
    vsb[k] = T(0); vdb[k] = T(0);
  }
  adj_mk_stage_joint<T, WIDE>(jt, stage, A.dt, q0, qs, vs, ap, qnb, vnb, apb, avb, q0b, v0b, qsb, vsb, vdb);
#pragma unroll
  for (int k = 0; k < KQ; ++k)
    if (k < nqi) {
      if (stage > 0) {
        at(A.qsb, A.Lqb, qoff + k) = qsb[k];
        li(A.q0b, qoff + k) = q0b[k];
      } else {  // (the stage-0 state is the base point itself)
        at(A.qsb, A.Lqb, qoff + k) = q0b[k] + qsb[k];
      }
    }
#pragma unroll
  for (int k = 0; k < KV; ++k)
    if (k < nvi) {
      li(A.vdb, voff + k) = vdb[k];
      if (stage > 0) {
        at(A.vsb, A.Lvb, voff + k) = vsb[k];
        li(A.v0b, voff + k) = v0b[k];
      } else {
        at(A.vsb, A.Lvb, voff + k) = v0b[k] + vsb[k];
      }
      if (stage == 3) { li(A.apb, voff + k) = apb[k]; li(A.avb, voff + k) = avb[k]; }
    }
}

// one stage for both joint classes (narrow: nn joints at jn, wide: nw at jw); `adjoint` picks the pullback, else the value map
template <typename T> hipError_t launch_mk_stage_classes(MkAdjArgs<T> A, const int32_t* jn, int nn, const int32_t* jw, int nw, int adjoint, hipStream_t s) {
  for (int c = 0; c < 2; ++c) {
    A.jl = c ? jw : jn;
    A.nj = c ? nw : nn;
    const long total = (long)A.nj * A.B;
    if (total == 0) continue;
    const dim3 grid((unsigned)((total + 63) / 64));
    if (adjoint) {
      if (c) hipLaunchKernelGGL((adjoint_mk_stage_kernel<T, true>), grid, dim3(64), 0, s, A);
      else hipLaunchKernelGGL((adjoint_mk_stage_kernel<T, false>), grid, dim3(64), 0, s, A);
    } else {
      if (c) hipLaunchKernelGGL((value_mk_stage_kernel<T, true>), grid, dim3(64), 0, s, A);
      else hipLaunchKernelGGL((value_mk_stage_kernel<T, false>), grid, dim3(64), 0, s, A);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

#define RBD_TAN_INST(T)                                                                                                                                    \
  template hipError_t launch_tangent_rnea<T>(const BigModel&, const TanArgs<T>&, void*, long, hipStream_t);                                              \
  template hipError_t launch_tangent_contact_rnea<T>(const BigModel&, const TanArgs<T>&, const TanContactArgs<T>&, void*, long, hipStream_t);             \
  template hipError_t launch_tangent_solve<T>(int, long, int, int, const void*, Layout, const void*, int, const ColOut<T>&, void*, hipStream_t);          \
  template hipError_t launch_symmetrize<T>(int, long, void*, Layout, hipStream_t);                                                                   \
  template hipError_t launch_tangent_mk_stage<T>(const MkTanArgs<T>&, hipStream_t);                                                                     \
  template hipError_t launch_tangent_mk_load<T>(long, int, int, int, int, int, int, const ColOut<T>&, const ColOut<T>&, const ColOut<T>&, const ColOut<T>&,   \
                                                const ColOut<T>&, const ColOut<T>&, hipStream_t);                                                        \
  template hipError_t launch_tangent_contact_stage<T>(const CtTanStageArgs<T>&, hipStream_t);                                                          \
  template hipError_t launch_tangent_contact_load<T>(long, int, int, int, int, int, const ColOut<T>&, const ColOut<T>&, hipStream_t);                    \
  template hipError_t launch_adjoint_rnea<T>(const BigModel&, const AdjArgs<T>&, void*, long, hipStream_t);                                              \
  template hipError_t launch_point_adjoint<T>(const BigModel&, const PointPlan&, const AdjArgs<T>&, const PointAdjArgs<T>&, void*, long, hipStream_t);         \
  template hipError_t launch_stage_rows<T>(int, long, const void*, Layout, void*, hipStream_t);                                                        \
  template hipError_t launch_mk_stage_classes<T>(MkAdjArgs<T>, const int32_t*, int, const int32_t*, int, int, hipStream_t);
RBD_TAN_INST(double)
RBD_TAN_INST(float)

}  // namespace rbd
