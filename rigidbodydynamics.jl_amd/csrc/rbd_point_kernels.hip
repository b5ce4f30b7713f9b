// rbd_point_kernels.hip — the forward kernel of rbd_point_kinematics (rbd_point.hpp point_kin_state): one thread per (point, state), thread = point · B + state
// (coalesced across the batch in SOA, as tangent_mk_stage_kernel).  Everything a thread carries lives in registers: no scratch, no LDS.  The pullback's kernel
// (point_adjoint_kernel) is with the adjoint pass it reuses, in rbd_tangent_kernels.hip.
#include "rbd_point.hpp"
#include "rbd_internal.hpp"

namespace rbd {

template <typename T>
__global__ __launch_bounds__(64) void point_kin_kernel(BigModel M, PointPlan P, PointArgs<T> A) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)P.np * A.B) return;
  const int pt = (int)(t / A.B);
  const long st = t - (long)pt * A.B;
  const long bq = layout_base(A.Lq, st), bv = layout_base(A.Lv, st), b3 = layout_base(A.L3, st), bj = layout_base(A.Lj, st);
  const T* rp = reinterpret_cast<const T*>(P.r) + 3 * pt;
  const T r[3] = {rp[0], rp[1], rp[2]};
  const int p0 = P.poff[pt], n = P.poff[pt + 1] - p0;
  const long j0 = (long)pt * 3 * M.nv;  // the point's 3 × nv block, column-major
  if (A.jac)
    for (long e = 0; e < 3L * M.nv; ++e) A.jac[(j0 + e) * A.Lj.sk + bj] = T(0);  // (columns off the path; the path's are written below by the same thread)
  T pos[3], vel[3], acc[3];
  point_kin_state<T>(
      M, P.path + p0, n, r, A.v != nullptr && (A.vel || A.acc), A.jac != nullptr,
      [&](int row) { return A.q[(long)row * A.Lq.sk + bq]; }, [&](int row) { return A.v[(long)row * A.Lv.sk + bv]; },
      [&](int row) { return A.vdot ? A.vdot[(long)row * A.Lv.sk + bv] : T(0); },
      [&](int col, int c, T x) { A.jac[(j0 + 3L * col + c) * A.Lj.sk + bj] = x; }, pos, vel, acc);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long o = (long)(3 * pt + k) * A.L3.sk + b3;
    if (A.pos) A.pos[o] = pos[k];
    if (A.vel) A.vel[o] = vel[k];
    if (A.acc) A.acc[o] = acc[k];
  }
}

template <typename T> hipError_t launch_point_kin(const BigModel& M, const PointPlan& P, const PointArgs<T>& A, hipStream_t s) {
  const long total = (long)P.np * A.B;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(point_kin_kernel<T>, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, s, M, P, A);
  return hipGetLastError();
}
template hipError_t launch_point_kin<double>(const BigModel&, const PointPlan&, const PointArgs<double>&, hipStream_t);
template hipError_t launch_point_kin<float>(const BigModel&, const PointPlan&, const PointArgs<float>&, hipStream_t);

}  // namespace rbd
