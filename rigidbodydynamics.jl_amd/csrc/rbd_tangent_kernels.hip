// rbd_tangent_kernels.hip — the kernels of the derivative entry points (rbd_inverse_dynamics_jvp, rbd_dynamics_jvp, rbd_inverse_dynamics_derivatives,
// rbd_dynamics_derivatives): the tangent RNEA (rbd_tangent.hpp) with one thread per (state, chunk of TAN_CHUNK directions), and the multi-right-hand-side
// triangular solve of dynamics! tangents against the Cholesky factor of M.  Compiled with -ffinite-math-only -fno-signed-zeros (build.sh): the zero
// tangents of the mechanism's constants fold out of the products.
#include "rbd_tangent.hpp"
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
  const long nchunks = (A.ntan + N - 1) / N, total = nchunks * A.B;
  for (long t0 = 0; t0 < total; t0 += max_threads) {  // slabs of the scratch's size
    const long nt = total - t0 < max_threads ? total - t0 : max_threads;
    hipLaunchKernelGGL((tangent_rnea_kernel<T, N>), dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, s, M, A, t0, nt, (T*)scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
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

#define RBD_TAN_INST(T)                                                                                                                                    \
  template hipError_t launch_tangent_rnea<T>(const BigModel&, const TanArgs<T>&, void*, long, hipStream_t);                                              \
  template hipError_t launch_tangent_solve<T>(int, long, int, int, const void*, Layout, const void*, int, const ColOut<T>&, void*, hipStream_t);          \
  template hipError_t launch_symmetrize<T>(int, long, void*, Layout, hipStream_t);
RBD_TAN_INST(double)
RBD_TAN_INST(float)

}  // namespace rbd
