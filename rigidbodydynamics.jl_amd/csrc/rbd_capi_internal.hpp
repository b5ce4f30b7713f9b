// rbd_capi_internal.hpp — what the two translation units of the C ABI share (rbd_capi.hip, rbd_capi_derivatives.hip): the model and the workspace behind the
// opaque handles of include/rbd_hip.h, the device buffers a workspace owns, and the helpers every entry point starts with.  Host-only.
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <climits>
#include <cmath>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "rbd_hip.h"
#include "rbd_internal.hpp"
#include "rbd_chain_plan.hpp"
#include "rbd_track_plan.hpp"
#include "rbd_walk_plan.hpp"
#include "rbd_reroot.hpp"
#include "rbd_state_plan.hpp"
#include "rbd_jit.hpp"
#include "rbd_mk_fuse.hpp"
#include "rbd_tangent.hpp"
#include "rbd_tangent_mk.hpp"
#include "rbd_adjoint.hpp"
#include "rbd_adjoint_mk.hpp"
#include "rbd_point.hpp"
#include "rbd_point_plan.hpp"

using namespace rbd;

// Everything below is shared by the two files only: hidden, so that tune, ensure, upload, … stay out of the library's dynamic symbol table now that they are no
// longer `static` (its interface is the rbd_* functions of include/rbd_hip.h)
#pragma GCC visibility push(hidden)

extern thread_local std::string g_last_hip_error;  // rbd_last_hip_error (defined in rbd_capi.hip: one per thread for the whole library)

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      g_last_hip_error = std::string(#expr) + ": " + hipGetErrorString(e_);                        \
      return (e_ == hipErrorOutOfMemory) ? RBD_ERR_OUT_OF_MEMORY : RBD_ERR_HIP;                    \
    }                                                                                              \
  } while (0)

// f(T()) with T the scalar type of `dtype`: one argument list for the fp64 and the fp32 instantiation of a launch
template <class F>
auto by_dtype(int dtype, F&& f) { return dtype == RBD_F64 ? f(double()) : f(float()); }

struct rbd_model {
  int32_t nb = 0, nq = 0, nv = 0, nc = 0, nloops = 0;
  int32_t lps = 1, nlevels = 0, maxchild = 0, maxnvj = 0;
  double gravity[3] = {0, 0, 0};
  std::vector<int32_t> ib;      // nb * IB_STRIDE
  std::vector<double> rb;       // nb * RB_STRIDE
  std::vector<int32_t> nslots;  // nlevels
  uint64_t perm_down = 0;
  int32_t inner_floating = 0, has3dof = 0;
  std::vector<int32_t> slot_of, order;  // reference body index <-> DFS pre-order slot
  std::vector<int32_t> dof_body;
  std::vector<int32_t> anc;     // nb * nlevels
  std::vector<uint64_t> row_mask;  // nv x row_words
  int32_t row_words = 1;
  std::vector<rbd_loop_joint_t> loops;
  std::vector<int32_t> loop_i, loop_path, jt_ref, voff_ref, parent_ref, qoff_ref;  // loop tables (reference body indices)
  std::vector<int32_t> mk1, mkf;  // the joints as the integrator stage folded into the compiled dynamics! kernels sees them (rbd_mk_fuse.hpp)
  bool loop_fused_ok = false;
  bool big = false;  // more than 64 bodies: only the any-size kernels of rbd_big_kernels.hip apply (reference-order tables below)
  std::vector<int32_t> big_tbl;
  std::vector<double> big_rb;  // small enough, and only 1-dof / fixed tree joints with parents before children: loop_fused_small_kernel
  std::vector<double> loop_r, axis_ref, axis2_ref;
  // banked lane-per-body mapping (aba_bank_kernel): two bodies per lane, split at level bank_L0; bank_lps == 0: not applicable
  int32_t bank_lps = 0, bank_L0 = 0, bank_nb[2] = {0, 0}, bank_aba_ok = 0;
  std::vector<int32_t> bank_ib[2];
  std::vector<double> bank_rb[2];
  uint64_t bank_perm_down = 0;
  ChainPlan chain;  // the chains of the tree packed on G tracks by list scheduling: what the track / walk plans are built on (rbd_model_chain_plan exposes it)
  TrackPlan track;  // the track schedule of the walk kernels (track.ok == false: mechanism outside their scope)
  // the tree re-rooted at its centre (rbd_reroot.hpp): its own slots, banks and track / walk plans; used by the ABA kernels that support it
  Reroot rr;
  struct RrSlots {
    bool ok = false;
    int32_t nlevels = 0;
    std::vector<int32_t> ib, nslots;
    std::vector<double> rb;
    TrackPlan track;
    WalkPlan walk;
  } rrs;
  // soft contact (src/contact.jl): points in the order of the additional state, half-spaces with unit normals
  int32_t ncp = 0, nhs = 0;
  std::vector<int32_t> cp_body;
  std::vector<double> cp_r, hs_r;  // ncp * CP_STRIDE, nhs * 6
  WalkPlan walk;    // parking slots of aba_walk_kernel on top of the track plan (walk.ok == false: track plan missing or too many steps)
  StatePlan state;  // plan of the one-lane-per-state kernels (state.ok == false: mechanism outside their scope)
  StatePlan state_wide;  // ... of the ones compiled for the mechanism when it has 3-dof joints / 6-dof joints below the world (state.ok == false, state_wide.ok)
  const StatePlan& spec_plan() const { return state.ok ? state : state_wide; }
};

// A program compiled for the mechanism at run time (rbd_jit.hip): `tried` once the answer is final (the module loaded, or no module), its source while the
// compilation is pending (generated once).  The slots of a workspace: the SPEC_* families at spec_slot(family), then the program of a small loop mechanism, the
// banked program and the 12 walk programs (SPEC_WALK + 4 kind + 2 rerooted + pair, as spec_walk)
struct SpecSlot { bool tried = false; hipModule_t mod = nullptr; std::string src; };
enum { SPEC_LOOP = SPEC_SLOTS, SPEC_BANK, SPEC_WALK, SPEC_PROGRAMS = SPEC_WALK + 12 };
// the kernel of run_aba's last launch, as far as simulate_core routes by it: the lane-per-state program compiled for the mechanism (aba_spec_*), its fp64 form
// with the spare rows in the HBM stash (aba_spec_gst_f64), the walk program compiled for the mechanism (aba_walk_spec), any other
enum AbaProgram { ABA_OTHER, ABA_SPEC, ABA_SPEC_STASH, ABA_WALK_SPEC };
// a compiled kernel that is held against the kernels built with the library on its first use by a workspace, and whether it has been (first_use)
struct SpecKernel { hipFunction_t f = nullptr; bool checked = false; };

// Device memory a workspace (or a call) owns: freed with its owner.  `bytes`: what was allocated (what ensure grows by); p == nullptr: empty
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

struct rbd_ws {
  const rbd_model* model = nullptr;
  int32_t device = 0, dtype = RBD_F64, max_batch = 0;
  hipStream_t stream = nullptr;
  DevModel dm{};
  BankModel bm{}; DevBuf d_bank_ib[2], d_bank_rb[2];
  // the re-rooted tree (rbd_reroot.hpp): banked records, chain table, walk plan
  DevBuf d_rr_chain_i, d_rr_chain_r;
  WalkModel wm_rr{}; bool walk_rr = false; DevBuf d_rrtrack_ri, d_rrtrack_rr, d_rrwalk_wk; size_t walk_rr_lds_bytes = 0, walk_rr_lds_bytes_pair = 0;
  TrackModel tm{}; DevBuf d_track_ri, d_track_rr;  // the track plan's records: what the walk kernels read
  ContactModel ctm{}; DevBuf d_cp_body, d_cp_r, d_hs_r;  // soft contact tables
  DevBuf d_tw, d_s0, d_sacc, d_sdot, d_rows;
  WalkModel wm{}; DevBuf d_walk_wk; size_t walk_lds_bytes = 0, walk_lds_bytes_pair = 0; long walk_min_batch = 0, walk_pair_min_batch = 0, sim_walk_min_batch = 1;
  // run-time specialised programs (rbd_jit.hip), loaded on the first use of a route that has them (spec_module), and their kernels; null: not available
  SpecSlot spec_prog[SPEC_PROGRAMS];
  hipFunction_t spec_kin = nullptr, spec_jac = nullptr, spec_mom = nullptr, spec_energy = nullptr, spec_com = nullptr; long spec_kin_min_batch = (long)1 << 62;  // the kinematics by-products compiled for the mechanism (SPEC_KIN, round 6)
  hipFunction_t spec_crba = nullptr, spec_crba_perm = nullptr, spec_emit = nullptr, spec_loop = nullptr, spec_bank_fused = nullptr;
  // (the kernels checked on their first use: first_use)
  SpecKernel spec_chol, spec_chol_nom, spec_chol_packed;  // (each checked with crba_spec_perm before it: M emitted | M_out = NULL | M as the packed triangle)
  SpecKernel spec_aba, spec_aba_nofext, spec_aba_gst, spec_aba_gst_nofext, spec_rnea;
  SpecKernel spec_bank_aba, spec_bank_rnea;  // (the banked programs; spec_bank_aba's check drops spec_bank_fused with it)
  SpecKernel spec_walk[12];  // [dynamics! | inverse dynamics | dynamics!, four `simulate` stages per launch][re-rooted tree][two fp32 states per lane]
  int spec_f64_max_scratch = 0;  // (RBD_TUNE spec_f64_max_scratch; set from the measurement in workspace_create)
  // fp64 dynamics! of those mechanisms: the program with its spare rows in the HBM stash (two wavefronts per CU, a longer chain) against the one with every row in
  // LDS (one per CU): RBD_TUNE spec_f64_stash = 1 always / 0 never / -1 whichever needs fewer chain-times for the batch; the chains' ratio in percent
  int spec_f64_stash = -1, spec_f64_stash_ratio = 170, spec_f64_stash_ratio_fext = 120, spec_ncu = 256;
  // first use of a run-time compiled program by this workspace: its result on the first states of the call against the kernels built with the library
  // (first_use; RBD_TUNE first_use_check=0 for timing experiments with programs that are wrong by construction)
  bool spec_first_use_check = true, spec_first_use_inject = false;
  int spec_aba_scratch = 0, spec_aba_nofext_scratch = 0, spec_rnea_scratch = 0;  // bytes per lane spilled by those kernels: only a kernel without any is picked on its own (it runs 3.4 times slower with: the dispatcher admits fewer wavefronts)
  bool no_reroot = false, loop_no_fused = false; int spec_max_scratch = 512;  // RBD_TUNE: walk_no_reroot, loop_no_fused (tests: the original tree / the three-launch loop route), spec_max_scratch (spilled bytes per lane above which a compiled kernel steps aside)
  bool spec_walk_f32 = true;  // fp32 batches through the compiled walk kernels too (RBD_SPEC_WALK_F32=0: not)
  std::vector<double> loop_gains; bool custom_gains = false;  // rbd_workspace_set_loop_gains: this workspace's Baumgarte gains (4 per loop joint), and whether they differ from the model's
  void* bound_M = nullptr; void* bound_c = nullptr;  // rbd_workspace_bind_result: the caller's own M / c buffers for the CRBA route of rbd_dynamics
  long spec_aba_min_batch = 0, spec_rnea_min_batch = 0, spec_walk_min_batch = 0, walk_one_round_batch = 0, rnea_walk_min_batch = 0;
  StateModel sm{}; DevBuf d_state_ops, d_state_cols, d_state_sr; long state_min_batch = 0; long mass_min_batch = (long)1 << 62, mass_solve_min_batch = (long)1 << 62; long spec_aba_fused_min_batch = (long)1 << 62; long sim_walk_max_batch = 0; bool state_aot = false;  // state_aot: the interpreting one-lane-per-state kernels take the mechanism
  DevBuf d_Msoa; long Msoa_B = -1; int Msoa_perm = -1;  // batch-innermost staging of M for the one-lane-per-state CRBA when the caller's layout is AOS
  long bank_min_batch = 0, rnea_bank_min_batch = 0, bank_resident_states = 0;
  DevBuf d_ib, d_rb, d_dof_body, d_anc, d_row_mask;
  // staging for RBD_MEM_HOST (lazy; HostIO)
  DevBuf stage[8];
  // internal device scratch (mass matrix / bias for the CRBA route), lazy
  DevBuf d_M, d_c, d_K, d_k;
  DevBuf d_body, d_scratch;
  BigModel big{}; DevBuf d_big_tbl, d_big_rb, d_big_scratch, d_big_L;  // rbd_big_kernels.hip (d_big_L: the Cholesky factor, result.L)
  DevBuf d_fused_i;  // loop_fused_small_kernel: parent, q offset, slot by reference body index
  DevBuf d_loop_i, d_loop_r, d_loop_path, d_jt_ref, d_voff_ref, d_axis_ref, d_axis2_ref;
  // Munthe-Kaas integrator scratch (lazy: mk_ensure, for mk_elems states); `mk`: the buffers as the kernels take them
  MkBuffers mk{}; DevBuf d_mk_q0, d_mk_v0, d_mk_phid[4], d_mk_vd[4], d_vdwork; size_t mk_elems = 0;
  DevBuf d_tauwork;  // torques of the device-side PD controller (un-fused integrator path)
  DevBuf d_notpd;  // device flag (an int): some state's mass matrix was not positive definite (checked by rbd_sync)
  int32_t result_layout = RBD_LAYOUT_SOA; int32_t result_B = 0;
  // timing
  int32_t timing = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool ev_pending = false;
  const char* last_kernel = "";  // dominant kernel of the last rbd_dynamics / rbd_simulate / rbd_mass_matrix_solve call
  std::string last_kernel_text;  // where an entry point composes the name (rbd_simulate_contact_controlled: its stage kernels + run_dynamics' route): last_kernel points into it
  int last_aba = ABA_OTHER;  // what the last run_aba launched (AbaProgram): simulate_core routes by it
  // the derivative entry points (rbd_capi_derivatives.hip; kernels: rbd_tangent_kernels.hip): the tree in the reference's order for every mechanism (BigModel
  // tables), the tangent scratch (tan_threads (state, chunk) threads per launch) and the dynamics! buffers — M, its factor, c, v̇, tangent right-hand sides for
  // tan_ntan directions, and for more than 64 coordinates the solve's own vectors — allocated by the first derivative call and when ntan grows
  bool tan_ready = false; BigModel tan{}; DevBuf d_tan_tbl, d_tan_rb, d_tan_scratch; long tan_threads = 0; int tan_ntan = 0;
  DevBuf d_tan_M, d_tan_L, d_tan_c, d_tan_vd, d_tan_rhs, d_tan_x;
  // the simulate derivatives (rbd_simulate_jvp, rbd_simulate_step_derivatives): the stage states' values, and the tangents of one pass of sim_tan_w directions;
  // with contact (rbd_simulate_contact_jvp, rbd_simulate_contact_step_derivatives) the saved initial s and the friction state's four tangents as well
  DevBuf d_sim_val, d_sim_tan; int sim_tan_w = 0;
  // the reverse-mode entry points (rbd_inverse_dynamics_vjp, rbd_dynamics_vjp): the adjoint scratch (adj_states states per launch), the cotangent of v̇
  // staged batch-innermost, λ = M⁻¹ v̇̄ when the caller passes no τ̄, and for more than 64 coordinates the solve's own vector
  bool adj_ready = false; long adj_states = 0;
  DevBuf d_adj_scratch, d_adj_rhs, d_adj_lam, d_adj_x;
  // rbd_simulate_vjp: the joints by class (1-coordinate / the rest, (jtype, qoff, voff) each), the stage states of one step and the cotangents of the
  // backward pass (d_sav), and the step starts kept (d_sav_ckpt)
  bool sav_ready = false; int sav_nn = 0, sav_nw = 0;
  DevBuf d_sav_joints, d_sav, d_sav_ckpt;
  // rbd_workspace_set_points: the points' tables (rbd_point.hpp PointPlan; d_pt_i: poff, path, uni, ubeg, upts in one buffer, d_pt_r: the points); the tables of
  // `tan` are built by then (tan_tbl_ready) without the dynamics! buffers of the derivative entry points
  bool tan_tbl_ready = false; PointPlan pts{}; DevBuf d_pt_i, d_pt_r;
  // rbd_contact_dynamics_vjp / rbd_dynamics_contact_vjp: the model's contact points as a PointPlan of their own (a caller's points stay), the per-point
  // cotangents contact_adjoint_kernel hands to point_adjoint_kernel, the total wrenches' cotangent when the caller takes no fext_bar, and the copy of s the
  // forward contact launch resets
  bool ct_ready = false; PointPlan ct_pts{}; DevBuf d_ct_i, d_ct_r, d_ct_pbar, d_ct_vbar, d_ct_wbar, d_ct_s;
  // rbd_simulate_contact_vjp: the friction state's stage states 1-3, running sum and ṡ of one step, and the cotangents of s0 and of the sum (7 ns values per state)
  bool sct_ready = false; DevBuf d_sct;
  // the loaded programs and the timing events; the buffers free themselves after it
  ~rbd_ws() {
    (void)hipSetDevice(device);
    for (const SpecSlot& p : spec_prog) if (p.mod) (void)hipModuleUnload(p.mod);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

long tune(const char* key, long dflt, bool* has = nullptr);  // RBD_TUNE (rbd_capi.hip)

inline size_t esize(const rbd_ws* w) { return w->dtype == RBD_F64 ? 8 : 4; }

inline Layout layout_of(int layout, long n, long B) {
  Layout L;
  if (layout == RBD_LAYOUT_AOS) { L.sk = 1; L.sb = n; } else { L.sk = B; L.sb = 1; }
  return L;
}

// a buffer with n scalars per state may only be missing when n == 0 (a mechanism whose tree joints are all Fixed has nq = nv = 0)
inline bool missing(const void* p, long n) { return p == nullptr && n > 0; }

struct Opts { int layout, memory, algorithm, stabilization; };

// What every entry point that takes a batch checks first, in this order: the workspace, the model's size, the batch, the layout and the memory kind.  *o: the
// options (the defaults when opts is NULL).  `any_size`: the entry point runs models of more than 64 bodies (on the any-size kernels of rbd_big_kernels.hip);
// the others refuse them
const bool kAnySize = true, kUpTo64Bodies = false;
inline int begin_call(rbd_ws* w, int32_t B, const rbd_opts_t* opts, bool any_size, Opts* o) {
  *o = opts ? Opts{opts->layout, opts->memory, opts->algorithm, opts->stabilization} : Opts{RBD_LAYOUT_SOA, RBD_MEM_DEVICE, RBD_ALGO_ABA, 1};
  if (!w) return RBD_ERR_INVALID_ARGUMENT;
  if (w->model->big && !any_size) return RBD_ERR_UNSUPPORTED;
  if (B < 0 || B > w->max_batch) return RBD_ERR_DIMENSION_MISMATCH;
  if (o->layout != RBD_LAYOUT_SOA && o->layout != RBD_LAYOUT_AOS) return RBD_ERR_INVALID_ARGUMENT;
  if (o->memory != RBD_MEM_DEVICE && o->memory != RBD_MEM_HOST) return RBD_ERR_INVALID_ARGUMENT;
  return RBD_OK;
}

struct Timed {
  rbd_ws* w;
  explicit Timed(rbd_ws* w_) : w(w_) { if (w->timing) (void)hipEventRecord(w->ev0, w->stream); }
  ~Timed() { if (w->timing) { (void)hipEventRecord(w->ev1, w->stream); w->ev_pending = true; } }
};

// at least `need` bytes: grows only — the old buffer freed before the larger one is allocated, the buffer left empty when that fails
int ensure(DevBuf& b, size_t need);
// The dense step of dynamics_solve! for a system of any size, in the workspace's scalar type: L = chol(M) (lower triangle of M read, layout Lm),
// x = M⁻¹(rhs − c) (rhs, c nullable; layout Lv), not positive definite ⇒ w->d_notpd.  Up to 64 coordinates: launch_chol_solve, L_out (nullable) in the layout
// of M.  Beyond (chol_beyond_lanes): launch_big_chol_solve with the factor in `factor` (batch-innermost; the workspace's d_big_L, or the derivative layer's
// d_tan_L), grown here to B states; an L_out that is not that buffer then gets the lower triangle copied, in the layout of M.
int dense_solve(rbd_ws* w, long B, const void* M, const void* rhs, const void* c, void* x, void* L_out, Layout Lm, Layout Lv, DevBuf& factor);
// a table copied to a fresh buffer of its size (16 bytes for an empty one); upload_real: real numbers, in the scalar type of `dtype`
int upload(DevBuf& dst, const void* src, size_t bytes);
int upload_real(DevBuf& dst, const std::vector<double>& src, int dtype);

// The buffers of one call.  RBD_MEM_HOST: each buffer the caller passes is staged in a device buffer of the workspace (w->stage, taken in the order the
// buffers are registered) — in() and inout() copy it there at once, finish() copies every out() and inout() buffer back; asynchronously on the workspace's
// stream (the caller synchronises, rbd_sync).  RBD_MEM_DEVICE: every pointer is the device buffer itself.  A NULL buffer stays NULL.
class HostIO {
 public:
  HostIO(rbd_ws* w, int memory) : w_(w), host_(memory == RBD_MEM_HOST) {}
  int in(const void* src, size_t bytes, const void** dev) {
    void* d;
    const int st = stage(const_cast<void*>(src), bytes, true, false, &d);
    *dev = d;
    return st;
  }
  int out(void* dst, size_t bytes, void** dev) { return stage(dst, bytes, false, true, dev); }
  int inout(void* buf, size_t bytes, void** dev) { return stage(buf, bytes, true, true, dev); }
  int finish() {
    for (int k = 0; k < nout_; ++k) HIP_TRY(hipMemcpyAsync(out_[k].host, out_[k].dev, out_[k].bytes, hipMemcpyDeviceToHost, w_->stream));
    return RBD_OK;
  }

 private:
  enum { kSlots = sizeof(rbd_ws::stage) / sizeof(DevBuf) };
  struct Out { void* host; const void* dev; size_t bytes; };
  int stage(void* buf, size_t bytes, bool copy_in, bool copy_out, void** dev) {
    *dev = buf;
    if (!host_ || !buf) return RBD_OK;
    const int k = nslot_++;
    if (k >= kSlots) return RBD_ERR_INVALID_ARGUMENT;  // (more buffers than slots: a call site that outgrew w->stage)
    if (int st = ensure(w_->stage[k], bytes)) return st;
    *dev = w_->stage[k].p;
    if (copy_in && bytes) HIP_TRY(hipMemcpyAsync(*dev, buf, bytes, hipMemcpyHostToDevice, w_->stream));
    if (copy_out) out_[nout_++] = Out{buf, *dev, bytes};
    return RBD_OK;
  }
  rbd_ws* w_;
  bool host_;
  int nslot_ = 0, nout_ = 0;
  Out out_[kSlots];
};

// what the derivative entry points call of rbd_capi.hip: the scratch of the any-size kernels, and contact_dynamics! on device pointers
// (the last two stand among the extern "C" entry points there, hence their linkage)
int big_scratch(rbd_ws* w, int32_t B);
extern "C" int run_contact_kinematics(rbd_ws* w, int32_t B, const Opts& o, const void* dq, const void* dv);
extern "C" int run_contact(rbd_ws* w, int32_t B, const Opts& o, const void* dq, const void* dv, void* ds, void* dsd, const void* df, void* dcw, void* dtw);

#pragma GCC visibility pop
