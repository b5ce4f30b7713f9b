/*
 * rbd_hip.h — C ABI of librbd_hip.so, the MI355X (gfx950) batched rigid-body
 * dynamics engine that replaces the data-parallel hot path of
 * RigidBodyDynamics.jl (reference paths are relative to the upstream repo):
 *
 *   rbd_dynamics          <->  dynamics!(result, state, τ, wext)       src/mechanism_algorithms.jl:845-864
 *   rbd_inverse_dynamics  <->  inverse_dynamics!(τ, jw, acc, state, v̇, wext)  src/mechanism_algorithms.jl:542-553
 *   rbd_dynamics_bias     <->  dynamics_bias!(result, state)           src/mechanism_algorithms.jl:484-498
 *   rbd_mass_matrix       <->  mass_matrix!(M::Symmetric, state)       src/mechanism_algorithms.jl:248-272
 *   rbd_mass_matrix_solve <->  dynamics_solve!(result, τ) (no-loop branch) src/mechanism_algorithms.jl:747-822
 *   rbd_model_create      <->  MechanismState(mechanism) index tables  src/mechanism_state.jl:79-172
 *   rbd_simulate          <->  simulate(state0, T; Δt) / MuntheKaasIntegrator.step  src/simulate.jl:36-55, src/ode_integrators.jl:233-299
 *
 * The reference is pure Julia and has no FFI layer; this header is what a
 * Julia `ccall` shim (julia/RigidBodyDynamicsGPU.jl) binds.
 *
 * Conventions
 *  - every entry point returns an int status (RBD_OK == 0); nothing throws or
 *    longjmps across the boundary; caller buffers are never owned by the library;
 *  - a *state* is one (q, v) of the mechanism; a *batch* is B independent states
 *    of the same mechanism (one evaluation per state);
 *  - batch buffers are DEVICE pointers of the workspace's dtype unless
 *    opts->memory == RBD_MEM_HOST (then the library stages through its own
 *    device buffers; PCIe time is then inside the call);
 *  - layout RBD_LAYOUT_SOA: element k of state b lives at x[k*B + b]
 *    (coordinate-major, coalesced);  RBD_LAYOUT_AOS: x[b*n + k] — the Julia
 *    `n × B` column-major matrix with one state per column;
 *  - motion vectors are (angular; linear), force vectors (torque; force), as in
 *    src/spatial/spatialmotion.jl:122-153 and src/spatial/spatialforce.jl:73-111;
 *  - calls are asynchronous on the workspace's HIP stream; rbd_sync() waits.
 *    (Since 600 one exception per program and workspace: the FIRST result of a
 *    kernel compiled for the mechanism at run time — dynamics!, inverse_dynamics!,
 *    fp32 mass_matrix! + solve — is compared with the interpreting kernel on the
 *    call's first states: a small allocation and one synchronisation in that call,
 *    never inside a stream capture; a program that differs is dropped, the call
 *    recomputed, rbd_last_hip_error says so.)
 *    A model handle is immutable and shareable; a workspace must not be used
 *    from two host threads at once (same rule as MechanismState/DynamicsResult,
 *    which are mutable caches: src/mechanism_state.jl:35-78).
 */
#ifndef RBD_HIP_H
#define RBD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------- */
enum {
  RBD_OK = 0,
  RBD_ERR_INVALID_ARGUMENT = 1,   /* Julia side: ArgumentError           */
  RBD_ERR_DIMENSION_MISMATCH = 2, /* Julia side: DimensionMismatch       */
  RBD_ERR_UNSUPPORTED = 3,        /* joint type / feature not built      */
  RBD_ERR_NO_DEVICE = 4,          /* no HIP device: the product has NO CPU fallback */
  RBD_ERR_HIP = 5,                /* a HIP runtime call failed (see rbd_last_hip_error) */
  RBD_ERR_OUT_OF_MEMORY = 6,
  RBD_ERR_HAS_LOOPS = 7,          /* inverse_dynamics! on a mechanism with loop joints
                                     (src/mechanism_algorithms.jl:549)   */
  RBD_ERR_NOT_POSITIVE_DEFINITE = 8
};

/* ---- joint types (src/joint_types/ *.jl) ---------------------------------- */
enum {
  RBD_JOINT_FIXED = 0,          /* fixed.jl            nq=0 nv=0 */
  RBD_JOINT_REVOLUTE = 1,       /* revolute.jl         nq=1 nv=1 */
  RBD_JOINT_PRISMATIC = 2,      /* prismatic.jl        nq=1 nv=1 */
  RBD_JOINT_QUAT_FLOATING = 3,  /* quaternion_floating.jl nq=7 (w,x,y,z,px,py,pz) nv=6 (ω; v) body frame */
  RBD_JOINT_PLANAR = 4,         /* planar.jl           nq=3 nv=3 */
  RBD_JOINT_QUAT_SPHERICAL = 5, /* quaternion_spherical.jl nq=4 nv=3 */
  RBD_JOINT_SINCOS_REVOLUTE = 6 /* sin_cos_revolute.jl nq=2 nv=1 */
};

enum { RBD_F64 = 0, RBD_F32 = 1 };
enum { RBD_LAYOUT_SOA = 0, RBD_LAYOUT_AOS = 1 };
enum { RBD_MEM_DEVICE = 0, RBD_MEM_HOST = 1 };
/* forward-dynamics algorithm behind rbd_dynamics */
enum {
  RBD_ALGO_ABA = 0,          /* fused articulated-body algorithm (default; tree mechanisms)   */
  RBD_ALGO_CRBA_CHOLESKY = 1,/* the reference's own route: bias-RNEA + CRBA + Cholesky; also
                                fills M and c in the workspace; the only route with loop joints */
  /* RBD_ALGO_ABA picks between three lane mappings of the same algorithm by how many wavefronts the batch makes of each
     (rbd_capi.hip run_aba); these force one (tests, benchmarks): */
  RBD_ALGO_ABA_LANES = 2,    /* one lane per (state, body), level-synchronous sweeps: small batches, every tree joint type          */
  RBD_ALGO_ABA_CHAINS = 3,   /* (round 1: chains of the tree on a few lanes per state.  Removed in round 3 — it lost at every batch
                                size; the value stays reserved and returns RBD_ERR_UNSUPPORTED)                                     */
  RBD_ALGO_ABA_BANKS = 4,    /* lane-per-body with two bodies per lane (levels split into two banks): twice the states per
                                wavefront; 1-dof / fixed tree joints, 6-dof joints on the world.  The bench workload (4096 Atlas states) */
  RBD_ALGO_ABA_TRACKS = 5,   /* (round 2: chains of the tree on a few lanes per state, per-body results in lane-private LDS rows.  Removed in
                                round 4 like RBD_ALGO_ABA_PIPE — both lost at every batch size; reserved, RBD_ERR_UNSUPPORTED)          */
  RBD_ALGO_ABA_WALK = 6,     /* the track schedule with one WAVEFRONT per track and one lane per state: a workgroup is up to four
                                wavefronts over the same 64 states, q / v / tau staged through LDS, per-joint results in accumulation
                                registers.  Trees of revolute / prismatic / fixed joints, 6-dof joints on the world, at most 11 steps per
                                track; RBD_ERR_UNSUPPORTED elsewhere or when the rows of 64 states do not fit one compute unit's LDS.
                                Large batches.  `simulate` on this mapping takes the four stages of a step in ONE launch (a looped instantiation of its own:
                                admitted statically — rbd_jit_check_walk_object — since 600)                                        */
  RBD_ALGO_ABA_PIPE = 7,     /* (round 2: a body-step cut into stages on the four SIMDs of a compute unit.  Removed; reserved)     */
  RBD_ALGO_ABA_COMPILED = 8  /* one lane per state, straight-line code compiled for the mechanism at run time (rbd_jit_* below): fp32,
                                trees of every joint type above (since 400: Planar, QuaternionSpherical, QuaternionFloating below the world
                                too), no loop joints, nv <= 64; RBD_ALGO_ABA picks it from half a chip-full of wavefronts up.  Since 600 also
                                fp64 for the mechanisms no walk kernel takes (3-dof joints, 6-dof joints below the world — the reference's
                                randmech(): 65 536 states 177 us against 684 one body per lane; two programs — every row in LDS, or the spare
                                rows in an HBM stash of the workspace and two wavefronts per CU — picked by batch); RBD_ALGO_ABA picks it from
                                8193 states.
                                RBD_ERR_UNSUPPORTED without hiprtc, outside that scope, or when the program's first result in this workspace
                                differs from the interpreting kernel's on the same states (first-use check, since 600: the program is
                                dropped, rbd_last_hip_error says so; RBD_ALGO_ABA recomputes the call on the interpreting kernels)    */
};

/* ---- loop (non-tree) joint: src/mechanism_modification.jl:38-43,
 *      constraint rows src/mechanism_algorithms.jl:574-673 ------------------ */
typedef struct rbd_loop_joint {
  int32_t predecessor;      /* moving-body index, -1 = world                          */
  int32_t successor;        /* moving-body index, -1 = world                          */
  int32_t joint_type;       /* RBD_JOINT_*                                            */
  int32_t _pad;
  double axis[3];           /* Revolute/Prismatic axis in frame_before                */
  double pred_rot[9];       /* joint_to_predecessor: frame_before -> predecessor body frame, row-major R */
  double pred_trans[3];
  double succ_rot[9];       /* joint_to_successor:  frame_after  -> successor body frame, row-major R   */
  double succ_trans[3];
  double rotation_from_z_aligned[9]; /* Revolute / Prismatic: rotation_from_z_aligned, src/joint_types/revolute.jl:12-17;
                                        Planar: the matrix with columns (x_axis, y_axis, x_axis × y_axis), planar.jl:22-35 */
  double gains[4];          /* Baumgarte SE3PDGains: angular k, d; linear k, d (default 100,20,100,20:
                               src/mechanism_algorithms.jl:610-612); all zero = stabilization off */
} rbd_loop_joint_t;

/* ---- soft contact (src/contact.jl): contact points on bodies against half-spaces of the environment --------------------------
 * DefaultContactPoint = ContactPoint{SoftContactModel{HuntCrossleyModel, ViscoelasticCoulombModel}} (src/contact.jl:196) and
 * HalfSpace3D (:202-222).  Every (contact point, half-space) pair owns 3 additional states (the tangential displacement of the
 * friction model; the normal model has none): s has 3 * n_contact_points * n_halfspaces entries per state of the batch, ordered
 * point-major as MechanismState lays them out (src/mechanism_state.jl:139-152: for body, for point, for half-space) — i.e. in the
 * order the points are listed here.                                                                                              */
typedef struct rbd_contact_point {
  int32_t body;            /* moving-body index                                                        */
  int32_t _pad;
  double location[3];      /* Point3D in the body's default frame (= frame_after of its joint)         */
  double hc_k, hc_lambda, hc_n;   /* HuntCrossleyModel k, λ, n   (hunt_crossley_hertz: λ = 3/2 α k, n = 3/2)   */
  double mu, k, b;         /* ViscoelasticCoulombModel μ, k, b                                         */
} rbd_contact_point_t;
typedef struct rbd_halfspace {
  double point[3];          /* root frame */
  double outward_normal[3]; /* root frame; normalized on model creation like HalfSpace3D's constructor */
} rbd_halfspace_t;

/* ---- the flattened mechanism ---------------------------------------------
 * Exactly the tables MechanismState builds once (src/mechanism_state.jl:85-118):
 * moving body i (0-based) is the successor of tree joint i; bodies are in the
 * reference's tree-joint order (topological: parents first). After
 * canonicalize_frame_definitions! (src/mechanism.jl:250-260) the body frame IS
 * frame_after(joint i) and joint_to_successor of tree joints is identity.      */
typedef struct rbd_flat_model {
  int32_t n_bodies;            /* number of moving bodies == tree joints               */
  int32_t nq, nv;              /* num_positions, num_velocities                        */
  int32_t n_loops;             /* non-tree joints                                      */
  const int32_t* parent;       /* [n_bodies] predecessor body of joint i, -1 = world   */
  const int32_t* joint_type;   /* [n_bodies] RBD_JOINT_*                               */
  const int32_t* q_offset;     /* [n_bodies] first q index (qranges)                   */
  const int32_t* v_offset;     /* [n_bodies] first v index (vranges)                   */
  const double* joint_axis;    /* [n_bodies*3] axis in frame_before (Revolute/Prismatic); Planar: x_axis */
  const double* joint_axis2;   /* [n_bodies*3] Planar y_axis (else ignored; may be NULL) */
  const double* pred_rot;      /* [n_bodies*9] joint_to_predecessor R, row-major (src/joint.jl:49) */
  const double* pred_trans;    /* [n_bodies*3]                                         */
  const double* inertia_moment;/* [n_bodies*9] J about the body-frame origin, row-major (src/spatial/motion_force_interaction.jl:28-37) */
  const double* inertia_cross; /* [n_bodies*3] cross_part = mass * com                 */
  const double* inertia_mass;  /* [n_bodies]                                           */
  double gravity[3];           /* gravitational_acceleration in the root frame (default 0,0,-9.81: src/mechanism.jl:1) */
  const rbd_loop_joint_t* loops; /* [n_loops] or NULL                                  */
  int32_t n_contact_points;    /* contact_points of all bodies (0: none, like every URDF-parsed mechanism) */
  int32_t n_halfspaces;        /* mechanism.environment.halfspaces                     */
  const rbd_contact_point_t* contact_points; /* [n_contact_points] or NULL, in the order of the additional state */
  const rbd_halfspace_t* halfspaces;         /* [n_halfspaces] or NULL                 */
} rbd_flat_model_t;

typedef struct rbd_model rbd_model_t; /* opaque, immutable after create               */
typedef struct rbd_ws rbd_ws_t;       /* opaque, one per host thread / HIP stream     */

typedef struct rbd_opts {
  int32_t layout;     /* RBD_LAYOUT_*  (default SOA)                                  */
  int32_t memory;     /* RBD_MEM_*     (default DEVICE)                               */
  int32_t algorithm;  /* RBD_ALGO_*    (rbd_dynamics only)                            */
  int32_t stabilization; /* 1 = Baumgarte stabilization with the workspace's gains (the model's — the
                            reference's default — unless rbd_workspace_set_loop_gains replaced them),
                            0 = `stabilization_gains=nothing`                         */
} rbd_opts_t;

/* ---- model / workspace lifetime ------------------------------------------ */
/* Sizes: mechanisms of up to 64 moving bodies with at most 8 children per body run on the wavefront-shaped kernels (any nv).  Mechanisms of MORE than 64 bodies, or
 * with a body of more than 8 children (since header 600; refused before), are accepted too and run on one-thread-per-state kernels with an HBM scratch (no speed
 * claim) — rbd_dynamics with its loop branch, rbd_inverse_dynamics[_bodies], rbd_dynamics_bias[_bodies], rbd_mass_matrix[_solve], rbd_mass_matrix_solve_packed,
 * rbd_dynamics_result, rbd_contact_dynamics, rbd_dynamics_contact, rbd_simulate / rbd_simulate_controlled (the PD law included) / rbd_mk_stage (since 500), since 600
 * the kinematics by-products rbd_kinematics, rbd_geometric_jacobian, rbd_momentum, since 700 the derivative entry points, and rbd_cholesky_solve (which
 * uses nv alone).  rbd_simulate_contact returns RBD_ERR_UNSUPPORTED for such a model.  The reference has no size limit (src/mechanism_algorithms.jl:28-50, :80-99, :313-327). */
int rbd_model_create(const rbd_flat_model_t* desc, rbd_model_t** out); /* deep-copies desc */
int rbd_model_destroy(rbd_model_t* model);
/* Introspection of the chain schedule under the track / walk plans: tracks per state, steps per pass, (lds_fields: 0, kept for ABI
 * stability), and the steps×tracks table of reference body indices (-1 = idle).  RBD_ERR_UNSUPPORTED when the mechanism is
 * outside the scope of those mappings.  Host-only, no device needed. */
/* ... and of the two-bodies-per-lane ("banked") mapping: lanes per state, the level at which bank 1 starts, bodies per bank, and whether
 * the banked ABA (not only the banked RNEA) takes the mechanism.  RBD_ERR_UNSUPPORTED when the split would not save lanes. */
int rbd_model_bank_plan(const rbd_model_t* model, int32_t* lanes, int32_t* first_level_of_bank1, int32_t* bodies_bank0, int32_t* bodies_bank1,
                        int32_t* aba_in_scope);
/* ... and of the track plan under the walk kernels (RBD_ALGO_ABA_WALK): dims[6] = tracks per state, steps, A/C mailboxes, B mailboxes, has a 6-dof root,
 * has prismatic/fixed joints; table: steps×tracks reference body indices (-1 = idle); ri / rr: the packed per-(step, track) records
 * the kernel reads (rbd_device.hpp TI_*, TR_*) — what tests/emu feeds to the CPU emulation of the kernel's step code.        */
int rbd_model_track_plan(const rbd_model_t* model, int32_t* dims, int32_t* table, int32_t table_cap, int32_t* ri, int32_t ri_cap, double* rr, int32_t rr_cap);
/* ... and of the plan the walk kernels run when the mechanism hangs on the world by one 6-dof joint and is shallower seen from another
 * body: the tree RE-ROOTED at its centre (csrc/rbd_reroot.hpp; the floating joint's coordinates stay where they are).
 * dims[12] = tracks, steps, A/C mailboxes, B mailboxes, 6-dof root, prismatic/fixed joints, parking slots, chain length, q / v offset of the
 * floating joint, new root body, old floating body;  ri: packed records followed by the per-step flags;  rr: constants;  wk: parking words
 * (BFD_* flags in bits 8..9);  chain_i[4·chain], chain_r[15·chain], fxp[12]: the joints between the old floating body and the new root.
 * RBD_ERR_UNSUPPORTED when the mechanism is not re-rooted.  Host-only. */
int rbd_model_reroot_plan(const rbd_model_t* model, int32_t* dims, int32_t* ri, int32_t ri_cap, double* rr, int32_t rr_cap, int32_t* wk, int32_t wk_cap,
                          int32_t* chain_i, double* chain_r, double* fxp);
int rbd_model_chain_plan(const rbd_model_t* model, int32_t* tracks, int32_t* steps, int32_t* lds_fields, int32_t* table, int32_t capacity);
int rbd_model_dims(const rbd_model_t* model, int32_t* n_bodies, int32_t* nq, int32_t* nv, int32_t* nc);

/* stream: a hipStream_t passed as void* (NULL = the device's default stream) */
int rbd_workspace_create(const rbd_model_t* model, int32_t max_batch, int32_t device,
                         int32_t dtype, void* stream, rbd_ws_t** out);
int rbd_workspace_destroy(rbd_ws_t* ws);
int rbd_workspace_set_stream(rbd_ws_t* ws, void* stream);
/* `stabilization_gains` as an AbstractDict{JointID, SE3PDGains} / ConstDict (src/mechanism_algorithms.jl:614-632, :848; src/simulate.jl:37): the Baumgarte
 * gains of the calls that FOLLOW on this workspace (rbd_dynamics, rbd_simulate*, rbd_mk_stage with opts->stabilization = 1).  gains: HOST array of
 * 4 × n_loops doubles — (angular k, angular d, linear k, linear d) for every loop joint in the order of rbd_flat_model_t.loops; NULL restores the
 * model's (rbd_loop_joint_t.gains).  Cheap when the gains are the ones already in force (no device access), so a binding may call it before every
 * dynamics!; otherwise it waits for the workspace's stream.  Non-finite gains: RBD_ERR_INVALID_ARGUMENT.  No-op for tree mechanisms. */
int rbd_workspace_set_loop_gains(rbd_ws_t* ws, const double* gains);
int rbd_sync(rbd_ws_t* ws);

/* ---- the hot path ----------------------------------------------------------
 * q[nq×B], v[nv×B], tau[nv×B] (NULL => zeros, like the ConstVector default),
 * fext[6*n_bodies×B] external wrench on each moving body in the ROOT frame,
 * (torque; force) (NULL => none, like NullDict); outputs vdot[nv×B],
 * qdot[nq×B] (nullable), lambda[nc×B] (nullable).                              */
/* Mechanisms WITH contact points and an environment: rbd_dynamics / rbd_simulate / rbd_simulate_controlled return RBD_ERR_UNSUPPORTED — the reference's
 * dynamics! always adds the contact wrenches (src/mechanism_algorithms.jl:849-856), which needs the additional state: use
 * rbd_dynamics_contact / rbd_simulate_contact / rbd_simulate_contact_controlled.  rbd_mk_stage takes them: its stage covers (q, v) only, and a caller with a
 * host-side controller carries the additional state through the same tableau beside it (rbd_dynamics_contact at every stage state). */
int rbd_dynamics(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* tau,
                 const void* fext, void* vdot, void* qdot, void* lambda, const rbd_opts_t* opts);

/* tau_out = M(q) vdot + c(q, v, fext); tree mechanisms only */
int rbd_inverse_dynamics(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* vdot,
                         const void* fext, void* tau_out, const rbd_opts_t* opts);

/* c_out = c(q, v, fext) = inverse dynamics with vdot = 0 */
int rbd_dynamics_bias(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* fext,
                      void* c_out, const rbd_opts_t* opts);

/* The same two entry points with the per-body outputs the reference fills beside the torques (every output nullable):
 *   jointwrenches_out[6*n_bodies×B]  jointwrenchesout of inverse_dynamics! / result.jointwrenches of dynamics_bias! — the wrench across
 *                                    the joint above each body after joint_wrenches_and_torques! (src/mechanism_algorithms.jl:442-459);
 *   accelerations_out[6*n_bodies×B]  accelerations of inverse_dynamics! (spatial_accelerations!, :387-417: root acceleration −g included)
 *                                    / result.accelerations of dynamics_bias! (bias_accelerations!, :377-385);
 * both in the ROOT frame, (angular; linear) / (torque; force), bodies in the flat model's order, layout as fext.  With them
 * DynamicsResult's accelerations / jointwrenches / totalwrenches (src/dynamics_result.jl:26-29) are complete: totalwrenches of a
 * mechanism without contact points is the caller's own fext (mechanism_algorithms.jl:851-855).
 * Large batches: the batch-innermost layout (RBD_LAYOUT_SOA) is the cheap one for these outputs — Atlas, 65 536 states, both outputs: fp32 51 us
 * (state-major 100 us: the kernel stores batch-innermost scratch and a second kernel moves it), fp64 78 us (state-major 118 us).      */
int rbd_inverse_dynamics_bodies(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* vdot, const void* fext, void* tau_out,
                                void* jointwrenches_out, void* accelerations_out, const rbd_opts_t* opts);
int rbd_dynamics_bias_bodies(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* fext, void* c_out, void* jointwrenches_out,
                             void* accelerations_out, const rbd_opts_t* opts);

/* M_out: nv×nv column-major per state (element (i,j) of state b at
 * M[(j*nv+i)*B + b] for SOA, M[b*nv*nv + j*nv + i] for AOS). Like the
 * reference (Symmetric, uplo 'L') the LOWER triangle i>=j is the result; the strict upper triangle is not to
 * be read (the reference leaves it undefined; most paths do not touch it, the fp32 path of
 * rbd_mass_matrix_solve on the kernels compiled for the mechanism — column-per-state callers, from 256 states since 600 (32 768 before: it is ahead at
 * every batch) — writes the mirror image there because whole cache lines leave the chip faster). */
int rbd_mass_matrix(rbd_ws_t* ws, int32_t B, const void* q, void* M_out, const rbd_opts_t* opts);

/* x = M(q)^-1 rhs; rhs, x: nv×B.  opts->algorithm == RBD_ALGO_CRBA_CHOLESKY: CRBA + batched lower Cholesky, the potrf/potrs
 * of dynamics_solve!;  RBD_ALGO_ABA (default): the O(n) articulated-body solve (forward dynamics with v = 0, g = 0,
 * tau = rhs), which never forms M.  M_out nullable (same layout as rbd_mass_matrix); tree mechanisms.              */
int rbd_mass_matrix_solve(rbd_ws_t* ws, int32_t B, const void* q, const void* rhs, void* x,
                          void* M_out, const rbd_opts_t* opts);
/* ... (CRBA + Cholesky) with M as LAPACK's PACKED lower triangle: element (i, j), i >= j, of state b at index i + j (2 nv − j − 1) / 2 of its
 * np = nv (nv + 1) / 2 values — M_packed_out: np × B in opts->layout (AOS: the np values of a state contiguous).  This is the part of M the reference defines
 * (`Symmetric(…, :L)`: src/dynamics_result.jl:42, mass_matrix! :248-272) and half the bytes of the square, which is what the emission of M costs at large
 * batches (Atlas, 65 536 fp32 states: 175 MB instead of 357 MB).  SURVEY.md §8(b) "lower triangle valid; or packed".                                    */
int rbd_mass_matrix_solve_packed(rbd_ws_t* ws, int32_t B, const void* q, const void* rhs, void* x, void* M_packed_out, const rbd_opts_t* opts);

/* The dense step of dynamics_solve! on its own: L = potrf!('L', M) and x = potrs!(L, rhs) for B caller-provided nv×nv SPD
 * matrices (lower triangles read, the strict upper ones never; device pointers).  L_out (nullable) receives the lower
 * triangle of the factor in the layout of M — DynamicsResult.L (src/dynamics_result.jl:32); its strict upper triangle
 * is left untouched.  Only nv of the model is used: every model and every nv is taken.  The kernel by nv: <= 40 the MFMA
 * tile kernels (chol_mfma_kernel fp32, chol_mfma64_kernel fp64), 41..48 chol_reg_kernel, 49..64 chol_solve_kernel (LDS),
 * beyond 64 big_chol_solve_kernel (one thread per state).  A matrix that is not positive definite: rbd_sync returns
 * status 8 once; the other states of the batch are not disturbed.                                                     */
int rbd_cholesky_solve(rbd_ws_t* ws, int32_t B, const void* M, const void* rhs, void* x, void* L_out, const rbd_opts_t* opts);

/* after rbd_dynamics(..., RBD_ALGO_CRBA_CHOLESKY): copy the DynamicsResult side
 * products out of the workspace (any pointer may be NULL). M: nv×nv (lower),
 * c: nv, K: nc×nv column-major, k: nc; layout per opts.                        */
int rbd_dynamics_result(rbd_ws_t* ws, int32_t B, void* M, void* c, void* K, void* k,
                        const rbd_opts_t* opts);
/* rbd_dynamics on the CRBA route leaves M and c in the workspace for rbd_dynamics_result to copy out.  A caller that wants them in its own buffers anyway
 * (the reference's dynamics!(result, ...) fills result.massmatrix / result.dynamicsbias in place) binds those buffers first: tree mechanisms then have M and c
 * written there directly — at 65 536 fp32 Atlas states the copy of M alone was a third of the call — and rbd_dynamics_result skips the bound fields.
 * Device pointers in the layout of the rbd_dynamics calls that follow; NULL unbinds.  Mechanisms with loop joints keep the workspace copies. */
int rbd_workspace_bind_result(rbd_ws_t* ws, void* M, void* c);

/* ---- the caller of the hot path: batched `simulate` --------------------------------------------
 * simulate(state0, final_time; Δt) src/simulate.jl:36-55 == MuntheKaasIntegrator.step (src/ode_integrators.jl:233-299) with
 * the runge_kutta_4 tableau (:48-55), for every state of the batch in lockstep, entirely on the device (no host round trip
 * per stage).  rbd_simulate: nsteps steps with constant tau / fext (the reference's default control is zero_torque!); q, v
 * are advanced in place.  rbd_mk_stage: one stage at a time for callers that evaluate a controller per stage —
 * stage 0 snapshots (q, v) as the base point and leaves the stage-1 state in (q, v); stage s = 1..3 takes the v̇ of the
 * previous stage state and leaves the next stage state in (q, v); stage 4 takes the last v̇ and leaves the end-of-step
 * state.  Loop mechanisms use the loop branch with opts->stabilization.                                              */
int rbd_simulate(rbd_ws_t* ws, int32_t B, void* q, void* v, const void* tau, const void* fext, double dt, int32_t nsteps,
                 const rbd_opts_t* opts);
int rbd_mk_stage(rbd_ws_t* ws, int32_t B, int32_t stage, double dt, void* q, void* v, const void* vdot_prev, const rbd_opts_t* opts);

/* ---- `simulate(state, T, control!)` without a host round trip per stage (src/simulate.jl:36-48: the reference calls control!(τ, t, state)
 *      before every stage's dynamics!).  Two device-side controller forms cover the common cases; anything else keeps the
 *      rbd_mk_stage + rbd_dynamics loop with the controller on the host.
 *   RBD_CONTROL_CONSTANT : τ = tau (nv × B, NULL = 0) — what rbd_simulate does.
 *   RBD_CONTROL_TABLE    : an open-loop τ(t): `tau` holds entries of nv × B each (batch layout of opts), entry 4·step + stage when
 *                          per_stage = 1 — the stage times t, t + h/2, t + h/2, t + h control! is called with — or entry `step` when
 *                          per_stage = 0 (zero-order hold over the step).
 *   RBD_CONTROL_PD       : τ_i = tau_i − kp_i (q_i − q_des_i) − kd_i v_i on every Revolute / Prismatic joint, evaluated on the STAGE state inside
 *                          the dynamics launch (other joint types: τ = tau).  kp, kd: [nv] gains, q_des: nq × B (NULL = 0), all DEVICE arrays of
 *                          the workspace's scalar type.
 * Device memory only (opts->memory = RBD_MEM_DEVICE); tree mechanisms without contact points (with them: rbd_simulate_contact_controlled). */
enum { RBD_CONTROL_CONSTANT = 0, RBD_CONTROL_TABLE = 1, RBD_CONTROL_PD = 2 };
typedef struct rbd_control {
  int32_t kind;       /* RBD_CONTROL_*                                   */
  int32_t per_stage;  /* TABLE: 1 = four entries per step, 0 = one       */
  const void* tau;    /* see above                                       */
  const void* q_des;  /* PD                                              */
  const void* kp;     /* PD                                              */
  const void* kd;     /* PD                                              */
} rbd_control_t;
int rbd_simulate_controlled(rbd_ws_t* ws, int32_t B, void* q, void* v, const rbd_control_t* control, const void* fext, double dt, int32_t nsteps,
                            const rbd_opts_t* opts);

/* ---- soft contact: contact_dynamics! (src/mechanism_algorithms.jl:680-723) and the entry points that include it --------------------
 * rbd_contact_dynamics: for every contact point inside a half-space the force of contact_dynamics! (src/contact.jl:79-93: Hunt–Crossley
 *   normal force, viscoelastic Coulomb friction) as a wrench on its body in the ROOT frame, and the state derivative of the friction
 *   model; for a pair that is not in contact the reference resets the state and zeroes the derivative — so `s` is IN/OUT.
 *   s, sdot: ns×B with ns = 3·n_contact_points·n_halfspaces; contactwrenches[6·n_bodies×B] = result.contactwrenches (nullable).
 * rbd_dynamics_contact: dynamics!(result, state, τ, wext) of a mechanism with contact points (:845-864): contact_dynamics!, then
 *   totalwrenches = wext + contactwrenches (:851-856), then forward dynamics with those.  totalwrenches nullable.
 * rbd_simulate_contact: simulate (src/simulate.jl:36-55) with the additional state integrated beside (q, v) by the same Runge–Kutta
 *   tableau (src/ode_integrators.jl:233-299).  Tree mechanisms.  It is rbd_simulate_contact_controlled with RBD_CONTROL_CONSTANT (below): one
 *   stage driver, the same scope and status codes, and rbd_workspace_last_kernel answers "contact_head_kernel + contact_sim_kernel + <the
 *   forward-dynamics route>" afterwards.  (Until the two were folded it ran a stage of its own — a kernel for s, a whole RNEA launch for the
 *   per-body kinematics, contact_kernel: fp64 results are those of that stage bit for bit on the recorded cases, fp32 results to rounding.)
 * rbd_contact_dynamics and rbd_dynamics_contact take their per-body kinematics from the same contact_head_kernel (trees of at most 64 bodies). */
int rbd_model_contact_dims(const rbd_model_t* model, int32_t* n_contact_points, int32_t* n_halfspaces, int32_t* n_additional_states);
int rbd_contact_dynamics(rbd_ws_t* ws, int32_t B, const void* q, const void* v, void* s, void* contactwrenches, void* sdot, const rbd_opts_t* opts);
int rbd_dynamics_contact(rbd_ws_t* ws, int32_t B, const void* q, const void* v, void* s, const void* tau, const void* fext, void* vdot, void* qdot,
                         void* sdot, void* contactwrenches, void* totalwrenches, const rbd_opts_t* opts);
int rbd_simulate_contact(rbd_ws_t* ws, int32_t B, void* q, void* v, void* s, const void* tau, const void* fext, double dt, int32_t nsteps,
                         const rbd_opts_t* opts);

/* rbd_simulate_contact_controlled (700 addition): `simulate(state, T, control!)` of a mechanism with contact points — the Munthe-Kaas RK4 step, the friction
 * state s through the same tableau and reset by contact_dynamics! at each stage state, with rbd_simulate_controlled's device-side controllers:
 *   RBD_CONTROL_CONSTANT : τ = tau (NULL = 0) — this is rbd_simulate_contact, bit for bit.
 *   RBD_CONTROL_TABLE    : entry 4·step + stage (per_stage = 1) or entry `step` (per_stage = 0), nv × B each in the layout of opts.
 *   RBD_CONTROL_PD       : τ_i = tau_i − kp_i (q_i − q_des_i) − kd_i v_i on Revolute / Prismatic joints, on the stage state; τ = tau on every other joint's
 *                          coordinates (q_des NULL = 0, tau NULL = 0).
 * The controller sees the stage state that contact_dynamics! and dynamics! of that stage see.  Per stage: the integrator's stage launch, contact_head_kernel (the
 * per-body kinematics of the stage state and the PD law), contact_sim_kernel (s through the tableau, the contact model, the total wrenches), forward dynamics.
 * fp32 and fp64, both layouts, device pointers only (RBD_MEM_HOST: RBD_ERR_UNSUPPORTED); trees of at most 64 bodies; loop joints: RBD_ERR_UNSUPPORTED; no contact
 * points or no environment: RBD_ERR_INVALID_ARGUMENT (use rbd_simulate_controlled).  NULL control, q, v or s, dt <= 0, nsteps < 0, TABLE without tau, PD without
 * kp or kd, kind out of range: RBD_ERR_INVALID_ARGUMENT.  B == 0 or nsteps == 0: nothing is touched.  Only the first call of a workspace (or a larger B)
 * allocates; no call synchronises.  No derivative entry point covers it. */
int rbd_simulate_contact_controlled(rbd_ws_t* ws, int32_t B, void* q, void* v, void* s, const rbd_control_t* control, const void* fext, double dt,
                                    int32_t nsteps, const rbd_opts_t* opts);

/* ---- kinematics by-products of the same forward-kinematics pass (every output nullable; opts->memory as for rbd_dynamics) ---------------
 * momentum_matrix: 6×nv column-major per state, root frame, (angular; linear) — momentum_matrix!(out, state)
 *   src/mechanism_algorithms.jl:313-327;  com: 3×B — center_of_mass(state) :28-50;  energy: 2×B = (kinetic_energy,
 *   gravitational_potential_energy) src/mechanism_state.jl:886-903 (needs v).
 * Larger batches (from 8193 states on an MI355X: a wavefront of 64 states for every other CU) take kernels compiled for the mechanism with one lane per state (family 11; Atlas,
 * 65 536 fp64 states: momentum matrix 56 us, energies 34, Jacobian 46, momentum 41 against 207 / 149 / 164 on the lane-per-body kernels).  A column of the momentum
 * matrix / Jacobian leaves as the lane's own 48 bytes: callers that can take the batch-innermost layout (RBD_LAYOUT_SOA) get whole 512-byte runs instead. */
int rbd_kinematics(rbd_ws_t* ws, int32_t B, const void* q, const void* v, void* momentum_matrix, void* com, void* energy,
                   const rbd_opts_t* opts);

/* momentum(state) and momentum_rate_bias(state), root frame — src/mechanism_state.jl:878-884, :975-987.  out: 12×B per state =
 * (momentum: angular 3, linear 3; momentum_rate_bias: torque 3, force 3).  d/dt momentum = momentum_matrix·v̇ + momentum_rate_bias.
*/
int rbd_momentum(rbd_ws_t* ws, int32_t B, const void* q, const void* v, void* out, const rbd_opts_t* opts);

/* geometric_jacobian!(jac, state, path(mechanism, base, target)) in the root frame — src/mechanism_algorithms.jl:80-99, :126-131.
 * base_body / target_body: body indices of the flat model, -1 = the root body.  jac: 6×nv column-major per state, (angular; linear);
 * columns off the path are written as zeros. */
int rbd_geometric_jacobian(rbd_ws_t* ws, int32_t B, const void* q, int32_t base_body, int32_t target_body, void* jac, const rbd_opts_t* opts);

/* ---- multi-GPU: the one exchange step (SURVEY.md §8 e) -------------------------------------------------------------------------
 * The batch shards by state — rank g of G owns states [g·B/G, (g+1)·B/G), model constants replicated, NO collective inside the
 * dynamics — and the shards of DynamicsResult.v̇ are brought together by one RCCL all-gather (or gather to one rank) over xGMI.
 * One process per GPU.  rbd_comm_unique_id on one rank, the 128 bytes handed to the others by the caller (as with ncclGetUniqueId),
 * then rbd_comm_create on every rank.  rbd_gather is asynchronous on `stream`; gathered holds world × count scalars in rank order
 * (AOS buffers: the (world·B/G) × n matrix; SOA: one n × B/G block per rank).  librccl is opened on first use.                  */
typedef struct rbd_comm rbd_comm_t;
int rbd_comm_unique_id(void* id128);
int rbd_comm_create(const void* id128, int32_t world, int32_t rank, int32_t device, rbd_comm_t** out);
int rbd_comm_destroy(rbd_comm_t* comm);
int rbd_comm_info(const rbd_comm_t* comm, int32_t* world, int32_t* rank);
int rbd_gather(rbd_comm_t* comm, int32_t dtype, const void* shard, void* gathered, int64_t count, int32_t root /* < 0: every rank */, void* stream);
/* ... with shards of different sizes (a batch that does not divide by the number of ranks): counts[world] scalars per rank, the shards back to back in rank
 * order in `gathered`; an empty shard is legal.  Every rank passes the same counts: ranks that disagree wait for each other forever, like mismatched ncclSend /
 * ncclRecv sizes — unless RBD_COMM_CHECK=1 is set (on every rank), in which case the ranks compare their counts first (one small all-gather and a wait for the
 * stream) and a rank that finds a disagreement returns RBD_ERR_DIMENSION_MISMATCH. */
int rbd_gatherv(rbd_comm_t* comm, int32_t dtype, const void* shard, void* gathered, const int64_t* counts, int32_t root /* < 0: every rank */, void* stream);
const char* rbd_comm_last_error(void);

/* ---- forward-mode derivatives of inverse_dynamics! and dynamics! (since 700) ---------------------------------------------------------------------------
 * What ForwardDiff.jacobian / Dual numbers through the reference compute (its own test suite: test/test_mechanism_algorithms.jl:600-652), on tree
 * mechanisms of any size, every tree joint type, fp32 and fp64, both layouts:
 *  - the derivatives are those of the function the library evaluates, in the RAW coordinates q: a quaternion joint's transform is the unnormalised
 *    rotation(jt, q, false) (src/joint_types/quaternion_floating.jl:81-83), so a direction dq need not be tangent to the unit sphere, and a SinCosRevolute's
 *    (s, c) are two independent coordinates.  Lie-algebra (tangent-space) derivatives are not offered: compose with the q̇ = Q(q) v map
 *    (velocity_to_configuration_derivative!) yourself;
 *  - loop joints: RBD_ERR_HAS_LOOPS (as inverse_dynamics!, src/mechanism_algorithms.jl:549); contact points with an environment: RBD_ERR_UNSUPPORTED (as
 *    rbd_dynamics); RBD_MEM_HOST: RBD_ERR_UNSUPPORTED (device pointers only);
 *  - the value outputs equal rbd_inverse_dynamics / the CRBA + Cholesky route of rbd_dynamics (dynamics_solve! :764, :819) to rounding;
 *  - allocation: the first derivative call of a workspace allocates its buffers (M, its factor, the tangent right-hand sides and scratch) for
 *    max_batch states and nq + nv directions, a JVP call with more directions than any before allocates again; no other call allocates or synchronises;
 *  - rbd_workspace_last_kernel names the tangent kernel afterwards.
 * Tangents (JVPs): ntan directions per state (ntan <= 0: RBD_ERR_INVALID_ARGUMENT).  A tangent argument of n coordinates holds n·ntan values per state,
 * direction d of state b at rows d·n … d·n+n−1 of that state's n·ntan (layout per opts, as every batch buffer).  Every tangent input is nullable
 * (= zero direction); every value output is nullable.  dfext: 6·n_bodies per direction. */
int rbd_inverse_dynamics_jvp(rbd_ws_t* ws, int32_t B, int32_t ntan, const void* q, const void* v, const void* vdot,
                             const void* fext, const void* dq, const void* dv, const void* dvdot, const void* dfext,
                             void* tau_out, void* dtau_out, const rbd_opts_t* opts);
/* dv̇ by the implicit-function identity M(q) dv̇ = dτ − ∂ID(q, v, v̇)·(dq, dv, 0, dfext) at the v̇ of the same call: one Cholesky factor per state,
 * ntan triangular solves against it. */
int rbd_dynamics_jvp(rbd_ws_t* ws, int32_t B, int32_t ntan, const void* q, const void* v, const void* tau,
                     const void* fext, const void* dq, const void* dv, const void* dtau, const void* dfext,
                     void* vdot_out, void* dvdot_out, const rbd_opts_t* opts);
/* Full Jacobians, column-major per state like rbd_geometric_jacobian: nv×nq (∂/∂q), nv×nv (∂/∂v, ∂/∂v̇, ∂/∂τ); fext held fixed.  Every output
 * nullable; M_out = ∂τ/∂v̇ = M (the full square), dvdot_dtau = M⁻¹ (the full square).  Column j is the JVP along the j-th coordinate unit vector. */
int rbd_inverse_dynamics_derivatives(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* vdot, const void* fext,
                                     void* tau_out, void* dtau_dq, void* dtau_dv, void* M_out, const rbd_opts_t* opts);
int rbd_dynamics_derivatives(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* tau, const void* fext,
                             void* vdot_out, void* dvdot_dq, void* dvdot_dv, void* dvdot_dtau, const rbd_opts_t* opts);
/* Derivatives of simulate steps (700 additions): nsteps steps of rbd_simulate (the Munthe-Kaas RK4 step, src/ode_integrators.jl:233-299) with tangents
 * carried through every stage — for iLQR / DDP, shooting and differentiable simulation.  Semantics as above: raw coordinates q, tree mechanisms only
 * (RBD_ERR_HAS_LOOPS, RBD_ERR_UNSUPPORTED for contact points with an environment and for RBD_MEM_HOST), device pointers.
 *  - The value path is the reference's own route at every stage state: CRBA, Cholesky with the factor in the workspace, the solve (as rbd_dynamics_jvp).
 *    The updated q, v therefore equal rbd_simulate's to rounding, not bit for bit.
 *  - The derivatives are those of the smooth step map: the integrator's small-angle branches (θ < eps in the rotation-vector and exp / log maps of
 *    quaternion joints) are removable singularities, and their derivatives are taken in the limit, finite at θ = 0.
 *  - ntan <= 0, dt <= 0, nsteps < 0, or a NULL q, v, dq or dv: RBD_ERR_INVALID_ARGUMENT; B == 0 or nsteps == 0: a successful no-op.
 *  - Allocation: the first call of a workspace, and one with a wider pass of directions than any before; no other call allocates or synchronises.  The
 *    tangent buffers of one pass hold at most 2 GiB (2·nq + 6·nv values per direction and state, for max_batch states): more directions run as
 *    several passes, each starting again from the caller's (q, v).
 *  - rbd_workspace_last_kernel names the tangent kernels afterwards.
 * q, v, dq, dv are IN/OUT.  dtau and dfext are held over every stage of every step (zero-order hold, as rbd_simulate holds tau / fext); every one of
 * tau, fext, dtau, dfext is nullable.  dq: nq·ntan, dv / dtau: nv·ntan, dfext: 6·n_bodies·ntan per state, in the layout of the tangents above. */
int rbd_simulate_jvp(rbd_ws_t* ws, int32_t B, int32_t ntan, void* q, void* v, const void* tau, const void* fext, double dt, int32_t nsteps,
                     void* dq, void* dv, const void* dtau, const void* dfext, const rbd_opts_t* opts);
/* One step: q, v advanced in place.  x = (q; v), nx = nq + nv.  dx_dx: nx×nx, dx_dtau: nx×nv, column-major per state like rbd_geometric_jacobian;
 * column j is the JVP along the j-th unit vector.  Both are nullable; fext is held fixed. */
int rbd_simulate_step_derivatives(rbd_ws_t* ws, int32_t B, void* q, void* v, const void* tau, const void* fext, double dt,
                                  void* dx_dx, void* dx_dtau, const rbd_opts_t* opts);
/* Reverse mode (700 additions): vector-Jacobian products, the gradient of a scalar loss through inverse_dynamics! / dynamics! from one adjoint RNEA
 * pass per state, where the Jacobians above cost nq + nv tangent directions.  Semantics as the JVPs: raw coordinates q, tree mechanisms only
 * (RBD_ERR_HAS_LOOPS; RBD_ERR_UNSUPPORTED for contact points with an environment and for RBD_MEM_HOST), device pointers, fp32 and fp64, both layouts.
 *  - One cotangent per state, in the batch layout of opts: tau_bar (nv) for inverse dynamics, vdot_bar (nv) for dynamics.
 *  - Every output is nullable and OVERWRITTEN (not accumulated): q_bar = (∂/∂q)ᵀ·cotangent has nq rows, v_bar, vdot_bar and tau_bar nv, fext_bar 6·n_bodies.
 *  - A NULL q, v or cotangent, or a NULL vdot for inverse dynamics: RBD_ERR_INVALID_ARGUMENT; B == 0 is a successful no-op.
 *  - The value outputs (tau_out, vdot_out, nullable) equal rbd_inverse_dynamics / the CRBA + Cholesky route of rbd_dynamics to rounding.
 *  - Allocation: the first reverse-mode call of a workspace allocates its adjoint scratch for max_batch states (at most 1 GiB; larger batches run in
 *    slabs) and the buffers every derivative call shares; no later call allocates or synchronises.
 *  - rbd_workspace_last_kernel names the adjoint kernel afterwards.
 * rbd_inverse_dynamics_vjp: τ = ID(q, v, v̇, fext) and, with λ = tau_bar, q̄ = (∂τ/∂q)ᵀλ, v̄ = (∂τ/∂v)ᵀλ, v̇̄ = Mλ, f̄ext = (∂τ/∂fext)ᵀλ. */
int rbd_inverse_dynamics_vjp(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* vdot, const void* fext,
                             const void* tau_bar, void* tau_out, void* q_bar, void* v_bar, void* vdot_bar, void* fext_bar,
                             const rbd_opts_t* opts);
/* rbd_dynamics_vjp: v̇ by CRBA + Cholesky (the factor kept), λ = M⁻¹ vdot_bar with one triangular solve pair against it, τ̄ = λ and
 * (q̄, v̄, f̄ext) = −(∂ID/∂(q, v, fext))ᵀλ at (q, v, v̇) — the implicit-function identity of rbd_dynamics_jvp, transposed. */
int rbd_dynamics_vjp(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* tau, const void* fext,
                     const void* vdot_bar, void* vdot_out, void* q_bar, void* v_bar, void* tau_bar, void* fext_bar,
                     const rbd_opts_t* opts);
/* rbd_simulate_vjp (700 addition): reverse mode through nsteps steps of rbd_simulate_jvp's integrator — the gradient of a scalar loss of the final state,
 * one cotangent per state, from a forward pass that keeps the step starts and a backward pass of four dynamics VJPs and stage-map pullbacks per step.
 *  - q, v: IN/OUT, advanced by nsteps as rbd_simulate_jvp does (the CRBA + Cholesky value route at every stage: rbd_simulate's state to rounding).
 *  - q_bar (nq), v_bar (nv): IN/OUT — the cotangent of the final (q, v) on entry, that of the initial (q, v) on return.
 *  - tau_bar (nv), fext_bar (6·n_bodies): nullable, OVERWRITTEN with the gradient in the held τ / fext, summed over every stage of every step.
 *  - Semantics as the other derivative entry points (raw coordinates, tree mechanisms only, RBD_ERR_UNSUPPORTED for contact points with an environment
 *    and for RBD_MEM_HOST, device pointers, fp32 and fp64, both layouts); dt <= 0, nsteps < 0 or a NULL q, v, q_bar or v_bar:
 *    RBD_ERR_INVALID_ARGUMENT; B == 0 is a no-op; nsteps == 0 leaves q, v, q_bar, v_bar and zeroes tau_bar / fext_bar.
 *  - Step starts are kept while nsteps·(nq + nv)·B values fit in 1 GiB, else every ⌈√nsteps⌉-th, one segment's others recomputed (two-level
 *    checkpointing).  The first call of a workspace allocates, and a call that needs more room for step starts than any before; nothing else does.
 *  - Per-step torques: one call per step (the cotangent chains through q_bar, v_bar). */
int rbd_simulate_vjp(rbd_ws_t* ws, int32_t B, void* q, void* v, const void* tau, const void* fext, double dt, int32_t nsteps,
                     void* q_bar, void* v_bar, void* tau_bar, void* fext_bar, const rbd_opts_t* opts);

/* Point kinematics (700 addition): positions, velocities, accelerations and Jacobians of P points fixed to bodies, and the pullback of positions and
 * velocities.  Points are expressed in the ROOT frame and paths run from the world: the reference's transform(state, point, world), point_velocity,
 * point_acceleration and point_jacobian! of path(world → body).  Tree mechanisms only (RBD_ERR_HAS_LOOPS: loop joints are out of scope here, and so
 * is relative_acceleration between two bodies); fp32 and fp64, both layouts, trees of any size, every tree joint type.
 * rbd_workspace_set_points: P points from HOST arrays, point k fixed to body body[k] (a flat-model body index, 0 … n_bodies − 1; several points may share
 * a body) at r[3k … 3k + 2] in that body's frame — the frame whose transform to root the per-body outputs return.  The call copies the points and builds
 * the path tables; it may allocate and synchronise.  npoints == 0 clears the points; a body index out of range is RBD_ERR_INVALID_ARGUMENT. */
int rbd_workspace_set_points(rbd_ws_t* ws, int32_t npoints, const int32_t* body, const double* r);
/* Every output is nullable; batch buffers in the layout of opts, RBD_MEM_HOST as rbd_geometric_jacobian.  Per state:
 *  - pos (3P) = R_b r + p_b;  vel (3P) = ω_b × pos + v_b with (ω_b; v_b) the body's twist with respect to the world (needs v);
 *  - acc (3P) = α_b × pos + a_b + ω_b × vel with (α_b; a_b) the body's spatial acceleration relative to the world, without gravity (needs v; a NULL
 *    vdot means v̇ = 0: acc is then the bias term J̇v of task-space control);
 *  - jac (3·nv·P): for point k a 3×nv column-major block whose column of a velocity coordinate of a joint on path(world → body[k]) is
 *    ang(S) × pos + lin(S), S that coordinate's motion subspace column in the root frame; the other columns are written as zeros.
 * No points set, a NULL q, or vel / acc without v: RBD_ERR_INVALID_ARGUMENT; B == 0 is a successful no-op.  The call neither allocates nor synchronises
 * (device memory).  rbd_workspace_last_kernel names the kernel afterwards. */
int rbd_point_kinematics(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* vdot, void* pos, void* vel, void* acc, void* jac,
                         const rbd_opts_t* opts);
/* The pullback of (pos, vel): one cotangent per output and state, pos_bar and vel_bar of 3P values each, either nullable (zero) but not both.
 * q_bar (nq) and v_bar (nv) are nullable and OVERWRITTEN; the pullback is in the RAW coordinates q, exactly as rbd_inverse_dynamics_vjp defines them.
 * Device pointers only; errors as the other VJPs.  The first call of a workspace allocates the adjoint scratch (unless a reverse-mode call did). */
int rbd_point_kinematics_vjp(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* pos_bar, const void* vel_bar, void* q_bar, void* v_bar,
                             const rbd_opts_t* opts);

/* Reverse mode through soft contact (700 addition): the pullbacks of rbd_contact_dynamics and of rbd_dynamics_contact for a mechanism with contact points and
 * an environment — the reference's default point model (Hunt–Crossley normal force, viscoelastic Coulomb friction, half-spaces), differentiated on the branch
 * the forward pass takes per (point, half-space) pair: outside (every cotangent zero), clamped normal force, sticking, slipping.  On a branch boundary the
 * model is not differentiable and the result is that of the branch taken; a Hunt–Crossley exponent n < 1 at zero penetration is not finite.
 * Semantics as the other VJPs: raw coordinates q, device pointers only (RBD_MEM_HOST: RBD_ERR_UNSUPPORTED), loop joints RBD_ERR_HAS_LOOPS, fp32 and fp64,
 * both layouts, trees of any size; a mechanism without contact points or without an environment: RBD_ERR_INVALID_ARGUMENT (as rbd_contact_dynamics);
 * a NULL q, v or s, or every cotangent NULL: RBD_ERR_INVALID_ARGUMENT; B == 0 is a successful no-op.  s (ns = 3·points·half-spaces) is const: the VJPs do
 * not reset it.  Every output is nullable and OVERWRITTEN.  The first call of a workspace allocates (what every reverse-mode call shares, the contact
 * points' path tables — kept apart from rbd_workspace_set_points' —, the per-point cotangents); no later call allocates or synchronises.
 * rbd_workspace_last_kernel names contact_adjoint_kernel afterwards.
 * rbd_contact_dynamics_vjp — pullback of contact_dynamics!: (cw_bar [6·n_bodies], sdot_bar [ns], s_out_bar [ns]) -> (q_bar, v_bar, s_bar); s_out is the
 * friction state after the resets; any cotangent nullable (zero), not all three. */
int rbd_contact_dynamics_vjp(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* s, const void* cw_bar, const void* sdot_bar,
                             const void* s_out_bar, void* q_bar, void* v_bar, void* s_bar, const rbd_opts_t* opts);
/* rbd_dynamics_contact_vjp — pullback of dynamics!(result, state, τ, wext) with contact points, the ODE form (q, v, s, τ, wext) -> (v̇, ṡ, s after the
 * resets): the forward contact launch, rbd_dynamics_vjp's pass at the total wrenches (its f̄ext is their cotangent: fext_bar, and the contact wrenches'),
 * the contact model's pullback, and the contact points' kinematics pulled back and added to q̄, v̄.  vdot_bar may be NULL (zero) when sdot_bar or s_out_bar
 * is given; vdot_out (nv) and sdot_out (ns) are nullable value outputs (the CRBA + Cholesky route, as rbd_dynamics_vjp). */
int rbd_dynamics_contact_vjp(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* s, const void* tau, const void* fext,
                             const void* vdot_bar, const void* sdot_bar, const void* s_out_bar, void* vdot_out, void* sdot_out,
                             void* q_bar, void* v_bar, void* s_bar, void* tau_bar, void* fext_bar, const rbd_opts_t* opts);
/* rbd_simulate_contact_vjp (700 addition): reverse mode through nsteps steps of rbd_simulate_contact — the gradient of a scalar loss of the final state
 * (q, v, s), one cotangent per state: rbd_simulate_vjp's checkpointed RK4 adjoint with the friction state s carried through the tableau in both directions
 * and, at every stage state, rbd_dynamics_contact_vjp's composition (the forward contact launch, the dynamics VJP at the total wrenches, the contact
 * model's pullback, the contact points' kinematic pullback).
 *  - q, v, s: IN/OUT, advanced by nsteps (the CRBA + Cholesky value route at every stage state: rbd_simulate_contact's state to rounding).
 *  - q_bar (nq), v_bar (nv), s_bar (ns): IN/OUT, all required — the cotangent of the final state on entry, that of the initial state on return.
 *  - tau_bar (nv), fext_bar (6·n_bodies): nullable, OVERWRITTEN with the gradient in the held τ / fext, summed over every stage of every step.
 *  - The gradient is that of the branch each (point, half-space) pair takes AT EACH STAGE STATE; a pair may change branch between stages and steps.  The
 *    reset of an outside pair's friction state happens in the stage state only and never reaches the state after the step, as in rbd_simulate_contact.
 *  - Semantics as rbd_dynamics_contact_vjp (raw coordinates, device pointers only, fp32 and fp64, both layouts, trees of any size; RBD_MEM_HOST:
 *    RBD_ERR_UNSUPPORTED; loop joints: RBD_ERR_HAS_LOOPS; no contact points or no environment: RBD_ERR_INVALID_ARGUMENT — use rbd_simulate_vjp).
 *    dt <= 0, nsteps < 0 or a NULL q, v, s, q_bar, v_bar or s_bar: RBD_ERR_INVALID_ARGUMENT; B == 0 is a no-op; nsteps == 0 leaves the state and the
 *    three cotangents and zeroes tau_bar / fext_bar.
 *  - Step starts (q, v, s) are kept while nsteps·(nq + nv + ns)·B values fit in 1 GiB, else two-level checkpointing as rbd_simulate_vjp.  The first call
 *    of a workspace allocates, and a call that needs more room for step starts than any before; nothing else allocates or synchronises.
 *  - rbd_workspace_last_kernel names contact_stage_adjoint_kernel afterwards, among the others.  Per-step torques: one call per step. */
int rbd_simulate_contact_vjp(rbd_ws_t* ws, int32_t B, void* q, void* v, void* s, const void* tau, const void* fext, double dt, int32_t nsteps,
                             void* q_bar, void* v_bar, void* s_bar, void* tau_bar, void* fext_bar, const rbd_opts_t* opts);

/* Forward mode through soft contact (700 addition): the tangents and Jacobians of rbd_contact_dynamics and of rbd_dynamics_contact for a mechanism with
 * contact points and an environment — what ForwardDiff computes through dynamics! of such a mechanism.  One pass: the tangent RNEA of rbd_dynamics_jvp
 * carries every body's (R, p, twist) with its tangents; between its two sweeps each (state, chunk of directions) thread forms every contact point's Dual
 * position, velocity and friction state, evaluates the pair model on them and subtracts the tangent of the point's wrench from its body's; the existing
 * multi-right-hand-side solve finishes dv̇.  No second walk over the tree, no per-direction wrench buffer.
 *  - Tangents as rbd_dynamics_jvp: ntan directions, direction d of a tangent of n coordinates at rows d·n … d·n+n−1 of the state's ntan·n; every tangent
 *    input nullable (a zero direction), every output nullable and OVERWRITTEN; ds, dsdot_out, ds_out_out have n = ns = 3·points·half-spaces; raw coordinates q.
 *  - Contact model as rbd_dynamics_contact_vjp: the derivative of the branch each (point, half-space) pair takes — outside, clamped, sticking, slipping —, an
 *    outside pair contributing exact zeros; the tangent of s after the resets is ds for inside pairs and 0 for outside pairs; s is const and not reset; on a
 *    branch boundary the result is that of the branch taken.
 *  - Values: vdot_out (nv), sdot_out (ns), nullable, equal rbd_dynamics_contact_vjp's to rounding (the forward contact launch, then CRBA + Cholesky at the
 *    total wrenches).
 *  - Errors: a mechanism without contact points or without an environment, ntan <= 0, a NULL q, v or s: RBD_ERR_INVALID_ARGUMENT; loop joints:
 *    RBD_ERR_HAS_LOOPS; RBD_MEM_HOST: RBD_ERR_UNSUPPORTED; B beyond the workspace's batch: RBD_ERR_DIMENSION_MISMATCH; B == 0 is a successful no-op.
 *  - fp32 and fp64, both layouts, trees of any size, every tree joint type.  The first call of a workspace allocates (what the forward- and reverse-mode
 *    contact calls share, the right-hand sides for max(ntan, nq + nv + ns) directions); a JVP call with more directions than any before allocates again;
 *    nothing else allocates or synchronises.  rbd_workspace_last_kernel names tangent_contact_rnea_kernel afterwards, among the others.
 * rbd_contact_dynamics_jvp — tangent of contact_dynamics!: (dq, dv, ds) -> (dcw [6·n_bodies·ntan], dsdot [ns·ntan], ds_out [ns·ntan]); the tangent pass
 * stops after the contact step (no wrench sweep). */
int rbd_contact_dynamics_jvp(rbd_ws_t* ws, int32_t B, int32_t ntan, const void* q, const void* v, const void* s,
                             const void* dq, const void* dv, const void* ds,
                             void* dcw_out, void* dsdot_out, void* ds_out_out, const rbd_opts_t* opts);
/* rbd_dynamics_contact_jvp — tangent of dynamics!(result, state, τ, wext) with contact points, the ODE form (q, v, s, τ, wext) -> (v̇, ṡ, s after the
 * resets): M dv̇ = dτ − ∂ID(q, v, v̇)·(dq, dv, 0, dfext + d contactwrenches); dvdot_out (nv·ntan), dsdot_out, ds_out_out (ns·ntan).  Without dvdot_out there
 * is no wrench sweep and no solve. */
int rbd_dynamics_contact_jvp(rbd_ws_t* ws, int32_t B, int32_t ntan, const void* q, const void* v, const void* s,
                             const void* tau, const void* fext,
                             const void* dq, const void* dv, const void* ds, const void* dtau, const void* dfext,
                             void* vdot_out, void* sdot_out, void* dvdot_out, void* dsdot_out, void* ds_out_out,
                             const rbd_opts_t* opts);
/* rbd_dynamics_contact_derivatives — the full Jacobians, column-major per state like rbd_dynamics_derivatives, fext held fixed: dvdot_dq nv×nq, dvdot_dv
 * nv×nv, dvdot_ds nv×ns, dvdot_dtau nv×nv = M⁻¹ (the full square); dsdot_dq ns×nq, dsdot_dv ns×nv, dsdot_ds ns×ns (ṡ does not depend on τ).  Column j is
 * the JVP along the j-th unit vector of (q; v; s): the columns of (q; v) in one tangent pass, those of s in a second.  Every output nullable; a pass none
 * of whose outputs is asked for is not launched. */
int rbd_dynamics_contact_derivatives(rbd_ws_t* ws, int32_t B, const void* q, const void* v, const void* s,
                                     const void* tau, const void* fext, void* vdot_out, void* sdot_out,
                                     void* dvdot_dq, void* dvdot_dv, void* dvdot_ds, void* dvdot_dtau,
                                     void* dsdot_dq, void* dsdot_dv, void* dsdot_ds, const rbd_opts_t* opts);

/* Forward mode through simulate steps with soft contact (700 addition): rbd_simulate_jvp / rbd_simulate_step_derivatives with the friction state s beside
 * (q, v), as in rbd_simulate_contact_vjp — the tangents of rbd_simulate_contact's steps and the step Jacobians A = ∂x⁺/∂x, B = ∂x⁺/∂τ with x = (q; v; s),
 * what iLQR / DDP, multiple shooting and Gauss–Newton need of a mechanism with contact points.
 *  - q, v, s: IN/OUT, advanced by nsteps steps on rbd_simulate_contact_vjp's value route (at every stage state the forward contact launch on a copy of the
 *    stage's s, then CRBA + Cholesky at the total wrenches): rbd_simulate_contact's state to rounding, not bit for bit.
 *  - dq (nq·ntan), dv (nv·ntan), ds (ns·ntan): IN/OUT, all required; dtau (nv·ntan), dfext (6·n_bodies·ntan): nullable, held over every stage of every
 *    step.  Direction d of an n-coordinate tangent at rows d·n … d·n+n−1, as in every other JVP; raw coordinates q.
 *  - The derivative is that of the branch each (point, half-space) pair takes AT EACH STAGE STATE, an outside pair contributing exact zeros; on a branch
 *    boundary it is that of the branch taken.  The reset of an outside pair's friction state happens in the stage state only and reaches neither s⁺ nor ds⁺.
 *    The integrator's small-angle branches are differentiated in the limit, as in rbd_simulate_jvp.
 *  - Errors: no contact points or no environment: RBD_ERR_INVALID_ARGUMENT (use rbd_simulate_jvp); loop joints: RBD_ERR_HAS_LOOPS; RBD_MEM_HOST:
 *    RBD_ERR_UNSUPPORTED; ntan <= 0, dt <= 0, nsteps < 0, or a NULL q, v, s, dq, dv or ds: RBD_ERR_INVALID_ARGUMENT; B beyond the workspace's batch:
 *    RBD_ERR_DIMENSION_MISMATCH; B == 0 or nsteps == 0: a successful no-op.  fp32 and fp64, both layouts, trees of any size, every tree joint type.
 *  - Allocation: the first call of a workspace, and one whose pass of directions is wider than any before; nothing else allocates or synchronises.  One pass
 *    holds 2·nq + 6·nv + 4·ns tangent values per direction and state (for max_batch states), at most 2 GiB: more directions run as several passes, each
 *    starting again from the caller's (q, v, s).
 *  - rbd_workspace_last_kernel names tangent_contact_stage_kernel afterwards, among the others. */
int rbd_simulate_contact_jvp(rbd_ws_t* ws, int32_t B, int32_t ntan, void* q, void* v, void* s, const void* tau, const void* fext, double dt,
                             int32_t nsteps, void* dq, void* dv, void* ds, const void* dtau, const void* dfext, const rbd_opts_t* opts);
/* One step: q, v, s advanced in place.  x = (q; v; s), nx = nq + nv + ns.  dx_dx: nx×nx, dx_dtau: nx×nv, column-major per state; column j is the JVP along
 * the j-th unit vector (made on the device).  Both are nullable — a block none of whose outputs is asked for is not run —; fext is held fixed. */
int rbd_simulate_contact_step_derivatives(rbd_ws_t* ws, int32_t B, void* q, void* v, void* s, const void* tau, const void* fext, double dt,
                                          void* dx_dx, void* dx_dtau, const rbd_opts_t* opts);

/* ---- diagnostics ------------------------------------------------------------ */
const char* rbd_status_string(int status);
const char* rbd_last_hip_error(void);   /* thread-local text of the last HIP failure     */
/* average device time (ms) of the dominant kernel of the last hot-path call on this
 * workspace, measured with hipEvents recorded around the launch on ws's stream.
 * Timing is off by default; enable=1 brackets every launch with events.            */
int rbd_workspace_enable_timing(rbd_ws_t* ws, int32_t enable);
int rbd_workspace_last_kernel_ms(rbd_ws_t* ws, float* ms);
/* name of the articulated-body kernel (lane mapping) the last rbd_dynamics / rbd_simulate / rbd_mass_matrix_solve call launched */
const char* rbd_workspace_last_kernel(const rbd_ws_t* ws);
/* 100·round + revision of this header.  rbd_flat_model_t grew its four contact fields at 200; a caller built against an older header must
 * not call a newer library (the Python and Julia loaders compare this with the value they were written for).  400: rbd_workspace_set_loop_gains.
 * 500: rbd_mass_matrix_solve_packed, rbd_gatherv.  600: rbd_jit_check_walk_object; no size limit left on any entry point; program family 11; family 1 in fp64.
 * 700: forward-mode derivatives — rbd_inverse_dynamics_jvp, rbd_dynamics_jvp, rbd_inverse_dynamics_derivatives, rbd_dynamics_derivatives;
 *      added to 700 without a new version: rbd_simulate_jvp, rbd_simulate_step_derivatives (derivatives of simulate steps);
 *      rbd_inverse_dynamics_vjp, rbd_dynamics_vjp (reverse mode); rbd_simulate_vjp (reverse mode through simulate steps);
 *      rbd_workspace_set_points, rbd_point_kinematics, rbd_point_kinematics_vjp (point kinematics);
 *      rbd_contact_dynamics_vjp, rbd_dynamics_contact_vjp (reverse mode through soft contact);
 *      rbd_simulate_contact_vjp (reverse mode through simulate steps with soft contact);
 *      rbd_contact_dynamics_jvp, rbd_dynamics_contact_jvp, rbd_dynamics_contact_derivatives (forward mode through soft contact);
 *      rbd_simulate_contact_jvp, rbd_simulate_contact_step_derivatives (forward mode through simulate steps with soft contact);
 *      rbd_simulate_contact_controlled (simulate with soft contact under a device-side controller); rbd_mk_stage takes mechanisms with contact points. */
#define RBD_HIP_H_VERSION 700
int rbd_version(void);
/* Run-time specialisation.  The one-lane-per-state kernels (mass_matrix! and mass_matrix! + Cholesky at large batches) exist in a second form
 * that is compiled for the mechanism at hand with hiprtc the first time a workspace needs it (the walk of the tree, joint types, offsets and
 * body constants become compile-time constants — what Julia's JIT does for the reference's `mass_matrix!`), cached on disk beside the library
 * (jit_cache/) or in $RBD_JIT_CACHE.  Without libhiprtc, or with RBD_JIT=0, the interpreting kernels run instead; results agree to rounding.
 * One program per family of kernels and scalar type — family 0: mass_matrix! (+ the sparse tile Cholesky and the emitter of M in fp32), 1: dynamics!
 * (fp32; since 600 fp64 for mechanisms with 3-dof joints / 6-dof joints below the world), 2: inverse_dynamics! / dynamics_bias! (fp32; fp64), 3: the whole loop-joint branch of dynamics! for small loop mechanisms (<= 4 bodies, nv <= 4,
 * nc <= 6: the four-bar linkage), 4 / 5: the one-wavefront-per-track kernels of dynamics! / inverse_dynamics! (batches beyond what the two-bodies-per-lane kernels hold at once), 6 / 7: the same with two
 * fp32 states per lane, 8: the two-bodies-per-lane kernels themselves (small batches — the bench workload — with the loops over the tree's levels unrolled against the
 * mechanism's level structure), 9 / 10: 4 / 6 with the four stages of a `simulate` step in one launch, 11 (since 600): the kinematics by-products one lane per state
 * (rbd_kinematics / rbd_geometric_jacobian / rbd_momentum at large batches: kin_spec, energy_spec, com_spec, jac_spec, mom_spec) — each compiled when a workspace first takes
 * that route.  Families 0-2 and 11 take every tree joint type; 4-7, 9, 10 and the fast form of 8 trees of 1-dof / fixed joints with 6-dof joints on the world.
 * rbd_jit_precompile compiles all of a model's programs of one scalar type (RBD_F32 / RBD_F64) into the cache ahead of time (no device needed);
 * rbd_jit_source returns the generated source of one (length without the terminator; buf may be NULL; -1: no such program for this mechanism). */
int rbd_jit_precompile(const rbd_model_t* model, int32_t dtype, char* log, int64_t log_capacity);
/* Compilation never blocks a hot-path call (since 400): a call that would use a program that is not in the cache starts its compilation on a background thread,
 * runs the interpreting kernel, and the first call after the compiler has finished switches over (RBD_JIT_ASYNC=0: the first call waits instead, as does a
 * call that names the compiled kernel, RBD_ALGO_ABA_COMPILED).  rbd_jit_precompile is the blocking form (all programs of the model in parallel; the log lists
 * the seconds each took).  rbd_jit_status is the non-blocking query for ONE program (family as above): 1 = ready, 0 = being compiled (started by this
 * call if nobody had), -1 = no such program / no hiprtc / compilation failed. */
int rbd_jit_status(const rbd_model_t* model, int32_t dtype, int32_t family);
/* Waits for every compilation this process has started in the background (no-op when there is none).  A host process calls it before it exits — the
 * Python mirror and the Julia shim register it with their `atexit`: the compiler's own teardown at process exit does not wait for a thread that is still
 * inside it (a process that exited seconds after its first large-batch call on a new mechanism ended in a segmentation fault). */
void rbd_jit_wait_idle(void);
int64_t rbd_jit_source(const rbd_model_t* model, int32_t dtype, int32_t family, char* buf, int64_t capacity);
/* The admission test the library applies to the code object of a one-wavefront-per-track ("walk") program before it loads it, on an object the caller hands in
 * (diagnostics and tests; host only, nothing is loaded).  Those kernels keep per-joint results in accumulation registers addressed BY NUMBER, counted down from a255
 * (csrc/rbd_walk.hpp WalkStash), behind the compiler's back.  Admitted: no scratch; the metadata's .agpr_count == 0 and <= 248 VGPRs — or, for the `simulate` program
 * whose source carries the marker "// rbd-walk-sim-loop stash-from=a<N>" (its register allocator may take accumulation registers of its own: a0 upwards), .agpr_count
 * <= N, so that the allocator's registers and the stash cannot alias whatever is live when; and a kernel descriptor of the known kind (AMDGPU HSA code object v5 / v6,
 * gfx950) that could be rewritten to cover all 256 accumulation registers.  RBD_OK: would be loaded; RBD_ERR_UNSUPPORTED: refused (log says why) — the kernels that
 * interpret the mechanism, or the four-launch form of `simulate`, serve then. */
int rbd_jit_check_walk_object(const char* source, const void* code, int64_t size, char* log, int64_t log_capacity);

#ifdef __cplusplus
}
#endif
#endif /* RBD_HIP_H */
