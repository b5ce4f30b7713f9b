# RigidBodyDynamicsGPU.jl — thin `ccall` shim that places librbd_hip.so (include/rbd_hip.h) under
# RigidBodyDynamics.jl's own generics for the batched hot path.
#
# EXPERIMENTAL / NOT EXECUTED IN THIS REPO: the build image has no Julia toolchain (SURVEY.md F3).  The file shows the binding a
# maintainer of the reference would add; the tested boundary is the C ABI itself (tests/ drive it through ctypes), and
# scripts/check_julia_ccalls.py (run by tests/test_capi_symbols.py) checks every `ccall` here against include/rbd_hip.h — symbol
# name, argument count, pointer-vs-integer kind of every argument — so the shim cannot drift from the header unnoticed.
#
# Usage sketch:
#     using RigidBodyDynamics, RigidBodyDynamicsGPU
#     mechanism = parse_urdf("atlas.urdf", floating = true)
#     state  = BatchedMechanismState(mechanism, 4096)            # q :: nq × B, v :: nv × B (one state per column), DEVICE resident
#     result = BatchedDynamicsResult(mechanism, 4096)
#     copyto!(state.q, qhost); copyto!(state.v, vhost)           # or storage = :host for plain Matrix buffers (PCIe inside every call)
#     dynamics!(result, state, τ)                                 # τ :: nv × B ; fills result.v̇, result.q̇ (asynchronous; synchronize(state))
#     inverse_dynamics!(τout, jointwrenches, accelerations, state, v̇, externalwrenches)
#     mass_matrix!(result, state) ; dynamics_bias!(result, state) ; dynamics!(ẋ, result, state, x)
module RigidBodyDynamicsGPU

using RigidBodyDynamics
using RigidBodyDynamics: Mechanism, MechanismState, DynamicsResult, Joint, JointType, Revolute, Prismatic, Fixed, Planar, QuaternionSpherical,
    QuaternionFloating, SinCosRevolute, RigidBody, BodyID, Wrench, tree_joints, non_tree_joints, predecessor, successor, joint_to_predecessor,
    joint_to_successor, spatial_inertia, joint_type, num_positions, num_velocities, num_constraints, root_body, modcount, bodies, JointID
using RigidBodyDynamics.PDControl: SE3PDGains
using RigidBodyDynamics.Spatial: rotation, translation, angular, linear
# the generics this file adds methods to (src/RigidBodyDynamics.jl:143-155 exports them)
import RigidBodyDynamics: dynamics!, inverse_dynamics!, mass_matrix!, dynamics_bias!, momentum_matrix!, geometric_jacobian!, center_of_mass,
    kinetic_energy, gravitational_potential_energy, momentum, momentum_rate_bias, simulate
using LinearAlgebra

export BatchedMechanismState, BatchedDynamicsResult, DeviceMatrix, RbdComm, gather!, gatherv!, mass_matrix_solve_packed!, synchronize, librbd_hip, TorqueTable, PDControl,
    inverse_dynamics_jvp!, dynamics_jvp!, inverse_dynamics_derivatives!, dynamics_derivatives!, simulate_jvp!, simulate_step_derivatives!,
    inverse_dynamics_vjp!, dynamics_vjp!, simulate_vjp!, set_points!, point_kinematics!, point_jacobian!, point_velocity!, point_kinematics_vjp!,
    contact_dynamics_vjp!, dynamics_contact_vjp!, simulate_contact_vjp!, contact_dynamics_jvp!, dynamics_contact_jvp!, dynamics_contact_derivatives!,
    simulate_contact_jvp!, simulate_contact_step_derivatives!

const librbd_hip = Ref("librbd_hip.so")   # set to <repo>/rigidbodydynamics.jl_amd/csrc/librbd_hip.so
const libhip = Ref("libamdhip64.so")

# ---- status codes -> Julia exceptions (same types the reference throws) --------------------------------------
function check(status::Cint, where::String)
    status == 0 && return nothing
    msg = unsafe_string(ccall((:rbd_status_string, librbd_hip[]), Cstring, (Cint,), status))
    status == 1 && throw(ArgumentError("$where: $msg"))
    status == 2 && throw(DimensionMismatch("$where: $msg"))
    status == 7 && error("This method can currently only handle tree Mechanisms.")   # mechanism_algorithms.jl:549
    status == 8 && throw(PosDefException(0))                                          # LAPACK.potrf!
    error("$where: $msg ($(unsafe_string(ccall((:rbd_last_hip_error, librbd_hip[]), Cstring, ()))))")
end

# ---- device-resident n × B buffers without a GPU array package: hipMalloc / hipMemcpy straight from libamdhip64 -------------------
mutable struct DeviceMatrix{T}
    ptr::Ptr{T}
    dims::NTuple{2, Int}
end
function DeviceMatrix{T}(n::Integer, B::Integer) where {T}
    p = Ref{Ptr{Cvoid}}(C_NULL)
    ccall((:hipMalloc, libhip[]), Cint, (Ref{Ptr{Cvoid}}, Csize_t), p, max(1, n * B) * sizeof(T)) == 0 || error("hipMalloc failed")
    ccall((:hipMemset, libhip[]), Cint, (Ptr{Cvoid}, Cint, Csize_t), p[], 0, max(1, n * B) * sizeof(T))
    d = DeviceMatrix{T}(Ptr{T}(p[]), (Int(n), Int(B)))
    finalizer(x -> ccall((:hipFree, libhip[]), Cint, (Ptr{Cvoid},), x.ptr), d)
    d
end
Base.size(d::DeviceMatrix) = d.dims
Base.size(d::DeviceMatrix, i) = d.dims[i]
Base.pointer(d::DeviceMatrix) = d.ptr
Base.unsafe_convert(::Type{Ptr{T}}, d::DeviceMatrix{T}) where {T} = d.ptr
function Base.copyto!(d::DeviceMatrix{T}, h::AbstractMatrix{T}) where {T}     # host -> device
    size(h) == d.dims || throw(DimensionMismatch())
    hc = Matrix{T}(h)
    ccall((:hipMemcpy, libhip[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Cint), d.ptr, hc, sizeof(hc), 1) == 0 || error("hipMemcpy failed")
    d
end
function Base.copyto!(h::Matrix{T}, d::DeviceMatrix{T}) where {T}             # device -> host
    size(h) == d.dims || throw(DimensionMismatch())
    ccall((:hipMemcpy, libhip[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Csize_t, Cint), h, d.ptr, sizeof(h), 2) == 0 || error("hipMemcpy failed")
    h
end
Base.Array(d::DeviceMatrix{T}) where {T} = copyto!(Matrix{T}(undef, d.dims...), d)
const Buffer{T} = Union{Matrix{T}, DeviceMatrix{T}}
newbuffer(::Val{:device}, ::Type{T}, n, B) where {T} = DeviceMatrix{T}(n, B)
newbuffer(::Val{:host}, ::Type{T}, n, B) where {T} = zeros(T, n, B)

# ---- C structs (field order == include/rbd_hip.h) -------------------------------------------------------------
struct RbdLoopJoint
    predecessor::Int32; successor::Int32; joint_type::Int32; _pad::Int32
    axis::NTuple{3, Float64}
    pred_rot::NTuple{9, Float64}; pred_trans::NTuple{3, Float64}
    succ_rot::NTuple{9, Float64}; succ_trans::NTuple{3, Float64}
    rotation_from_z_aligned::NTuple{9, Float64}
    gains::NTuple{4, Float64}
end

struct RbdContactPoint        # DefaultContactPoint: src/contact.jl:72-77, :196
    body::Int32; _pad::Int32
    location::NTuple{3, Float64}
    hc_k::Float64; hc_lambda::Float64; hc_n::Float64     # HuntCrossleyModel
    mu::Float64; k::Float64; b::Float64                  # ViscoelasticCoulombModel
end
struct RbdHalfSpace           # HalfSpace3D: src/contact.jl:202-222
    point::NTuple{3, Float64}; outward_normal::NTuple{3, Float64}
end

struct RbdFlatModel
    n_bodies::Int32; nq::Int32; nv::Int32; n_loops::Int32
    parent::Ptr{Int32}; joint_type::Ptr{Int32}; q_offset::Ptr{Int32}; v_offset::Ptr{Int32}
    joint_axis::Ptr{Float64}; joint_axis2::Ptr{Float64}
    pred_rot::Ptr{Float64}; pred_trans::Ptr{Float64}
    inertia_moment::Ptr{Float64}; inertia_cross::Ptr{Float64}; inertia_mass::Ptr{Float64}
    gravity::NTuple{3, Float64}
    loops::Ptr{RbdLoopJoint}
    n_contact_points::Int32; n_halfspaces::Int32
    contact_points::Ptr{RbdContactPoint}; halfspaces::Ptr{RbdHalfSpace}
end

struct RbdOpts
    layout::Int32; memory::Int32; algorithm::Int32; stabilization::Int32
end
struct RbdControl             # device-side controllers of rbd_simulate_controlled (include/rbd_hip.h)
    kind::Int32; per_stage::Int32
    tau::Ptr{Cvoid}; q_des::Ptr{Cvoid}; kp::Ptr{Cvoid}; kd::Ptr{Cvoid}
end
const LAYOUT_AOS = Int32(1)    # Julia n × B column-major == one state per column
const MEM_DEVICE, MEM_HOST = Int32(0), Int32(1)

jointtag(::Fixed) = Int32(0); jointtag(::Revolute) = Int32(1); jointtag(::Prismatic) = Int32(2)
jointtag(::QuaternionFloating) = Int32(3); jointtag(::Planar) = Int32(4); jointtag(::QuaternionSpherical) = Int32(5)
jointtag(::SinCosRevolute) = Int32(6)
jointtag(jt::JointType) = throw(ArgumentError("joint type $(typeof(jt)) is not supported by librbd_hip (e.g. SPQuatFloating)"))
jointaxis(jt::Union{Revolute, Prismatic, SinCosRevolute}) = Tuple(Float64.(jt.axis))
jointaxis(jt::Planar) = Tuple(Float64.(jt.x_axis))          # planar.jl: translation along x_axis / y_axis, rotation about x × y
jointaxis(::JointType) = (0.0, 0.0, 0.0)
jointaxis2(jt::Planar) = Tuple(Float64.(jt.y_axis))
jointaxis2(::JointType) = (0.0, 0.0, 0.0)
rowmajor(R) = Float64[R[i, j] for i in 1:3 for j in 1:3]    # the C side stores rotations row-major

# ---- flatten once on the host: exactly the tables MechanismState tabulates (mechanism_state.jl:85-118) -----------
mutable struct FlatModelHandle
    handle::Ptr{Cvoid}
    modcount::Int
    nq::Int; nv::Int; nc::Int; nb::Int
    bodyindex::Dict{RigidBody, Int32}   # body -> index in the flat model (-1 = root body)
    bodyids::Dict{BodyID, Int32}
    loopjointids::Vector{JointID}       # the non-tree joints in the order of rbd_flat_model_t.loops (= the order of rbd_workspace_set_loop_gains)
end

const WAIT_HOOK = Ref(false)
const HEADER_VERSION = 700    # RBD_HIP_H_VERSION of the include/rbd_hip.h these structs mirror (rbd_flat_model_t grew its contact fields at 200; 400: rbd_workspace_set_loop_gains; 500: rbd_mass_matrix_solve_packed, rbd_gatherv; 600: rbd_jit_check_walk_object; 700: the derivative entry points)

function FlatModelHandle(mechanism::Mechanism)
    ccall((:rbd_version, librbd_hip[]), Cint, ()) == HEADER_VERSION ||
        error("librbd_hip.so reports another header version than this shim was written for ($HEADER_VERSION): struct layouts may differ")
    if !WAIT_HOOK[]  # once: a kernel compilation still running in the background is waited for before the process tears the compiler down
        atexit(() -> ccall((:rbd_jit_wait_idle, librbd_hip[]), Cvoid, ()))
        WAIT_HOOK[] = true
    end
    tj = collect(tree_joints(mechanism))
    nb = length(tj)
    bodyindex = Dict(successor(j, mechanism) => Int32(i - 1) for (i, j) in enumerate(tj))
    bodyindex[root_body(mechanism)] = Int32(-1)
    parent = Int32[bodyindex[predecessor(j, mechanism)] for j in tj]
    jtype = Int32[jointtag(joint_type(j)) for j in tj]
    qoff = Int32[0; cumsum(num_positions.(tj))[1:end-1]]
    voff = Int32[0; cumsum(num_velocities.(tj))[1:end-1]]
    axis = reduce(vcat, [collect(jointaxis(joint_type(j))) for j in tj]; init = Float64[])
    axis2 = reduce(vcat, [collect(jointaxis2(joint_type(j))) for j in tj]; init = Float64[])
    prot = reduce(vcat, [rowmajor(rotation(joint_to_predecessor(j))) for j in tj]; init = Float64[])
    ptrans = reduce(vcat, [Float64.(translation(joint_to_predecessor(j))) for j in tj]; init = Float64[])
    inertias = [spatial_inertia(successor(j, mechanism)) for j in tj]      # expressed in frame_after(joint) after canonicalization
    moment = reduce(vcat, [rowmajor(I.moment) for I in inertias]; init = Float64[])
    cross = reduce(vcat, [Float64.(I.cross_part) for I in inertias]; init = Float64[])
    mass = Float64[I.mass for I in inertias]
    loops = RbdLoopJoint[]
    for j in non_tree_joints(mechanism)
        jt = joint_type(j)
        # rotation_from_z_aligned: revolute.jl:12-17, prismatic.jl, sin_cos_revolute.jl:13 (all three carry the field; the C side builds
        # the constraint wrench basis of a loop joint from its columns)
        Rz = jt isa Union{Revolute, Prismatic, SinCosRevolute} ? rowmajor(jt.rotation_from_z_aligned) :
             jt isa Planar ? rowmajor(hcat(jt.x_axis, jt.y_axis, jt.rot_axis)) :      # columns (x, y, x × y): include/rbd_hip.h
             rowmajor(Matrix(1.0I, 3, 3))
        push!(loops, RbdLoopJoint(bodyindex[predecessor(j, mechanism)], bodyindex[successor(j, mechanism)], jointtag(jt), 0,
            jointaxis(jt), Tuple(rowmajor(rotation(joint_to_predecessor(j)))), Tuple(Float64.(translation(joint_to_predecessor(j)))),
            Tuple(rowmajor(rotation(joint_to_successor(j)))), Tuple(Float64.(translation(joint_to_successor(j)))),
            Tuple(Rz), (100.0, 20.0, 100.0, 20.0)))     # default_constraint_stabilization_gains (mechanism_algorithms.jl:610-612)
    end
    # soft contact: points in the order of the additional state (for body in bodies(m), for point: mechanism_state.jl:143), half-spaces
    cps = RbdContactPoint[]
    for body in bodies(mechanism), point in RigidBodyDynamics.contact_points(body)
        model = RigidBodyDynamics.Contact.contact_model(point)
        loc = RigidBodyDynamics.Contact.location(point).v
        push!(cps, RbdContactPoint(bodyindex[body], 0, (loc[1], loc[2], loc[3]), model.normal.k, model.normal.λ, model.normal.n,
            model.friction.μ, model.friction.k, model.friction.b))
    end
    hss = [RbdHalfSpace(Tuple(Float64.(h.point.v)), Tuple(Float64.(h.outward_normal.v))) for h in mechanism.environment.halfspaces]
    g = mechanism.gravitational_acceleration.v
    handle = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve parent jtype qoff voff axis axis2 prot ptrans moment cross mass loops cps hss begin
        desc = Ref(RbdFlatModel(nb, sum(num_positions, tj; init = 0), sum(num_velocities, tj; init = 0), length(loops),
            pointer(parent), pointer(jtype), pointer(qoff), pointer(voff), pointer(axis), pointer(axis2), pointer(prot), pointer(ptrans),
            pointer(moment), pointer(cross), pointer(mass), (g[1], g[2], g[3]), isempty(loops) ? C_NULL : pointer(loops),
            length(cps), length(hss), isempty(cps) ? C_NULL : pointer(cps), isempty(hss) ? C_NULL : pointer(hss)))
        check(ccall((:rbd_model_create, librbd_hip[]), Cint, (Ref{RbdFlatModel}, Ref{Ptr{Cvoid}}), desc, handle), "rbd_model_create")
    end
    m = FlatModelHandle(handle[], modcount(mechanism), num_positions(mechanism), num_velocities(mechanism),
        sum(num_constraints, non_tree_joints(mechanism); init = 0), nb, Dict{RigidBody, Int32}(bodyindex),
        Dict{BodyID, Int32}(BodyID(b) => i for (b, i) in bodyindex), JointID[JointID(j) for j in non_tree_joints(mechanism)])
    finalizer(x -> ccall((:rbd_model_destroy, librbd_hip[]), Cint, (Ptr{Cvoid},), x.handle), m)
    m
end

# Run-time specialised kernels (csrc/rbd_jit.hip): `mass_matrix!` at large batches runs code compiled for this mechanism by hiprtc the first time a
# workspace needs it; `precompile_kernels` pays for the compilation up front (no device needed, the code object is cached on disk).
function precompile_kernels(mechanism::Mechanism; T::Type = Float64)
    model = FlatModelHandle(mechanism)
    log = Vector{UInt8}(undef, 1 << 16)
    status = ccall((:rbd_jit_precompile, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{UInt8}, Int64), model.handle, T === Float64 ? 0 : 1, log, length(log))
    status == 3 && return false    # RBD_ERR_UNSUPPORTED: outside the specialised kernels' scope, or no hiprtc — the generic kernels run
    status == 0 || error("rbd_jit_precompile: " * unsafe_string(pointer(log)))
    true
end

# ---- batched state / result: same field names as the reference types -------------------------------------------
mutable struct BatchedMechanismState{T, A <: Buffer{T}}
    mechanism::Mechanism
    model::FlatModelHandle
    ws::Ptr{Cvoid}
    memory::Int32     # MEM_DEVICE: q, v (and every buffer handed to a call) are device pointers — the default; MEM_HOST: plain Matrix
    q::A              # nq × B
    v::A              # nv × B
    s::A              # num_additional_states × B: the soft-contact friction states (mechanism_state.jl:64, :139-152)
end

"""`storage = :device` (default): q, v are `DeviceMatrix` — resident in HBM, calls are asynchronous on the workspace's stream;
`storage = :host`: plain `Matrix` buffers, staged through PCIe inside every call (convenient, ~5× slower than the kernel)."""
function BatchedMechanismState(mechanism::Mechanism, B::Integer; T::Type = Float64, device::Integer = 0, storage::Symbol = :device)
    model = FlatModelHandle(mechanism)
    ws = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rbd_workspace_create, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
        model.handle, B, device, T === Float64 ? 0 : 1, C_NULL, ws), "rbd_workspace_create")
    q, v = newbuffer(Val(storage), T, model.nq, B), newbuffer(Val(storage), T, model.nv, B)
    s = BatchedMechanismState{T, typeof(q)}(mechanism, model, ws[], storage === :device ? MEM_DEVICE : MEM_HOST, q, v,
        newbuffer(Val(storage), T, RigidBodyDynamics.num_additional_states(mechanism), B))
    finalizer(x -> ccall((:rbd_workspace_destroy, librbd_hip[]), Cint, (Ptr{Cvoid},), x.ws), s)
    s
end

"wait for the asynchronous calls issued on this state's workspace; PosDefException if a mass matrix was not positive definite"
synchronize(state::BatchedMechanismState) = check(ccall((:rbd_sync, librbd_hip[]), Cint, (Ptr{Cvoid},), state.ws), "rbd_sync")
finish(state::BatchedMechanismState) = state.memory == MEM_HOST ? synchronize(state) : nothing   # host buffers must be complete on return

# @modcountcheck (src/util.jl:61): re-flatten when the mechanism was modified
function checkmodcount(state::BatchedMechanismState)
    modcount(state.mechanism) == state.model.modcount || throw(RigidBodyDynamics.ModificationCountMismatch("state out of date with mechanism"))
end

struct BatchedDynamicsResult{T, A <: Buffer{T}}
    massmatrix::A               # (nv·nv) × B: per state an nv × nv column-major matrix, lower triangle valid (Symmetric(…, :L))
    dynamicsbias::A             # nv × B
    q̇::A; v̇::A; λ::A
    constraintjacobian::A; constraintbias::A
    accelerations::A            # (6·n_bodies) × B — src/dynamics_result.jl:26-29, root frame, (angular; linear) per body
    jointwrenches::A
    totalwrenches::A
    ṡ::A                        # num_additional_states × B (dynamics_result.jl:20)
    contactwrenches::A          # (6·n_bodies) × B (dynamics_result.jl:25)
end
function BatchedDynamicsResult(mechanism::Mechanism, B::Integer; T::Type = Float64, storage::Symbol = :device)
    nq, nv, nb = num_positions(mechanism), num_velocities(mechanism), length(collect(tree_joints(mechanism)))
    nc = sum(num_constraints, non_tree_joints(mechanism); init = 0)
    z(n) = newbuffer(Val(storage), T, n, B)
    r = (z(nv * nv), z(nv), z(nq), z(nv), z(nc), z(nc * nv), z(nc), z(6nb), z(6nb), z(6nb), z(RigidBodyDynamics.num_additional_states(mechanism)), z(6nb))
    BatchedDynamicsResult{T, typeof(r[1])}(r...)
end

opts(state; algorithm = 0, stabilization = 1) = Ref(RbdOpts(LAYOUT_AOS, state.memory, algorithm, stabilization))

# `stabilization_gains` (src/mechanism_algorithms.jl:614-632, :848; src/simulate.jl:37) -> the flag of rbd_opts_t + rbd_workspace_set_loop_gains:
#   nothing                                   no Baumgarte stabilization;
#   :default                                  the model's gains = default_constraint_stabilization_gains (100, 20, 100, 20);
#   AbstractDict{JointID, <:SE3PDGains}       per loop joint (a ConstDict{JointID} is one — its getindex ignores the key); a missing joint throws the
#                                             dictionary's own KeyError, as stabilization_gains[nontreejointid] (:655) does in the reference.
# Scalar gains only: the kernels apply k and d as scalars (every use in the reference and its tests); matrix gains throw an ArgumentError
# instead of being silently replaced.  The call is cheap when the gains are the ones already in force.
scalargain(x::Number) = Float64(x)
scalargain(x) = throw(ArgumentError("stabilization_gains: only scalar PD gains are supported by librbd_hip, got $(typeof(x))"))
function stabilization(state, ::Nothing)
    Int32(0)
end
function stabilization(state, gains::Symbol)
    gains === :default || throw(ArgumentError("stabilization_gains: $gains"))
    isempty(state.model.loopjointids) || check(ccall((:rbd_workspace_set_loop_gains, librbd_hip[]), Cint, (Ptr{Cvoid}, Ptr{Float64}), state.ws, C_NULL),
        "rbd_workspace_set_loop_gains")
    Int32(1)
end
function stabilization(state, gains::AbstractDict{JointID, <:SE3PDGains})
    ids = state.model.loopjointids
    isempty(ids) && return Int32(1)
    g = Float64[]
    for id in ids
        gj = gains[id]
        append!(g, (scalargain(gj.angular.k), scalargain(gj.angular.d), scalargain(gj.linear.k), scalargain(gj.linear.d)))
    end
    check(ccall((:rbd_workspace_set_loop_gains, librbd_hip[]), Cint, (Ptr{Cvoid}, Ptr{Float64}), state.ws, g), "rbd_workspace_set_loop_gains")
    Int32(1)
end
stabilization(state, gains) = throw(ArgumentError("stabilization_gains must be nothing or an AbstractDict{JointID, <:SE3PDGains}, got $(typeof(gains))"))
nullable(x) = pointer(x)
nullable(::Nothing) = C_NULL
batchsize(state) = size(state.q, 2)

# externalwrenches: `nothing` (NullDict), a dense (6·n_bodies) × B buffer of root-frame wrenches (torque; force) per body, or the
# reference's own `AbstractDict{BodyID, <:Wrench}` (root frame; applied to every state of the batch) which is densified here
function densewrenches(state::BatchedMechanismState{T}, w::AbstractDict{BodyID, <:Wrench}) where {T}
    nb, B = state.model.nb, batchsize(state)
    h = zeros(T, 6nb, B)
    for (id, wrench) in w
        i = state.model.bodyids[id]
        i < 0 && continue
        h[6i+1:6i+3, :] .= angular(wrench); h[6i+4:6i+6, :] .= linear(wrench)
    end
    state.memory == MEM_HOST ? h : copyto!(DeviceMatrix{T}(6nb, B), h)
end
densewrenches(state, w) = w

# ---- the four generics -----------------------------------------------------------------------------------------
"""`dynamics!(result, state, torques, externalwrenches; stabilization_gains)` — src/mechanism_algorithms.jl:845-864.
`torques`: nv × B or `nothing` (zeros).  Fills result.v̇, q̇ (λ, M, c, K, k on the reference's CRBA route) and, like the reference, the
per-body fields: totalwrenches, and the bias accelerations / joint wrenches of its dynamics_bias! call."""
function dynamics!(result::BatchedDynamicsResult{T}, state::BatchedMechanismState{T}, torques = nothing, externalwrenches = nothing;
        stabilization_gains = :default, algorithm::Symbol = :aba, bodies::Bool = false) where {T}
    checkmodcount(state)
    B = batchsize(state)
    torques === nothing || size(torques) == (state.model.nv, B) || throw(DimensionMismatch("torques"))
    wext = densewrenches(state, externalwrenches)
    o = opts(state; algorithm = algorithm === :aba ? 0 : 1, stabilization = stabilization(state, stabilization_gains))
    λptr = state.model.nc > 0 ? pointer(result.λ) : C_NULL
    if size(state.s, 1) > 0
        # contact points: contact_dynamics! (:680-723), totalwrenches = externalwrenches + contactwrenches (:851-856), then forward dynamics.
        # state.s is reset where a point is not in contact, exactly as the reference resets the contact state in place.  Device buffers only.
        check(ccall((:rbd_dynamics_contact, librbd_hip[]), Cint,
            (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
            state.ws, B, state.q, state.v, state.s, nullable(torques), nullable(wext), result.v̇, result.q̇, result.ṡ, result.contactwrenches,
            result.totalwrenches, o), "rbd_dynamics_contact")
        finish(state)
        return nothing
    end
    # the reference's route on a tree mechanism with device buffers: M and c are written into the result's own buffers (no copy out of the workspace)
    bind = algorithm !== :aba && state.model.nc == 0 && state.memory == MEM_DEVICE
    bind && check(ccall((:rbd_workspace_bind_result, librbd_hip[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), state.ws, result.massmatrix.ptr, result.dynamicsbias.ptr),
        "rbd_workspace_bind_result")
    try
        check(ccall((:rbd_dynamics, librbd_hip[]), Cint,
            (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
            state.ws, B, state.q, state.v, nullable(torques), nullable(wext), result.v̇, result.q̇, λptr, o), "rbd_dynamics")
    finally     # never leave the result's buffers bound to the workspace: a later call would write into them, freed or not
        bind && ccall((:rbd_workspace_bind_result, librbd_hip[]), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), state.ws, C_NULL, C_NULL)
    end
    if !bind && (algorithm !== :aba || state.model.nc > 0)
        check(ccall((:rbd_dynamics_result, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
            state.ws, B, result.massmatrix, result.dynamicsbias, state.model.nc > 0 ? pointer(result.constraintjacobian) : C_NULL,
            state.model.nc > 0 ? pointer(result.constraintbias) : C_NULL, o), "rbd_dynamics_result")
    end
    if bodies   # result.accelerations / jointwrenches as dynamics!'s own dynamics_bias! call leaves them (:851-856)
        check(ccall((:rbd_dynamics_bias_bodies, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
            state.ws, B, state.q, state.v, nullable(wext), result.dynamicsbias, result.jointwrenches, result.accelerations, opts(state)), "rbd_dynamics_bias_bodies")
    end
    finish(state)
    nothing
end

"""`dynamics!(ẋ, result, state, x, torques, externalwrenches; stabilization_gains)` — the ODE form, :880-889: x = [q; v] per column,
ẋ = [q̇; v̇] (no additional state: there are no contact points)."""
function dynamics!(ẋ::Matrix{T}, result::BatchedDynamicsResult{T}, state::BatchedMechanismState{T}, x::Matrix{T}, torques = nothing,
        externalwrenches = nothing; stabilization_gains = :default) where {T}
    nq, nv = state.model.nq, state.model.nv
    size(x) == (nq + nv, batchsize(state)) || throw(DimensionMismatch("x"))
    copyto!(state.q, x[1:nq, :]); copyto!(state.v, x[nq+1:end, :])          # copyto!(state, x), mechanism_state.jl:465-491
    dynamics!(result, state, torques, externalwrenches; stabilization_gains = stabilization_gains)
    synchronize(state)
    ẋ[1:nq, :] .= result.q̇ isa Matrix ? result.q̇ : Array(result.q̇)          # copyto!(ẋ, result), dynamics_result.jl:89
    ẋ[nq+1:end, :] .= result.v̇ isa Matrix ? result.v̇ : Array(result.v̇)
    ẋ
end

"""`inverse_dynamics!(torquesout, jointwrenchesout, accelerations, state, v̇, externalwrenches)` — :542-553, the reference's own
arity: `jointwrenchesout` / `accelerations` are (6·n_bodies) × B buffers (root frame) or `nothing`."""
function inverse_dynamics!(torquesout::Buffer{T}, jointwrenchesout, accelerations, state::BatchedMechanismState{T}, v̇::Buffer{T},
        externalwrenches = nothing) where {T}
    checkmodcount(state)
    B = batchsize(state)
    size(torquesout) == (state.model.nv, B) || error("length of torque vector is wrong")
    check(ccall((:rbd_inverse_dynamics_bodies, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, v̇, nullable(densewrenches(state, externalwrenches)), torquesout, nullable(jointwrenchesout),
        nullable(accelerations), opts(state)), "rbd_inverse_dynamics_bodies")
    finish(state)
    torquesout
end
# the short form many callers use: inverse_dynamics!(τ, state, v̇, wext)
inverse_dynamics!(torquesout::Buffer{T}, state::BatchedMechanismState{T}, v̇::Buffer{T}, externalwrenches = nothing) where {T} =
    inverse_dynamics!(torquesout, nothing, nothing, state, v̇, externalwrenches)

"""`dynamics_bias!(result, state)` — :496-498 (external wrenches = result.totalwrenches, as in the reference)."""
function dynamics_bias!(result::BatchedDynamicsResult{T}, state::BatchedMechanismState{T}, externalwrenches = nothing) where {T}
    checkmodcount(state)
    check(ccall((:rbd_dynamics_bias_bodies, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, batchsize(state), state.q, state.v, nullable(densewrenches(state, externalwrenches)), result.dynamicsbias, result.jointwrenches,
        result.accelerations, opts(state)), "rbd_dynamics_bias_bodies")
    finish(state)
    result.dynamicsbias
end

"""`mass_matrix!(M, state)` / `mass_matrix!(result, state)` — :248-274; lower triangles written (uplo == 'L')."""
function mass_matrix!(M::Buffer{T}, state::BatchedMechanismState{T}) where {T}
    checkmodcount(state)
    nv, B = state.model.nv, batchsize(state)
    size(M) == (nv * nv, B) || throw(DimensionMismatch("mass matrix has wrong size"))
    check(ccall((:rbd_mass_matrix, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, M, opts(state)), "rbd_mass_matrix")
    finish(state)
    M
end
mass_matrix!(result::BatchedDynamicsResult, state::BatchedMechanismState) = mass_matrix!(result.massmatrix, state)

# ---- forward-mode derivatives (header 700): what `ForwardDiff.jacobian` / `Dual` numbers through the reference give (test/test_mechanism_algorithms.jl:600-652),
# in the raw coordinates q.  Tangent buffers are (n·ntan) × B (direction d of a state at rows d·n+1 … d·n+n); Jacobians (nv·ncols) × B, column-major per
# state (`reshape(J[:, b], nv, :)`); every tangent input and every output may be `nothing`.

"""`inverse_dynamics_jvp!(dτ, state, v̇, ntan; dq, dv, dv̇, externalwrenches, dexternalwrenches, torquesout)` — `inverse_dynamics!` pushed forward along
`ntan` directions per state (`rbd_inverse_dynamics_jvp`)."""
function inverse_dynamics_jvp!(dτ, state::BatchedMechanismState{T}, v̇::Buffer{T}, ntan::Integer; dq = nothing, dv = nothing, dv̇ = nothing,
        externalwrenches = nothing, dexternalwrenches = nothing, torquesout = nothing) where {T}
    checkmodcount(state)
    nq, nv, B = state.model.nq, state.model.nv, batchsize(state)
    ntan > 0 || throw(ArgumentError("ntan must be positive"))
    for (x, n) in ((dτ, nv), (dq, nq), (dv, nv), (dv̇, nv))
        x === nothing || size(x) == (n * ntan, B) || throw(DimensionMismatch("tangent buffer has wrong size"))
    end
    check(ccall((:rbd_inverse_dynamics_jvp, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, ntan, state.q, state.v, v̇, nullable(densewrenches(state, externalwrenches)), nullable(dq), nullable(dv), nullable(dv̇),
        nullable(dexternalwrenches), nullable(torquesout), nullable(dτ), opts(state)), "rbd_inverse_dynamics_jvp")
    finish(state)
    dτ
end

"""`dynamics_jvp!(dv̇, state, ntan; torques, dq, dv, dτ, externalwrenches, dexternalwrenches, v̇out)` — `dynamics!` pushed forward along `ntan` directions
per state: M dv̇ = dτ − ∂ID·(dq, dv, 0, dfext) at the v̇ of the same call (`rbd_dynamics_jvp`)."""
function dynamics_jvp!(dv̇, state::BatchedMechanismState{T}, ntan::Integer; torques = nothing, dq = nothing, dv = nothing, dτ = nothing,
        externalwrenches = nothing, dexternalwrenches = nothing, v̇out = nothing) where {T}
    checkmodcount(state)
    nq, nv, B = state.model.nq, state.model.nv, batchsize(state)
    ntan > 0 || throw(ArgumentError("ntan must be positive"))
    for (x, n) in ((dv̇, nv), (dq, nq), (dv, nv), (dτ, nv))
        x === nothing || size(x) == (n * ntan, B) || throw(DimensionMismatch("tangent buffer has wrong size"))
    end
    check(ccall((:rbd_dynamics_jvp, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, ntan, state.q, state.v, nullable(torques), nullable(densewrenches(state, externalwrenches)), nullable(dq), nullable(dv), nullable(dτ),
        nullable(dexternalwrenches), nullable(v̇out), nullable(dv̇), opts(state)), "rbd_dynamics_jvp")
    finish(state)
    dv̇
end

"""`inverse_dynamics_derivatives!(∂τ∂q, ∂τ∂v, M, state, v̇; externalwrenches, torquesout)` — the Jacobians of `inverse_dynamics!` (fext fixed): (nv·nq) × B,
(nv·nv) × B, and M = ∂τ/∂v̇ as the full square (`rbd_inverse_dynamics_derivatives`)."""
function inverse_dynamics_derivatives!(dτdq, dτdv, M, state::BatchedMechanismState{T}, v̇::Buffer{T}; externalwrenches = nothing, torquesout = nothing) where {T}
    checkmodcount(state)
    nq, nv, B = state.model.nq, state.model.nv, batchsize(state)
    for (x, n) in ((dτdq, nv * nq), (dτdv, nv * nv), (M, nv * nv))
        x === nothing || size(x) == (n, B) || throw(DimensionMismatch("Jacobian buffer has wrong size"))
    end
    check(ccall((:rbd_inverse_dynamics_derivatives, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, v̇, nullable(densewrenches(state, externalwrenches)), nullable(torquesout), nullable(dτdq), nullable(dτdv), nullable(M),
        opts(state)), "rbd_inverse_dynamics_derivatives")
    finish(state)
    dτdq, dτdv, M
end

"""`dynamics_derivatives!(∂v̇∂q, ∂v̇∂v, ∂v̇∂τ, state; torques, externalwrenches, v̇out)` — the Jacobians of `dynamics!` (fext fixed); ∂v̇/∂τ = M⁻¹
(`rbd_dynamics_derivatives`)."""
function dynamics_derivatives!(dv̇dq, dv̇dv, dv̇dτ, state::BatchedMechanismState{T}; torques = nothing, externalwrenches = nothing, v̇out = nothing) where {T}
    checkmodcount(state)
    nq, nv, B = state.model.nq, state.model.nv, batchsize(state)
    for (x, n) in ((dv̇dq, nv * nq), (dv̇dv, nv * nv), (dv̇dτ, nv * nv))
        x === nothing || size(x) == (n, B) || throw(DimensionMismatch("Jacobian buffer has wrong size"))
    end
    check(ccall((:rbd_dynamics_derivatives, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, nullable(torques), nullable(densewrenches(state, externalwrenches)), nullable(v̇out), nullable(dv̇dq), nullable(dv̇dv),
        nullable(dv̇dτ), opts(state)), "rbd_dynamics_derivatives")
    finish(state)
    dv̇dq, dv̇dv, dv̇dτ
end

"""`simulate_jvp!(dq, dv, state, ntan, Δt; nsteps = 1, torques, dτ, externalwrenches, dexternalwrenches)` — `nsteps` Munthe-Kaas RK4 steps of `simulate`
with `ntan` directions per state carried along: `state.q`, `state.v`, `dq` ((nq·ntan) × B) and `dv` ((nv·ntan) × B) advanced in place; `dτ` and the wrench
directions held over every stage, as the torques are (`rbd_simulate_jvp`)."""
function simulate_jvp!(dq::Buffer{T}, dv::Buffer{T}, state::BatchedMechanismState{T}, ntan::Integer, Δt::Real; nsteps::Integer = 1, torques = nothing,
        dτ = nothing, externalwrenches = nothing, dexternalwrenches = nothing) where {T}
    checkmodcount(state)
    nq, nv, B = state.model.nq, state.model.nv, batchsize(state)
    ntan > 0 || throw(ArgumentError("ntan must be positive"))
    Δt > 0 || throw(ArgumentError("Δt must be positive"))
    nsteps >= 0 || throw(ArgumentError("nsteps must be non-negative"))
    for (x, n) in ((dq, nq), (dv, nv), (dτ, nv))
        x === nothing || size(x) == (n * ntan, B) || throw(DimensionMismatch("tangent buffer has wrong size"))
    end
    check(ccall((:rbd_simulate_jvp, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cdouble, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, ntan, state.q, state.v, nullable(torques), nullable(densewrenches(state, externalwrenches)), Float64(Δt), nsteps, dq, dv,
        nullable(dτ), nullable(dexternalwrenches), opts(state)), "rbd_simulate_jvp")
    finish(state)
    dq, dv
end

"""`simulate_step_derivatives!(∂x∂x, ∂x∂τ, state, Δt; torques, externalwrenches)` — one step of `simulate` (`state` advanced in place) and its Jacobians
with x = (q; v), nx = nq + nv: (nx·nx) × B and (nx·nv) × B, column-major per state, either one `nothing`; the wrenches held fixed
(`rbd_simulate_step_derivatives`)."""
function simulate_step_derivatives!(dxdx, dxdτ, state::BatchedMechanismState{T}, Δt::Real; torques = nothing, externalwrenches = nothing) where {T}
    checkmodcount(state)
    nq, nv, B = state.model.nq, state.model.nv, batchsize(state)
    nx = nq + nv
    Δt > 0 || throw(ArgumentError("Δt must be positive"))
    for (x, n) in ((dxdx, nx * nx), (dxdτ, nx * nv))
        x === nothing || size(x) == (n, B) || throw(DimensionMismatch("Jacobian buffer has wrong size"))
    end
    check(ccall((:rbd_simulate_step_derivatives, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cdouble, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, nullable(torques), nullable(densewrenches(state, externalwrenches)), Float64(Δt), nullable(dxdx), nullable(dxdτ),
        opts(state)), "rbd_simulate_step_derivatives")
    finish(state)
    dxdx, dxdτ
end

# ---- reverse mode (700 additions): vector-Jacobian products, one cotangent per state (nv × B), raw coordinates q as above.  Every output may be
# `nothing` and is overwritten; q̄ is nq × B, v̄ / v̇̄ / τ̄ nv × B, f̄ext (6·n_bodies) × B.  (A ChainRules `rrule` would wrap these.)

"""`inverse_dynamics_vjp!(q̄, v̄, v̇̄, state, v̇, τ̄; externalwrenches, f̄ext, torquesout)` — `inverse_dynamics!` pulled back: q̄ = (∂τ/∂q)ᵀτ̄,
v̄ = (∂τ/∂v)ᵀτ̄, v̇̄ = M τ̄, f̄ext = (∂τ/∂fext)ᵀτ̄ (`rbd_inverse_dynamics_vjp`)."""
function inverse_dynamics_vjp!(q̄, v̄, v̇̄, state::BatchedMechanismState{T}, v̇::Buffer{T}, τ̄::Buffer{T}; externalwrenches = nothing, f̄ext = nothing,
        torquesout = nothing) where {T}
    checkmodcount(state)
    nq, nv, B = state.model.nq, state.model.nv, batchsize(state)
    for (x, n) in ((q̄, nq), (v̄, nv), (v̇̄, nv), (τ̄, nv), (torquesout, nv))
        x === nothing || size(x) == (n, B) || throw(DimensionMismatch("cotangent buffer has wrong size"))
    end
    check(ccall((:rbd_inverse_dynamics_vjp, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, v̇, nullable(densewrenches(state, externalwrenches)), τ̄, nullable(torquesout), nullable(q̄), nullable(v̄),
        nullable(v̇̄), nullable(f̄ext), opts(state)), "rbd_inverse_dynamics_vjp")
    finish(state)
    q̄, v̄, v̇̄
end

"""`dynamics_vjp!(q̄, v̄, τ̄, state, v̇̄; torques, externalwrenches, f̄ext, v̇out)` — `dynamics!` pulled back at the v̇ of the same call: λ = M⁻¹v̇̄, τ̄ = λ,
(q̄, v̄, f̄ext) = −(∂ID/∂(q, v, fext))ᵀλ (`rbd_dynamics_vjp`)."""
function dynamics_vjp!(q̄, v̄, τ̄, state::BatchedMechanismState{T}, v̇̄::Buffer{T}; torques = nothing, externalwrenches = nothing, f̄ext = nothing,
        v̇out = nothing) where {T}
    checkmodcount(state)
    nq, nv, B = state.model.nq, state.model.nv, batchsize(state)
    for (x, n) in ((q̄, nq), (v̄, nv), (τ̄, nv), (v̇̄, nv), (v̇out, nv))
        x === nothing || size(x) == (n, B) || throw(DimensionMismatch("cotangent buffer has wrong size"))
    end
    check(ccall((:rbd_dynamics_vjp, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, nullable(torques), nullable(densewrenches(state, externalwrenches)), v̇̄, nullable(v̇out), nullable(q̄), nullable(v̄),
        nullable(τ̄), nullable(f̄ext), opts(state)), "rbd_dynamics_vjp")
    finish(state)
    q̄, v̄, τ̄
end

"""`simulate_vjp!(q̄, v̄, state, Δt; nsteps = 1, torques, externalwrenches, τ̄, f̄ext)` — `nsteps` Munthe-Kaas RK4 steps of `simulate` pulled back
(`state` advanced in place, as `simulate_jvp!`): q̄ (nq × B), v̄ (nv × B) hold the cotangent of the final state on entry and that of the initial state on
return; τ̄, f̄ext (each may be `nothing`) are overwritten with the gradient in the held torques / wrenches over every stage (`rbd_simulate_vjp`)."""
function simulate_vjp!(q̄::Buffer{T}, v̄::Buffer{T}, state::BatchedMechanismState{T}, Δt::Real; nsteps::Integer = 1, torques = nothing,
        externalwrenches = nothing, τ̄ = nothing, f̄ext = nothing) where {T}
    checkmodcount(state)
    nq, nv, B = state.model.nq, state.model.nv, batchsize(state)
    Δt > 0 || throw(ArgumentError("Δt must be positive"))
    nsteps >= 0 || throw(ArgumentError("nsteps must be non-negative"))
    for (x, n) in ((q̄, nq), (v̄, nv), (τ̄, nv))
        x === nothing || size(x) == (n, B) || throw(DimensionMismatch("cotangent buffer has wrong size"))
    end
    check(ccall((:rbd_simulate_vjp, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cdouble, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, nullable(torques), nullable(densewrenches(state, externalwrenches)), Float64(Δt), Int32(nsteps), q̄, v̄,
        nullable(τ̄), nullable(f̄ext), opts(state)), "rbd_simulate_vjp")
    finish(state)
    q̄, v̄, τ̄
end

"""`mass_matrix_solve_packed!(x, Mpacked, state, rhs)` — `mass_matrix!` + the potrf!/potrs! of `dynamics_solve!` (:764, :819) with M as LAPACK's packed lower
triangle: `Mpacked` is nv(nv+1)/2 × B, element (i, j), i ≥ j (0-based), of a state at i + j(2nv − j − 1)/2 — what `Symmetric(M, :L)` defines, half the bytes of
the square (`rbd_mass_matrix_solve_packed`)."""
function mass_matrix_solve_packed!(x::Buffer{T}, Mpacked::Buffer{T}, state::BatchedMechanismState{T}, rhs::Buffer{T}) where {T}
    checkmodcount(state)
    nv, B = state.model.nv, batchsize(state)
    size(Mpacked) == (nv * (nv + 1) ÷ 2, B) && size(x) == (nv, B) && size(rhs) == (nv, B) || throw(DimensionMismatch("packed mass matrix / x / rhs have wrong sizes"))
    check(ccall((:rbd_mass_matrix_solve_packed, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, rhs, x, Mpacked, opts(state; algorithm = 1)), "rbd_mass_matrix_solve_packed")   # 1 = RBD_ALGO_CRBA_CHOLESKY
    finish(state)
    x
end

# number of steps of integrate(), src/ode_integrators.jl:311-314: `while t < final_time` in the state's scalar type
function stepcount(::Type{T}, final_time, Δt) where {T}
    nsteps, t = 0, zero(T)
    while t < final_time
        t += Δt; nsteps += 1
    end
    nsteps
end
hostcopy(x::Matrix) = copy(x)
hostcopy(x::DeviceMatrix) = Array(x)

"""`simulate(state0, final_time; Δt, stabilization_gains)` — src/simulate.jl:36-55 for the whole batch: Munthe-Kaas RK4 on the
device (`rbd_simulate`), constant `torques` (the default control is `zero_torque!`), optional `externalwrenches`; `state.q`, `state.v` are advanced
in place.  Returns `(ts, qs, vs)` like the reference; `store = true` (the reference always stores, `ExpandingStorage`) keeps a host copy of q and v
(nq × B, nv × B) per step in `qs`, `vs` — one launch sequence per step; `store = false` (default here: B trajectories are B times the memory) runs
all the steps without returning to the host and returns `qs = vs = nothing`."""
function simulate(state::BatchedMechanismState{T}, final_time; Δt = 1e-4, torques = nothing, externalwrenches = nothing, stabilization_gains = :default,
        store::Bool = false) where {T}
    checkmodcount(state)
    nsteps = stepcount(T, final_time, Δt)
    B = batchsize(state)
    wext = densewrenches(state, externalwrenches)
    ts = range(zero(T), step = T(Δt), length = nsteps + 1)
    qs, vs = store ? ([hostcopy(state.q)], [hostcopy(state.v)]) : (nothing, nothing)
    for chunk in (store ? fill(1, nsteps) : (nsteps,))
        if size(state.s, 1) > 0     # contact points: the additional state is integrated beside (q, v) with the same tableau
            check(ccall((:rbd_simulate_contact, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cdouble, Int32, Ref{RbdOpts}),
                state.ws, B, state.q, state.v, state.s, nullable(torques), nullable(wext), Float64(Δt), chunk, opts(state)), "rbd_simulate_contact")
        else
            check(ccall((:rbd_simulate, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cdouble, Int32, Ref{RbdOpts}),
                state.ws, B, state.q, state.v, nullable(torques), nullable(wext), Float64(Δt), chunk,
                opts(state; stabilization = stabilization(state, stabilization_gains))), "rbd_simulate")
        end
        if store
            synchronize(state); push!(qs, hostcopy(state.q)); push!(vs, hostcopy(state.v))
        end
    end
    finish(state)
    ts, qs, vs
end

"""`simulate(state0, final_time, control!; Δt, stabilization_gains)` — src/simulate.jl:36-55 with ANY controller: `control!(torques, t, state)` is
called before every Runge-Kutta stage's `dynamics!` exactly as the reference's closure does (:42-48), with `torques` the nv × B buffer of the batch
(a `DeviceMatrix`: fill it with `copyto!` or a kernel of your own; the state must be device-resident — `ArgumentError` otherwise), `t` the stage time and `state` holding the STAGE state.
The stage arithmetic of MuntheKaasIntegrator.step (src/ode_integrators.jl:233-299) runs on the device (`rbd_mk_stage`: stage 0 snapshots the base
point, stages 1..3 take the previous stage's v̇, stage 4 closes the step); only the controller runs on the host.  Returns `(ts, qs, vs)` (`store`
as above).  Controllers that can run on the device should use `TorqueTable` / `PDControl` below: no host round trip per stage."""
function simulate(state::BatchedMechanismState{T}, final_time, control!::Function; Δt = 1e-4, externalwrenches = nothing, stabilization_gains = :default,
        store::Bool = false) where {T}
    checkmodcount(state)
    size(state.s, 1) == 0 || throw(ArgumentError("control! with contact points: drive dynamics! per stage yourself"))
    # rbd_mk_stage advances q, v in place on the device (it answers RBD_ERR_INVALID_ARGUMENT to host memory): say so here, by name
    state.memory == MEM_DEVICE || throw(ArgumentError("simulate with a control! callback needs a device-resident state (storage = :device); " *
                                                      "a host-resident one can be stepped with dynamics!(ẋ, result, state, x) and an integrator of your own"))
    nsteps = stepcount(T, final_time, Δt)
    B, nv, nc = batchsize(state), state.model.nv, state.model.nc
    wext = densewrenches(state, externalwrenches)
    o = opts(state; stabilization = stabilization(state, stabilization_gains))
    storage = Val(:device)
    τ, v̇, λ = newbuffer(storage, T, nv, B), newbuffer(storage, T, nv, B), newbuffer(storage, T, max(nc, 1), B)
    ts = range(zero(T), step = T(Δt), length = nsteps + 1)
    qs, vs = store ? ([hostcopy(state.q)], [hostcopy(state.v)]) : (nothing, nothing)
    stagetimes = (zero(T), T(Δt) / 2, T(Δt) / 2, T(Δt))     # runge_kutta_4's c (src/ode_integrators.jl:48-55)
    for k in 1:nsteps
        for stage in 0:4
            check(ccall((:rbd_mk_stage, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Int32, Cdouble, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
                state.ws, B, stage, Float64(Δt), state.q, state.v, stage > 0 ? pointer(v̇) : Ptr{T}(C_NULL), o), "rbd_mk_stage")
            stage == 4 && break
            synchronize(state)      # the controller may read the stage state from the host
            control!(τ, ts[k] + stagetimes[stage + 1], state)
            check(ccall((:rbd_dynamics, librbd_hip[]), Cint,
                (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
                state.ws, B, state.q, state.v, τ, nullable(wext), v̇, C_NULL, nc > 0 ? pointer(λ) : Ptr{T}(C_NULL), o), "rbd_dynamics")
        end
        if store
            synchronize(state); push!(qs, hostcopy(state.q)); push!(vs, hostcopy(state.v))
        end
    end
    finish(state)
    ts, qs, vs
end

"""`simulate(state0, final_time, control; Δt)` with a controller that runs on the device (no host round trip per Runge-Kutta stage — the
reference calls `control!(τ, t, state)` before every stage's `dynamics!`, src/simulate.jl:42-48):
`TorqueTable(τ, per_stage)` — τ :: (nv·B) × entries, entry 4·step + stage (the stage times) or entry `step` (zero-order hold);
`PDControl(kp, kd, q_des, τff)` — τ = τff − kp (q − q_des) − kd v on Revolute / Prismatic joints, on the stage state (kp, kd :: nv × 1).
A mechanism with contact points takes both (`rbd_simulate_contact_controlled`): `state.s` is integrated beside (q, v) and reset at every stage state."""
struct TorqueTable{T}; torques::DeviceMatrix{T}; per_stage::Bool; end
struct PDControl{T}; kp::DeviceMatrix{T}; kd::DeviceMatrix{T}; q_des::Union{Nothing, DeviceMatrix{T}}; torques::Union{Nothing, DeviceMatrix{T}}; end
function simulate(state::BatchedMechanismState{T}, final_time, control::Union{TorqueTable{T}, PDControl{T}}; Δt = 1e-4, externalwrenches = nothing) where {T}
    checkmodcount(state)
    state.memory == MEM_DEVICE || throw(ArgumentError("device-side controllers need device-resident states (storage = :device)"))
    nsteps = stepcount(T, final_time, Δt)
    B, nq, nv = batchsize(state), state.model.nq, state.model.nv
    # the kernels index the controller's buffers without bounds: check them here (the C entry point sees only pointers)
    if control isa TorqueTable
        need = (control.per_stage ? 4 : 1) * nsteps
        size(control.torques, 1) == nv * B && size(control.torques, 2) >= need ||
            throw(DimensionMismatch("TorqueTable: need a (nv·B) × n table with n ≥ $need entries, got $(size(control.torques))"))
    else
        prod(size(control.kp)) == nv && prod(size(control.kd)) == nv || throw(DimensionMismatch("PDControl: kp, kd must hold nv = $nv gains"))
        control.q_des === nothing || size(control.q_des) == (nq, B) || throw(DimensionMismatch("PDControl: q_des must be nq × B"))
        control.torques === nothing || size(control.torques) == (nv, B) || throw(DimensionMismatch("PDControl: torques must be nv × B"))
    end
    wext = densewrenches(state, externalwrenches)
    vp(x) = x === nothing ? Ptr{Cvoid}(C_NULL) : Ptr{Cvoid}(pointer(x))
    ctl = control isa TorqueTable ? RbdControl(1, control.per_stage ? 1 : 0, vp(control.torques), C_NULL, C_NULL, C_NULL) :
                                    RbdControl(2, 0, vp(control.torques), vp(control.q_des), vp(control.kp), vp(control.kd))
    if size(state.s, 1) > 0     # contact points: the controller on the stage state contact_dynamics! and dynamics! see, s integrated beside (q, v)
        check(ccall((:rbd_simulate_contact_controlled, librbd_hip[]), Cint,
            (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdControl}, Ptr{T}, Cdouble, Int32, Ref{RbdOpts}),
            state.ws, B, state.q, state.v, state.s, ctl, nullable(wext), Float64(Δt), nsteps, opts(state)), "rbd_simulate_contact_controlled")
    else
        check(ccall((:rbd_simulate_controlled, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ref{RbdControl}, Ptr{T}, Cdouble, Int32, Ref{RbdOpts}),
            state.ws, B, state.q, state.v, ctl, nullable(wext), Float64(Δt), nsteps, opts(state)), "rbd_simulate_controlled")
    end
    finish(state)
    range(zero(T), step = T(Δt), length = nsteps + 1), nothing, nothing
end

# ---- kinematics by-products of the same forward-kinematics pass (root frame) -------------------------------------------------------
# momentum_matrix!(out, state) mechanism_algorithms.jl:313-327: out is (6·nv) × B, per state a 6 × nv column-major matrix
function momentum_matrix!(out::Buffer{T}, state::BatchedMechanismState{T}) where {T}
    checkmodcount(state)
    B = batchsize(state)
    size(out) == (6 * state.model.nv, B) || throw(DimensionMismatch())
    check(ccall((:rbd_kinematics, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, out, C_NULL, C_NULL, opts(state)), "rbd_kinematics")
    finish(state)
    out
end

# center_of_mass(state) :28-50 -> 3 × B;  kinetic_energy / gravitational_potential_energy mechanism_state.jl:886-903 -> B each
function kin(state::BatchedMechanismState{T}, n::Int, slot::Int) where {T}
    B = batchsize(state)
    out = newbuffer(Val(state.memory == MEM_HOST ? :host : :device), T, n, B)
    ptrs = (C_NULL, C_NULL, C_NULL)
    check(ccall((:rbd_kinematics, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, C_NULL, slot == 2 ? pointer(out) : Ptr{T}(C_NULL), slot == 3 ? pointer(out) : Ptr{T}(C_NULL), opts(state)), "rbd_kinematics")
    synchronize(state)
    out isa Matrix ? out : Array(out)
end
center_of_mass(state::BatchedMechanismState) = kin(state, 3, 2)
kinetic_energy(state::BatchedMechanismState) = kin(state, 2, 3)[1, :]
gravitational_potential_energy(state::BatchedMechanismState) = kin(state, 2, 3)[2, :]

# momentum(state), momentum_rate_bias(state) mechanism_state.jl:975-987 -> 6 × B each
function momenta(state::BatchedMechanismState{T}) where {T}
    B = batchsize(state)
    out = newbuffer(Val(state.memory == MEM_HOST ? :host : :device), T, 12, B)
    check(ccall((:rbd_momentum, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}), state.ws, B, state.q, state.v, out, opts(state)),
        "rbd_momentum")
    synchronize(state)
    out isa Matrix ? out : Array(out)
end
momentum(state::BatchedMechanismState) = momenta(state)[1:6, :]
momentum_rate_bias(state::BatchedMechanismState) = momenta(state)[7:12, :]

# geometric_jacobian!(out, state, path) :80-99 in the root frame; the path is given by its end bodies (path(mechanism, base, body))
function geometric_jacobian!(out::Buffer{T}, state::BatchedMechanismState{T}, base::RigidBody, body::RigidBody) where {T}
    checkmodcount(state)
    B = batchsize(state)
    size(out) == (6 * state.model.nv, B) || throw(DimensionMismatch())
    check(ccall((:rbd_geometric_jacobian, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Int32, Int32, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.model.bodyindex[base], state.model.bodyindex[body], out, opts(state)), "rbd_geometric_jacobian")
    finish(state)
    out
end

# ---- point kinematics (700 addition): P points fixed to bodies, expressed in the root frame, paths from the world — transform(state, point, world),
# point_velocity, point_acceleration and point_jacobian! (src/mechanism_algorithms.jl:168-189) over a batch.  Tree mechanisms only.

"""`set_points!(state, bodies, r)` — point k is fixed to `bodies[k]` at `r[:, k]` (3 × P, in that body's frame); the library copies them. An empty list clears them."""
function set_points!(state::BatchedMechanismState, bodies::AbstractVector{<:RigidBody}, r::AbstractMatrix{<:Real})
    checkmodcount(state)
    P = length(bodies)
    size(r) == (3, P) || throw(DimensionMismatch("r must be 3 × P"))
    idx = Int32[state.model.bodyindex[b] for b in bodies]
    rr = Vector{Float64}(vec(r))
    check(ccall((:rbd_workspace_set_points, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}), state.ws, P, idx, rr), "rbd_workspace_set_points")
    state
end

"""`point_kinematics!(state; pos, vel, acc, jac, v̇)` — every output optional: `pos`, `vel`, `acc` 3P × B, `jac` (3·nv·P) × B (per point a 3 × nv column-major
block, zero off the point's path); without `v̇` the acceleration is the bias term J̇v (`rbd_point_kinematics`)."""
function point_kinematics!(state::BatchedMechanismState{T}; pos = nothing, vel = nothing, acc = nothing, jac = nothing, v̇ = nothing) where {T}
    checkmodcount(state)
    B = batchsize(state)
    check(ccall((:rbd_point_kinematics, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, nullable(v̇), nullable(pos), nullable(vel), nullable(acc), nullable(jac), opts(state)), "rbd_point_kinematics")
    finish(state)
    nothing
end
"`point_jacobian!(out, state)` — the point Jacobians of the points of `set_points!`, (3·nv·P) × B"
point_jacobian!(out::Buffer, state::BatchedMechanismState) = (point_kinematics!(state; jac = out); out)
"`point_velocity!(out, state)` — the velocities of the points of `set_points!` in the root frame, 3P × B"
point_velocity!(out::Buffer, state::BatchedMechanismState) = (point_kinematics!(state; vel = out); out)

"""`point_kinematics_vjp!(q̄, v̄, state; pos̄, vel̄)` — positions and velocities pulled back to the raw coordinates: q̄ (nq × B) and v̄ (nv × B) are
overwritten; one of the cotangents `pos̄`, `vel̄` (3P × B) may be `nothing` (`rbd_point_kinematics_vjp`)."""
function point_kinematics_vjp!(q̄, v̄, state::BatchedMechanismState{T}; pos̄ = nothing, vel̄ = nothing) where {T}
    checkmodcount(state)
    nq, nv, B = state.model.nq, state.model.nv, batchsize(state)
    for (x, n) in ((q̄, nq), (v̄, nv))
        x === nothing || size(x) == (n, B) || throw(DimensionMismatch("cotangent buffer has wrong size"))
    end
    check(ccall((:rbd_point_kinematics_vjp, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, nullable(pos̄), nullable(vel̄), nullable(q̄), nullable(v̄), opts(state)), "rbd_point_kinematics_vjp")
    finish(state)
    q̄, v̄
end

"""`contact_dynamics_vjp!(q̄, v̄, s̄, state; c̄w, ṡ̄, s̄out)` — `contact_dynamics!` pulled back on the branch each (point, half-space) pair takes: the cotangents
of the contact wrenches `c̄w` (6·n_bodies × B), of ṡ and of the friction state after the resets (ns × B; each may be `nothing`, not all) give q̄, v̄, s̄
(overwritten).  `state.s` is read, not reset (`rbd_contact_dynamics_vjp`)."""
function contact_dynamics_vjp!(q̄, v̄, s̄, state::BatchedMechanismState{T}; c̄w = nothing, ṡ̄ = nothing, s̄out = nothing) where {T}
    checkmodcount(state)
    nq, nv, ns, B = state.model.nq, state.model.nv, size(state.s, 1), batchsize(state)
    for (x, n) in ((q̄, nq), (v̄, nv), (s̄, ns), (ṡ̄, ns), (s̄out, ns))
        x === nothing || size(x) == (n, B) || throw(DimensionMismatch("cotangent buffer has wrong size"))
    end
    check(ccall((:rbd_contact_dynamics_vjp, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, state.s, nullable(c̄w), nullable(ṡ̄), nullable(s̄out), nullable(q̄), nullable(v̄), nullable(s̄), opts(state)),
        "rbd_contact_dynamics_vjp")
    finish(state)
    q̄, v̄, s̄
end

"""`dynamics_contact_vjp!(q̄, v̄, s̄, τ̄, state; v̇̄, ṡ̄, s̄out, torques, externalwrenches, f̄ext, v̇out, ṡout)` — `dynamics!` of a mechanism with contact points
pulled back, the ODE form (q, v, s, τ, wext) -> (v̇, ṡ, s after the resets), in one call: the cotangents `v̇̄` (nv × B), `ṡ̄`, `s̄out` (ns × B; each may be
`nothing`, not all) give q̄, v̄, s̄, τ̄ and f̄ext (overwritten).  `state.s` is read, not reset (`rbd_dynamics_contact_vjp`)."""
function dynamics_contact_vjp!(q̄, v̄, s̄, τ̄, state::BatchedMechanismState{T}; v̇̄ = nothing, ṡ̄ = nothing, s̄out = nothing, torques = nothing,
        externalwrenches = nothing, f̄ext = nothing, v̇out = nothing, ṡout = nothing) where {T}
    checkmodcount(state)
    nq, nv, ns, B = state.model.nq, state.model.nv, size(state.s, 1), batchsize(state)
    for (x, n) in ((q̄, nq), (v̄, nv), (s̄, ns), (τ̄, nv), (v̇̄, nv), (ṡ̄, ns), (s̄out, ns), (v̇out, nv), (ṡout, ns))
        x === nothing || size(x) == (n, B) || throw(DimensionMismatch("cotangent buffer has wrong size"))
    end
    check(ccall((:rbd_dynamics_contact_vjp, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, state.s, nullable(torques), nullable(densewrenches(state, externalwrenches)), nullable(v̇̄), nullable(ṡ̄),
        nullable(s̄out), nullable(v̇out), nullable(ṡout), nullable(q̄), nullable(v̄), nullable(s̄), nullable(τ̄), nullable(f̄ext), opts(state)),
        "rbd_dynamics_contact_vjp")
    finish(state)
    q̄, v̄, s̄, τ̄
end

"""`simulate_contact_vjp!(q̄, v̄, s̄, state, Δt; nsteps = 1, torques, externalwrenches, τ̄, f̄ext)` — `nsteps` Munthe-Kaas RK4 steps of `simulate` of a mechanism
with contact points pulled back (`state`'s q, v and s advanced in place): q̄ (nq × B), v̄ (nv × B), s̄ (ns × B) hold the cotangent of the final state on entry
and that of the initial state on return; τ̄, f̄ext (each may be `nothing`) are overwritten with the gradient in the held torques / wrenches over every stage.
The gradient is that of the branch each (point, half-space) pair takes at each stage state (`rbd_simulate_contact_vjp`)."""
function simulate_contact_vjp!(q̄::Buffer{T}, v̄::Buffer{T}, s̄::Buffer{T}, state::BatchedMechanismState{T}, Δt::Real; nsteps::Integer = 1, torques = nothing,
        externalwrenches = nothing, τ̄ = nothing, f̄ext = nothing) where {T}
    checkmodcount(state)
    nq, nv, ns, B = state.model.nq, state.model.nv, size(state.s, 1), batchsize(state)
    Δt > 0 || throw(ArgumentError("Δt must be positive"))
    nsteps >= 0 || throw(ArgumentError("nsteps must be non-negative"))
    for (x, n) in ((q̄, nq), (v̄, nv), (s̄, ns), (τ̄, nv))
        x === nothing || size(x) == (n, B) || throw(DimensionMismatch("cotangent buffer has wrong size"))
    end
    check(ccall((:rbd_simulate_contact_vjp, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cdouble, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, state.s, nullable(torques), nullable(densewrenches(state, externalwrenches)), Float64(Δt), Int32(nsteps), q̄, v̄, s̄,
        nullable(τ̄), nullable(f̄ext), opts(state)), "rbd_simulate_contact_vjp")
    finish(state)
    q̄, v̄, s̄, τ̄
end

"""`contact_dynamics_jvp!(dcw, dṡ, dsout, state, ntan; dq, dv, ds)` — `contact_dynamics!` pushed forward along `ntan` directions per state on the branch each
(point, half-space) pair takes: the tangents of the contact wrenches (6·n_bodies·ntan × B), of ṡ and of the friction state after the resets (ns·ntan × B;
each may be `nothing`).  `state.s` is read, not reset (`rbd_contact_dynamics_jvp`)."""
function contact_dynamics_jvp!(dcw, dṡ, dsout, state::BatchedMechanismState{T}, ntan::Integer; dq = nothing, dv = nothing, ds = nothing) where {T}
    checkmodcount(state)
    nq, nv, ns, B = state.model.nq, state.model.nv, size(state.s, 1), batchsize(state)
    ntan > 0 || throw(ArgumentError("ntan must be positive"))
    for (x, n) in ((dṡ, ns), (dsout, ns), (dq, nq), (dv, nv), (ds, ns))
        x === nothing || size(x) == (n * ntan, B) || throw(DimensionMismatch("tangent buffer has wrong size"))
    end
    check(ccall((:rbd_contact_dynamics_jvp, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, ntan, state.q, state.v, state.s, nullable(dq), nullable(dv), nullable(ds), nullable(dcw), nullable(dṡ), nullable(dsout), opts(state)),
        "rbd_contact_dynamics_jvp")
    finish(state)
    dcw, dṡ, dsout
end

"""`dynamics_contact_jvp!(dv̇, dṡ, dsout, state, ntan; torques, externalwrenches, dq, dv, ds, dτ, dexternalwrenches, v̇out, ṡout)` — `dynamics!` of a mechanism
with contact points pushed forward along `ntan` directions per state, the ODE form (q, v, s, τ, wext) -> (v̇, ṡ, s after the resets), in one pass: what
`ForwardDiff` computes through `dynamics!` of such a mechanism (`rbd_dynamics_contact_jvp`)."""
function dynamics_contact_jvp!(dv̇, dṡ, dsout, state::BatchedMechanismState{T}, ntan::Integer; torques = nothing, externalwrenches = nothing, dq = nothing,
        dv = nothing, ds = nothing, dτ = nothing, dexternalwrenches = nothing, v̇out = nothing, ṡout = nothing) where {T}
    checkmodcount(state)
    nq, nv, ns, B = state.model.nq, state.model.nv, size(state.s, 1), batchsize(state)
    ntan > 0 || throw(ArgumentError("ntan must be positive"))
    for (x, n) in ((dv̇, nv), (dṡ, ns), (dsout, ns), (dq, nq), (dv, nv), (ds, ns), (dτ, nv))
        x === nothing || size(x) == (n * ntan, B) || throw(DimensionMismatch("tangent buffer has wrong size"))
    end
    check(ccall((:rbd_dynamics_contact_jvp, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, ntan, state.q, state.v, state.s, nullable(torques), nullable(densewrenches(state, externalwrenches)), nullable(dq), nullable(dv),
        nullable(ds), nullable(dτ), nullable(dexternalwrenches), nullable(v̇out), nullable(ṡout), nullable(dv̇), nullable(dṡ), nullable(dsout), opts(state)),
        "rbd_dynamics_contact_jvp")
    finish(state)
    dv̇, dṡ, dsout
end

"""`dynamics_contact_derivatives!(∂v̇∂q, ∂v̇∂v, ∂v̇∂s, ∂v̇∂τ, ∂ṡ∂q, ∂ṡ∂v, ∂ṡ∂s, state; torques, externalwrenches, v̇out, ṡout)` — the Jacobians of `dynamics!` of a
mechanism with contact points (fext fixed), column-major per state: (nv·nq), (nv·nv), (nv·ns), (nv·nv) = M⁻¹, (ns·nq), (ns·nv), (ns·ns) × B; each may be
`nothing` (`rbd_dynamics_contact_derivatives`)."""
function dynamics_contact_derivatives!(dv̇dq, dv̇dv, dv̇ds, dv̇dτ, dṡdq, dṡdv, dṡds, state::BatchedMechanismState{T}; torques = nothing, externalwrenches = nothing,
        v̇out = nothing, ṡout = nothing) where {T}
    checkmodcount(state)
    nq, nv, ns, B = state.model.nq, state.model.nv, size(state.s, 1), batchsize(state)
    for (x, n) in ((dv̇dq, nv * nq), (dv̇dv, nv * nv), (dv̇ds, nv * ns), (dv̇dτ, nv * nv), (dṡdq, ns * nq), (dṡdv, ns * nv), (dṡds, ns * ns))
        x === nothing || size(x) == (n, B) || throw(DimensionMismatch("Jacobian buffer has wrong size"))
    end
    check(ccall((:rbd_dynamics_contact_derivatives, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, state.s, nullable(torques), nullable(densewrenches(state, externalwrenches)), nullable(v̇out), nullable(ṡout),
        nullable(dv̇dq), nullable(dv̇dv), nullable(dv̇ds), nullable(dv̇dτ), nullable(dṡdq), nullable(dṡdv), nullable(dṡds), opts(state)),
        "rbd_dynamics_contact_derivatives")
    finish(state)
    dv̇dq, dv̇dv, dv̇ds, dv̇dτ, dṡdq, dṡdv, dṡds
end

"""`simulate_contact_jvp!(dq, dv, ds, state, ntan, Δt; nsteps = 1, torques, dτ, externalwrenches, dexternalwrenches)` — `nsteps` Munthe-Kaas RK4 steps of
`simulate` of a mechanism with contact points with `ntan` directions per state carried along: `state`'s q, v and s, `dq` ((nq·ntan) × B), `dv` ((nv·ntan) × B)
and `ds` ((ns·ntan) × B) advanced in place; `dτ` and the wrench directions held over every stage.  The derivative is that of the branch each (point,
half-space) pair takes at each stage state (`rbd_simulate_contact_jvp`)."""
function simulate_contact_jvp!(dq::Buffer{T}, dv::Buffer{T}, ds::Buffer{T}, state::BatchedMechanismState{T}, ntan::Integer, Δt::Real; nsteps::Integer = 1,
        torques = nothing, dτ = nothing, externalwrenches = nothing, dexternalwrenches = nothing) where {T}
    checkmodcount(state)
    nq, nv, ns, B = state.model.nq, state.model.nv, size(state.s, 1), batchsize(state)
    ntan > 0 || throw(ArgumentError("ntan must be positive"))
    Δt > 0 || throw(ArgumentError("Δt must be positive"))
    nsteps >= 0 || throw(ArgumentError("nsteps must be non-negative"))
    for (x, n) in ((dq, nq), (dv, nv), (ds, ns), (dτ, nv))
        x === nothing || size(x) == (n * ntan, B) || throw(DimensionMismatch("tangent buffer has wrong size"))
    end
    check(ccall((:rbd_simulate_contact_jvp, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cdouble, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, ntan, state.q, state.v, state.s, nullable(torques), nullable(densewrenches(state, externalwrenches)), Float64(Δt), Int32(nsteps), dq, dv,
        ds, nullable(dτ), nullable(dexternalwrenches), opts(state)), "rbd_simulate_contact_jvp")
    finish(state)
    dq, dv, ds
end

"""`simulate_contact_step_derivatives!(∂x∂x, ∂x∂τ, state, Δt; torques, externalwrenches)` — one step of `simulate` of a mechanism with contact points (`state`'s
q, v and s advanced in place) and its Jacobians with x = (q; v; s), nx = nq + nv + ns: (nx·nx) × B and (nx·nv) × B, column-major per state, either one
`nothing`; the wrenches held fixed (`rbd_simulate_contact_step_derivatives`)."""
function simulate_contact_step_derivatives!(dxdx, dxdτ, state::BatchedMechanismState{T}, Δt::Real; torques = nothing, externalwrenches = nothing) where {T}
    checkmodcount(state)
    nq, nv, ns, B = state.model.nq, state.model.nv, size(state.s, 1), batchsize(state)
    nx = nq + nv + ns
    Δt > 0 || throw(ArgumentError("Δt must be positive"))
    for (x, n) in ((dxdx, nx * nx), (dxdτ, nx * nv))
        x === nothing || size(x) == (n, B) || throw(DimensionMismatch("Jacobian buffer has wrong size"))
    end
    check(ccall((:rbd_simulate_contact_step_derivatives, librbd_hip[]), Cint,
        (Ptr{Cvoid}, Int32, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Ptr{T}, Cdouble, Ptr{T}, Ptr{T}, Ref{RbdOpts}),
        state.ws, B, state.q, state.v, state.s, nullable(torques), nullable(densewrenches(state, externalwrenches)), Float64(Δt), nullable(dxdx),
        nullable(dxdτ), opts(state)), "rbd_simulate_contact_step_derivatives")
    finish(state)
    dxdx, dxdτ
end

# ---- multi-GPU: one process per GPU, the batch sharded by state, v̇ gathered over RCCL (SURVEY.md §8 e) ------------------------------
mutable struct RbdComm
    handle::Ptr{Cvoid}
    world::Int; rank::Int
end
"128-byte unique id (call on one rank, hand to the others by whatever means the launcher offers — MPI, a file, a socket)"
function unique_id()
    id = zeros(UInt8, 128)
    check(ccall((:rbd_comm_unique_id, librbd_hip[]), Cint, (Ptr{Cvoid},), id), "rbd_comm_unique_id")
    id
end
function RbdComm(id::Vector{UInt8}, world::Integer, rank::Integer; device::Integer = 0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:rbd_comm_create, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Int32, Int32, Ref{Ptr{Cvoid}}), id, world, rank, device, h), "rbd_comm_create")
    c = RbdComm(h[], world, rank)
    finalizer(x -> ccall((:rbd_comm_destroy, librbd_hip[]), Cint, (Ptr{Cvoid},), x.handle), c)
    c
end
"gathered (n × world·B_local) ← every rank's shard (n × B_local); `root = nothing`: on every rank, else on that rank only"
function gather!(gathered::Union{DeviceMatrix{T}, Nothing}, comm::RbdComm, shard::DeviceMatrix{T}; root = nothing) where {T}
    check(ccall((:rbd_gather, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}),
        comm.handle, T === Float64 ? 0 : 1, shard.ptr, gathered === nothing ? C_NULL : gathered.ptr, prod(size(shard)), root === nothing ? -1 : root, C_NULL), "rbd_gather")
    gathered
end
"... of shards with different numbers of states: `cols[r + 1]` states on rank r (a batch that does not divide by the number of ranks), gathered n × sum(cols)"
function gatherv!(gathered::Union{DeviceMatrix{T}, Nothing}, comm::RbdComm, shard::DeviceMatrix{T}, cols::AbstractVector{<:Integer}; root = nothing) where {T}
    length(cols) == comm.world && cols[comm.rank + 1] == size(shard, 2) || throw(DimensionMismatch("cols must list every rank's states; cols[rank + 1] must be this shard's"))
    counts = Int64[size(shard, 1) * c for c in cols]
    check(ccall((:rbd_gatherv, librbd_hip[]), Cint, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Int32, Ptr{Cvoid}),
        comm.handle, T === Float64 ? 0 : 1, shard.ptr, gathered === nothing ? C_NULL : gathered.ptr, counts, root === nothing ? -1 : root, C_NULL), "rbd_gatherv")
    gathered
end

end # module
