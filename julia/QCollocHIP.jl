# QCollocHIP.jl — thin `ccall` layer over libqcolloc_hip.so (include/qcolloc.h).
#
# UNTESTED IN THIS REPOSITORY'S CI: the build image has no Julia.  It is the binding a maintainer of
# QuantumCollocation.jl would add; it builds an object with the fields the MOI evaluator of
# QuantumCollocationCore consumes — `F`, `∂F`, `∂F_structure`, `μ∂²F`, `μ∂²F_structure`, `dim` —
# exactly as they are used in test/scripts/integrator_test_1qubit.jl:41-52, so that replacing the constructor call of that script,
#
#     dynamics = QuantumDynamics(f, Z)        ->        dynamics = QCollocHIP.QuantumDynamics(f, Z)
#
# (line 41; the same positional arguments) swaps the CPU per-knot loop for the MI355X kernels while Ipopt keeps driving the solve unchanged.
module QCollocHIP

using Libdl

const LIB = Ref{String}(get(ENV, "QCOLLOC_HIP_LIB", "libqcolloc_hip.so"))
const QC_MAX_DERIV = 8
const QC_SWEEP_WIDE = 1            # qc_sweep_desc.wide, bit 0: the matrix-core form up to 2N = 32 ("mfma32-sweep")
const QC_SWEEP_WIDE_TANGENT = 16   # qc_sweep_desc.wide, bit 4 (only with bit 0): pushforwards in that form
const QC_SWEEP_WIDE_NOISE = 64     # qc_sweep_desc.wide, bit 6 (only with bit 0): noise-trajectory sweeps and their gradients in that form
const QC_SWEEP_WIDE_HESSIAN = 256  # qc_sweep_desc.wide, bit 8 (only with bit 0): Hessian products of closed systems in that form
const QC_SWEEP_WIDE_64_GRAD = 2048 # qc_sweep_desc.wide, bit 11 (only with bits 0 and 10): gradients and pullbacks of closed systems in the "mfma64-sweep" form
const QC_SWEEP_WIDE_64_PARAMS = 8192 # qc_sweep_desc.wide, bit 13 (only with bits 0, 10 and 11): parameter gradients and parameter cotangents in the "mfma64-sweep" form
const QC_SWEEP_WIDE_64_TANGENT = 16384 # qc_sweep_desc.wide, bit 14 (only with bits 0 and 10): pushforwards in the "mfma64-sweep" form, any generators, 2N·cols ≤ 2048
const QC_SWEEP_WIDE_64_NOISE = 65536 # qc_sweep_desc.wide, bit 16 (only with bits 0 and 10): noise-trajectory sweeps in the "mfma64-sweep" form (their gradients with bit 11 as well)
const QC_SWEEP_WIDE_64_STORED = 262144 # qc_sweep_desc.wide, bit 18 (only with bits 0, 10 and 11): with stored_states, reverse mode of ANY generators in the "mfma64-sweep" form (at most 32 state columns)
const QC_SWEEP_WIDE_64 = 1024      # qc_sweep_desc.wide, bit 10 (only with bit 0): 32 < 2N ≤ 64 with up to 16 drives on the matrix cores ("mfma64-sweep", forward sweep only)
const QC_ABI_VERSION = 6      # QC_VERSION_MAJOR * 1000 + QC_VERSION_MINOR of the include/qcolloc.h these mirrors were written against

# mirror of `qc_desc` (include/qcolloc.h); field order and types must match the header -- `__init__` checks the sizes against
# the library's own `sizeof` (qc_sizeof_desc / qc_sizeof_dims / qc_sizeof_terms_desc) when the module is loaded
struct QCDesc
    N::Int32; m::Int32; T::Int64; zdim::Int32; global_dim::Int64
    off_U::Int32; off_a::Int32; off_dt::Int32; dt_fixed::Float64
    integrator::Int32; pade_order::Int32; n_deriv::Int32
    deriv_x_off::NTuple{QC_MAX_DERIV,Int32}; deriv_dx_off::NTuple{QC_MAX_DERIV,Int32}; deriv_dim::NTuple{QC_MAX_DERIV,Int32}
    G_drift::Ptr{Float64}; G_drives::Ptr{Float64}
    device::Int32; kernel::Int32; t_begin::Int64; t_end::Int64
    state_cols::Int32                       # 0 = unitary iso-vec; K = K ket integrators stored back to back
    hess_align::Int32                       # 0 / 1 = exactly the structural entries (default); 16 = interval blocks padded to whole 128-byte lines
    rows_per_interval::Int64; row_offset::Int64; jac_per_interval::Int64; jac_offset::Int64   # composition (all 0 =
    hess_per_interval::Int64; hess_offset::Int64                                               # this handle is the whole dynamics)
    row_placement::Int32                    # 0 = rows stacked in integrator order, 1 = rows at the state components' positions
    hess_tail_zeros::Int32
    deriv_row_off::NTuple{QC_MAX_DERIV,Int32}
    jac_block_order::NTuple{5,Int32}        # order of the value blocks inside an interval (ABI 0.6): permutations of QC_JB_* / QC_HB_*,
    hess_block_order::NTuple{8,Int32}       # all zeros = the library's default order (what `julia/reconcile.jl` prints is Core's)
end

struct QCDims
    n_rows::Int64; n_cols::Int64; ddim::Int64; jac_nnz_interval::Int64; hess_nnz_interval::Int64
    n_intervals::Int64; F_len::Int64; jac_nnz::Int64; hess_nnz::Int64; Z_len::Int64; kernel::Int32; reserved::Int32
end

# mirror of `qc_terms_desc`
struct QCTermsDesc
    T::Int64; zdim::Int32; off_dt::Int32; global_dim::Int64; dt_fixed::Float64
    n_reg::Int32; weighting::Int32; reg_index::Ptr{Int32}; reg_R::Ptr{Float64}; reg_baseline::Ptr{Float64}
    min_time_D::Float64; min_time_knots::Int64; device::Int32; reserved0::Int32
end

# mirror of `qc_terms_ext`
struct QCTermsExt
    n_smooth::Int32; n_pair::Int32; n_lin::Int32; reserved0::Int32
    smooth_index::Ptr{Int32}; smooth_R::Ptr{Float64}; pair_a::Ptr{Int32}; pair_b::Ptr{Int32}; pair_Q::Ptr{Float64}
    lin_index::Ptr{Int32}; lin_w::Ptr{Float64}; reserved1::NTuple{2,Int64}
end

# mirror of `qc_fidelity_desc`
struct QCFidelityDesc
    kind::Int32; N::Int32; goal_iso::Ptr{Float64}; subspace::Ptr{Int32}; n_sub::Int32; form::Int32; n_phases::Int32; device::Int32
    phase_dims::Ptr{Int32}; phase_ops::Ptr{Float64}
end

# mirror of `qc_robust_desc`
struct QCRobustDesc
    T::Int64; zdim::Int32; off_state::Int32; N::Int32; n_sub::Int32; subspace::Ptr{Int32}
    H_re::Ptr{Float64}; H_im::Ptr{Float64}; off_dt::Int32; reserved0::Int32; dt_fixed::Float64
    global_dim::Int64; n_knots::Int64; hessian::Int32; device::Int32; reserved1::NTuple{2,Int64}
end

# mirror of `qc_sweep_desc`
struct QCSweepDesc
    T::Int64; zdim::Int32; off_a::Int32; off_dt::Int32; N::Int32; dt_fixed::Float64; global_dim::Int64
    m::Int32; state_cols::Int32; n_pert::Int32; fid_kind::Int32
    G_drift::Ptr{Float64}; G_drives::Ptr{Float64}; G_pert::Ptr{Float64}
    fid_form::Int32; n_sub::Int32; goal_iso::Ptr{Float64}; subspace::Ptr{Int32}
    device::Int32; wide::Int32; reserved1::NTuple{2,Int64}
end

function __init__()
    # constants were renumbered between ABI 0.1 / 0.2 / 0.3 and retired in 0.4 (QC_REG_*): the struct sizes do not show that, the version does
    abi = ccall(dlsym(dlopen(LIB[]), :qc_abi_version), Int32, ())
    abi == QC_ABI_VERSION || error("QCollocHIP: $(LIB[]) has ABI version $abi, this binding mirrors $QC_ABI_VERSION")
    # a stale mirror would corrupt memory silently: compare with the structs the library was compiled with
    for (sym, T) in ((:qc_sizeof_desc, QCDesc), (:qc_sizeof_dims, QCDims), (:qc_sizeof_terms_desc, QCTermsDesc),
                     (:qc_sizeof_robust_desc, QCRobustDesc), (:qc_sizeof_terms_ext, QCTermsExt),
                     (:qc_sizeof_sweep_desc, QCSweepDesc))
        lib = ccall(dlsym(dlopen(LIB[]), sym), Int64, ())
        lib == sizeof(T) || error("QCollocHIP: $(T) has $(sizeof(T)) bytes, $(LIB[]) expects $lib (header / binding version mismatch)")
    end
end

function check(rc::Cint, h::Ptr{Cvoid}=C_NULL)
    rc == 0 && return
    msg = unsafe_string(ccall((:qc_last_error, LIB[]), Cstring, (Ptr{Cvoid},), h))
    error("libqcolloc_hip error $rc: $msg")
end

pad8(v) = ntuple(i -> i <= length(v) ? Int32(v[i]) : Int32(0), QC_MAX_DERIV)

# Pinned host memory of the library (`qc_host_alloc`) for the optional result rings.  The blocks belong to ONE owner object that the
# `HIPDynamics` references and that frees them in its own finalizer, after `qc_destroy` (ADVICE round 4): `reshape` / `vec` of a
# result on Julia >= 1.11 share the memory without keeping the wrapping Array alive, so a per-array finalizer could free a block under
# a live alias.  RING RESULTS MUST NOT OUTLIVE THE DYNAMICS OBJECT; `fresh = true` (and the default `result_ring = 0`) return ordinary
# Julia vectors with no such condition.
mutable struct PinnedOwner
    blocks::Vector{Ptr{Cvoid}}
end
free_pinned!(o::PinnedOwner) = (foreach(p -> ccall((:qc_host_free, LIB[]), Cint, (Ptr{Cvoid},), p), o.blocks); empty!(o.blocks); nothing)
function pinned_zeros!(o::PinnedOwner, len::Integer)
    len * 8 >= 65536 || return zeros(Float64, len)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    ccall((:qc_host_alloc, LIB[]), Cint, (Int64, Ptr{Ptr{Cvoid}}), len * 8, p) == 0 || return zeros(Float64, len)
    push!(o.blocks, p[])
    return fill!(unsafe_wrap(Array, Ptr{Float64}(p[]), len; own=false), 0.0)
end
# Result vectors of one closure, handed out in turn (opt-in): allocated (pinned) and written once when the ring is built, so that no call
# pays for page faults or per-call pinning.
struct ResultRing
    bufs::Vector{Vector{Float64}}
    next::Base.RefValue{Int}
end
ResultRing(o::PinnedOwner, len::Integer, n::Integer) = ResultRing(Vector{Float64}[pinned_zeros!(o, len) for _ in 1:(len > 0 ? n : 0)], Ref(1))
function next!(r::ResultRing, len::Integer, fresh::Bool)
    (fresh || isempty(r.bufs)) && return Vector{Float64}(undef, len)
    v = r.bufs[r.next[]]
    r.next[] = r.next[] % length(r.bufs) + 1
    return v
end

"""
Field-compatible stand-in for `QuantumDynamics` (QuantumCollocationCore.Dynamics).

`F(Z⃗)`, `∂F(Z⃗)`, `μ∂²F(Z⃗, μ⃗)` -- the only shapes QuantumCollocationCore's evaluator uses (test/scripts/integrator_test_1qubit.jl:45-52)
-- return a newly allocated vector that is the caller's for good, as the reference's closures do (`result_ring = 0`, the default).
A fresh `Vector{Float64}(undef, 5_034_960)` per `∂F` call costs 2.7 - 4 ms of first-touch page faults at BASELINE config 3, ten times
the evaluation: an evaluator that copies each result into Ipopt's buffer at once (Core's does) opts in to `result_ring = 3` -- the next
vector of a ring of three per closure, pinned and written once when the ring is built; such a result stays intact until the third-next
call OF THE SAME CLOSURE and must not outlive the dynamics object; `∂F(Z⃗; fresh=true)` still allocates.
`F!`, `∂F!`, `μ∂²F!` write into a caller-owned vector (what an evaluator that owns the MOI callbacks does with Ipopt's buffers).
"""
mutable struct HIPDynamics
    handle::Ptr{Cvoid}
    dims::QCDims
    F::Function
    ∂F::Function
    ∂F_structure::Vector{Tuple{Int,Int}}
    μ∂²F::Union{Function,Nothing}
    μ∂²F_structure::Union{Vector{Tuple{Int,Int}},Nothing}
    dim::Int
    F!::Function
    ∂F!::Function
    μ∂²F!::Union{Function,Nothing}
    handles::Vector{Ptr{Cvoid}}      # every qc_handle this object owns (one; one per state integrator for `dynamics_list`)
    pinned::PinnedOwner              # the result rings' memory
end
# handles first, then the pinned blocks (nothing of the library refers to them once the handles are gone)
function release!(dyn::HIPDynamics)
    foreach(h -> ccall((:qc_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), h), dyn.handles)
    empty!(dyn.handles)
    dyn.handle = C_NULL
    free_pinned!(dyn.pinned)
end

# first row of state component `name` among the trajectory's state components (controls carry no dynamics rows)
function state_row_offset(traj, name)
    r = 0
    for other in traj.names
        other == name && return r
        other in traj.control_names || (r += length(traj.components[other]))
    end
    error("no state component $name")
end

# qc_desc.jac_block_order / hess_block_order: `nothing` = the library's default order (all zeros), else a permutation of 0:n-1
block_order(order, n::Int) = isnothing(order) ? ntuple(_ -> Int32(0), n) :
    (sort(collect(order)) == collect(0:n-1) || error("block order must be a permutation of 0:$(n-1)"); ntuple(i -> Int32(order[i]), n))

"""
    dynamics(integrators, traj, system; device=0, devices=nothing, eval_hessian=true, rows=:stacked, padded=false, result_ring=0)

`integrators[1]` must be the `UnitaryPadeIntegrator` / `UnitaryExponentialIntegrator`, followed by
`DerivativeIntegrator`s (the order of unitary_smooth_pulse_problem.jl:175-179).  `component_offset(traj, name)`
is `first(traj.components[name]) - 1`.

`devices = 0:7` builds ONE evaluator over several GPUs (`qc_create_multi`): the knots are sharded inside the library, each
GPU copies its own contiguous slice of `∂F` into the caller's vector over its own PCIe link; everything else is unchanged.
`rows = :by_component` places every integrator's rows at its state component's position (`Z.dims.states` rows per interval).
`μ∂²F_structure` holds exactly the structural entries (config 3: 1 832 per interval), so `length` and `==` comparisons with
QuantumCollocationCore's own structure are meaningful (julia/reconcile.jl).  `padded = true` (= `hess_align = 16`) is the layout of
device-resident consumers: every interval's value block padded to whole cache lines with explicit zero duplicates, which a COO
consumer sums away -- a host-buffer call is bound by PCIe and gains nothing from it.
`set_new_x!(dyn, false)` is Ipopt's `new_x = false`: the following calls reuse the knots already on the device.
`result_ring`: 0 (default) = `F` / `∂F` / `μ∂²F` return fresh vectors; n >= 3 = rings of n pinned result vectors per closure (see `HIPDynamics`).
`jac_block_order` / `hess_block_order`: the order of the value blocks inside an interval (`qc_desc.jac_block_order`, ABI 0.6) -- a
permutation of `0:4` (−F copies, B copies / identity, ∂a, ∂Δt, derivative integrators) / `0:7` ((Ũ_t,a), (a,Ũ_t+1), (Ũ_t,Δt),
(Δt,Ũ_t+1), (a,a), (a,Δt), (Δt,Δt), (dx,Δt)); `julia/reconcile.jl` prints the order QuantumCollocationCore's structures have.
"""
function dynamics(integrators, traj, system; device::Int=0, devices=nothing, eval_hessian::Bool=true,
                  state_name=:Ũ⃗, control_name=:a, pade_order::Int=4, exponential::Bool=false,
                  derivative_pairs=[(:a, :da), (:da, :dda)], n_kets::Int=0, rows::Symbol=:stacked, hess_align::Int=0,
                  padded::Bool=false, result_ring::Int=0, offsets=nothing, generators=nothing,
                  jac_block_order=nothing, hess_block_order=nothing)
    (result_ring == 0 || result_ring >= 3) || error("result_ring must be 0 (fresh vectors) or at least 3")
    padded && (hess_align = 16)
    # `offsets` (0-based positions inside a knot, keyed by name) and `generators` = (G_drift, [G_1 .. G_m]) override what is read from
    # `traj.components` and `system`: what `QuantumDynamics(integrators, traj)` below passes after reading the integrator objects
    off(name) = (!isnothing(offsets) && haskey(offsets, name)) ? Int(offsets[name]) : first(traj.components[name]) - 1
    G0 = Matrix{Float64}(isnothing(generators) ? system.G_drift : generators[1])                       # column-major n x n
    Gs = isnothing(generators) ? system.G_drives : generators[2]
    Gd = reduce(hcat, [vec(Matrix{Float64}(G)) for G in Gs])   # n^2 x m, column j = vec(G_j)
    levels = size(G0, 1) ÷ 2
    free_time = traj.timestep isa Symbol
    xs = [off(p[1]) for p in derivative_pairs]; dxs = [off(p[2]) for p in derivative_pairs]
    dms = [length(traj.components[p[1]]) for p in derivative_pairs]
    bycomp = rows == :by_component
    h = Ref{Ptr{Cvoid}}(C_NULL)
    dims = Ref{QCDims}()
    devs = isnothing(devices) ? Int32[] : Int32.(collect(devices))
    GC.@preserve G0 Gd devs begin
        desc = Ref(QCDesc(levels, length(Gs), traj.T, traj.dim, traj.global_dim,
                          off(state_name), off(control_name), free_time ? off(traj.timestep) : -1,
                          free_time ? 0.0 : Float64(traj.timestep),
                          exponential ? 1 : 0, exponential ? 0 : pade_order, length(derivative_pairs),
                          pad8(xs), pad8(dxs), pad8(dms), pointer(G0), pointer(Gd),
                          isempty(devs) ? device : devs[1], 0, 0, 0, n_kets, hess_align,
                          bycomp ? traj.dims.states : 0, bycomp ? state_row_offset(traj, state_name) : 0, 0, 0, 0, 0,
                          bycomp ? 1 : 0, 0, bycomp ? pad8([state_row_offset(traj, p[1]) for p in derivative_pairs]) : pad8(Int[]),
                          block_order(jac_block_order, 5), block_order(hess_block_order, 8)))
        if isempty(devs)
            check(ccall((:qc_create, LIB[]), Cint, (Ref{QCDesc}, Ref{Ptr{Cvoid}}), desc, h))
        else
            check(ccall((:qc_create_multi, LIB[]), Cint, (Ref{QCDesc}, Int32, Ptr{Int32}, Ref{Ptr{Cvoid}}), desc, length(devs), devs, h))
        end
    end
    check(ccall((:qc_dims, LIB[]), Cint, (Ptr{Cvoid}, Ref{QCDims}), h[], dims), h[])
    d = dims[]
    rows_ = Vector{Int64}(undef, d.jac_nnz); cols = similar(rows_)
    check(ccall((:qc_jac_structure, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Cint), h[], rows_, cols, 1), h[])
    ∂F_structure = collect(zip(Int.(rows_), Int.(cols)))          # 1-based (row, col) tuples, value order
    F! = function (out::AbstractVector{Float64}, Z⃗::AbstractVector{Float64})
        length(out) == d.F_len || error("F!: output has length $(length(out)), expected $(d.F_len)")
        GC.@preserve Z⃗ out check(ccall((:qc_eval_F, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), h[], Z⃗, out), h[])
        return out
    end
    ∂F! = function (out::AbstractVector{Float64}, Z⃗::AbstractVector{Float64})
        length(out) == d.jac_nnz || error("∂F!: output has length $(length(out)), expected $(d.jac_nnz)")
        GC.@preserve Z⃗ out check(ccall((:qc_eval_jac, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), h[], Z⃗, out), h[])
        return out
    end
    pinned = PinnedOwner(Ptr{Cvoid}[])
    ringF = ResultRing(pinned, d.F_len, result_ring); ring∂F = ResultRing(pinned, d.jac_nnz, result_ring)
    F = (Z⃗; fresh::Bool=false) -> F!(next!(ringF, d.F_len, fresh), Z⃗)
    ∂F = (Z⃗; fresh::Bool=false) -> ∂F!(next!(ring∂F, d.jac_nnz, fresh), Z⃗)
    μ∂²F = nothing; μ∂²F! = nothing; μ∂²F_structure = nothing
    if eval_hessian && d.hess_nnz > 0
        hr = Vector{Int64}(undef, d.hess_nnz); hc = similar(hr)
        check(ccall((:qc_hess_structure, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Cint), h[], hr, hc, 1), h[])
        μ∂²F_structure = collect(zip(Int.(hr), Int.(hc)))       # upper triangle, as test/test_utils.jl:14-27 expects; with
                                                                # `padded` the padding repeats an entry with value 0 (duplicates are summed)
        μ∂²F! = function (out::AbstractVector{Float64}, Z⃗::AbstractVector{Float64}, μ⃗::AbstractVector{Float64})
            length(out) == d.hess_nnz || error("μ∂²F!: output has length $(length(out)), expected $(d.hess_nnz)")
            length(μ⃗) == d.n_rows || error("μ∂²F!: μ has length $(length(μ⃗)), expected $(d.n_rows)")
            GC.@preserve Z⃗ μ⃗ out check(ccall((:qc_eval_hess, LIB[]), Cint,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h[], Z⃗, μ⃗, out), h[])
            return out
        end
        ringH = ResultRing(pinned, d.hess_nnz, result_ring)
        μ∂²F = (Z⃗, μ⃗; fresh::Bool=false) -> μ∂²F!(next!(ringH, d.hess_nnz, fresh), Z⃗, μ⃗)
    end
    dyn = HIPDynamics(h[], d, F, ∂F, ∂F_structure, μ∂²F, μ∂²F_structure, Int(bycomp ? traj.dims.states : d.ddim), F!, ∂F!, μ∂²F!,
                      Ptr{Cvoid}[h[]], pinned)
    finalizer(release!, dyn)
    return dyn
end

# ---------------------------------------------------------------------------------------------------------------
#  The reference's own constructor call: QuantumDynamics(integrators, traj)        (test/scripts/integrator_test_1qubit.jl:41)
# ---------------------------------------------------------------------------------------------------------------

# first of `names` that is a property of `x` (nothing when none is): the integrator structs of QuantumCollocationCore are not vendored
# with the reference, so every field is looked up under the names recalled for 0.3.x (SURVEY Appendix B) AND has a keyword fallback
function field_of(x, names...)
    for nm in names
        hasproperty(x, nm) && return getproperty(x, nm)
    end
    return nothing
end
type_name(x) = String(nameof(typeof(x)))
is_derivative_integrator(x) = occursin("DerivativeIntegrator", type_name(x))
is_state_integrator(x) = !is_derivative_integrator(x) && (occursin("Pade", type_name(x)) || occursin("Exponential", type_name(x)))
# trajectory component whose index range starts at `first_index` (1-based position inside a knot)
function component_at(traj, first_index::Integer)
    for nm in traj.names
        first(traj.components[nm]) == first_index && return nm
    end
    error("QCollocHIP.QuantumDynamics: no trajectory component starts at knot position $first_index")
end
# (G_drift, [G_1 .. G_m]) from the integrator's generator closure G(a) = G_drift + sum_j a_j G_j (affine in a: m + 1 evaluations),
# and ONE more evaluation at a generic point that checks the assumption: a closure that is not affine in a (a nonlinear drive, a
# time-dependent frame) would otherwise be replaced by its linearisation without a word (ADVICE round 5)
function generators_from_closure(G, m::Integer)
    G0 = Matrix{Float64}(G(zeros(m)))
    Gs = [Matrix{Float64}(G([j == k ? 1.0 : 0.0 for k in 1:m])) - G0 for j in 1:m]
    a = [0.37 + 0.21 * k - 0.05 * k^2 for k in 1:m]
    model = m == 0 ? G0 : G0 + sum(a[k] * Gs[k] for k in 1:m)
    err = maximum(abs, Matrix{Float64}(G(a)) - model; init=0.0)
    err <= 1e-12 * max(1.0, maximum(abs, model; init=0.0)) ||
        error("QCollocHIP.QuantumDynamics: the integrator's generator closure G(a) is not affine in a (deviation $err at a test point): " *
              "this library evaluates G(a) = G_drift + sum_j a_j G_j only; pass `system = ...` if the closure is not the system's")
    return G0, Gs
end

"""
    QuantumDynamics(integrators, traj; system=nothing, state_name=nothing, control_name=nothing, pade_order=nothing,
                    derivative_pairs=nothing, kwargs...)

The positional arguments of the reference's own constructor call, `dynamics = QuantumDynamics(f, Z)` with `f = [P, D]`
(test/scripts/integrator_test_1qubit.jl:39-41; `QuantumControlProblem` makes the same call with `prob.integrators`,
unitary_smooth_pulse_problem.jl:175-190): qualifying that one call with `QCollocHIP.` is the whole change to the script.
Everything `dynamics(integrators, traj, system; ...)` needs is read from the integrator objects:

| needed                         | read from (first that exists)                                                  | keyword fallback     |
|--------------------------------|--------------------------------------------------------------------------------|----------------------|
| state component                | `P.unitary_components` / `P.state_components` (index range inside a knot), `P.unitary_name` / `P.state_name` / `P.state_symb` | `state_name`  |
| control component              | `P.drive_components`, `P.control_name` / `P.drive_name` / `P.drive_symb`      | `control_name`       |
| generators `G_drift, G_drives` | `P.system` (`.G_drift`, `.G_drives`), else `P.G_drift` / `P.G_drives`, else the closure `P.G` evaluated at `0` and the unit vectors | `system` |
| Padé order                     | `P.order` (an `...ExponentialIntegrator` type name selects the exponential)    | `pade_order`         |
| derivative integrators         | `D.variable_components` / `D.derivative_components`, or `D.variable` / `D.derivative` names, of every element whose type name contains `DerivativeIntegrator` | `derivative_pairs` |

NOT YET A VERIFIED DROP-IN: this constructor has never run against QuantumCollocationCore (no Julia in the build image; ADVICE
round 5) -- `julia/reconcile.jl` is the first thing to run on a machine that has both.
The field names are those recalled for QuantumCollocationCore 0.3.x (not vendored with the reference, SURVEY Appendix B): a field that
is absent under every listed name raises an error naming the keyword that supplies it.  Lists with several state integrators (sampling
and direct-sum problems) go to `dynamics_list`.  Remaining keywords (`device`, `devices`, `eval_hessian`, `rows`, `padded`,
`result_ring`) are `dynamics`' own.
"""
function QuantumDynamics(integrators::AbstractVector, traj; system=nothing, state_name=nothing, control_name=nothing,
                         pade_order=nothing, derivative_pairs=nothing, kwargs...)
    states = [I for I in integrators if is_state_integrator(I)]
    derivs = [I for I in integrators if is_derivative_integrator(I)]
    length(states) + length(derivs) == length(integrators) || error("QCollocHIP.QuantumDynamics: an integrator is neither a Padé / exponential state integrator nor a DerivativeIntegrator")
    isempty(states) && error("QCollocHIP.QuantumDynamics: the list holds no state integrator")
    need(x, what, kw) = isnothing(x) ? error("QCollocHIP.QuantumDynamics: cannot read $what from $(type_name(states[1])); pass `$kw = ...`") : x
    component(I, range_fields, name_fields, given, what, kw) = begin
        !isnothing(given) && return given
        r = field_of(I, range_fields...)
        !isnothing(r) && return component_at(traj, first(r))
        need(field_of(I, name_fields...), what, kw)
    end
    part_of(P) = begin
        sname = component(P, (:unitary_components, :state_components, :ket_components), (:unitary_name, :state_name, :state_symb, :unitary_symb),
                          length(states) == 1 ? state_name : nothing, "the state component", "state_name")
        cname = component(P, (:drive_components, :control_components), (:control_name, :drive_name, :drive_symb),
                          control_name, "the control component", "control_name")
        expo = occursin("Exponential", type_name(P))
        ord = expo ? 0 : Int(need(isnothing(pade_order) ? field_of(P, :order) : pade_order, "the Padé order", "pade_order"))
        m = length(traj.components[cname])
        gens = begin
            sys = isnothing(system) ? field_of(P, :system, :sys) : system
            if !isnothing(sys)
                (sys.G_drift, collect(sys.G_drives))
            elseif !isnothing(field_of(P, :G_drift)) && !isnothing(field_of(P, :G_drives))
                (P.G_drift, collect(P.G_drives))
            else
                generators_from_closure(need(field_of(P, :G), "the generators (no `system`, `G_drift` / `G_drives` or `G` field)", "system"), m)
            end
        end
        (sname, cname, expo, ord, gens)
    end
    dpairs = if !isnothing(derivative_pairs)
        collect(derivative_pairs)
    else
        map(derivs) do D
            x = field_of(D, :variable_components); dx = field_of(D, :derivative_components)
            if !isnothing(x) && !isnothing(dx)
                (component_at(traj, first(x)), component_at(traj, first(dx)))
            else
                v = field_of(D, :variable, :variable_name, :x); dv = field_of(D, :derivative, :derivative_name, :dx)
                (isnothing(v) || isnothing(dv)) && error("QCollocHIP.QuantumDynamics: cannot read the components of $(type_name(D)); pass `derivative_pairs = [(:a, :da), ...]`")
                (Symbol(v), Symbol(dv))
            end
        end
    end
    any(I -> occursin("DensityOperator", type_name(I)), states) &&
        error("QCollocHIP.QuantumDynamics: density-operator integrators need the Lindblad generators: call `dynamics(...; n_kets = 1, generators = ...)`")
    kets_of(I) = occursin("QuantumState", type_name(I)) ? 1 : 0          # a QuantumState...Integrator propagates one ket (2N x 1 iso state)
    if length(states) == 1
        sname, cname, expo, ord, gens = part_of(states[1])
        return dynamics(integrators, traj, nothing; state_name=sname, control_name=cname, pade_order=expo ? 4 : ord, exponential=expo,
                        derivative_pairs=dpairs, generators=gens, n_kets=kets_of(states[1]), kwargs...)
    end
    # several state integrators: each with the derivative integrators that follow it in the list (the order QuantumDynamics stacks rows in)
    parts = []
    for (i, I) in enumerate(integrators)
        if is_state_integrator(I)
            sname, cname, expo, ord, gens = part_of(I)
            push!(parts, (system=(G_drift=gens[1], G_drives=gens[2], levels=size(gens[1], 1) ÷ 2), state_name=sname, control_name=cname,
                          derivative_pairs=Tuple{Symbol,Symbol}[], pade_order=expo ? 4 : ord, exponential=expo, n_kets=kets_of(I)))
        else
            isempty(parts) && error("QCollocHIP.QuantumDynamics: a DerivativeIntegrator comes before every state integrator of the list; " *
                                    "rows are stacked in list order behind the state integrator a derivative integrator follows " *
                                    "(unitary_smooth_pulse_problem.jl:175-179): put the Padé / exponential integrator first")
            k = count(is_derivative_integrator, integrators[1:i])
            push!(parts[end].derivative_pairs, dpairs[k])
        end
    end
    allowed = (:device, :devices, :eval_hessian, :padded, :result_ring)
    return dynamics_list(parts, traj; (k => v for (k, v) in kwargs if k in allowed)...)
end

"""
    dynamics_list(parts, traj; device=0, devices=nothing, eval_hessian=true, padded=false, result_ring=0)

The integrator lists with SEVERAL state integrators -- `UnitarySamplingProblem` ([U_1 .. U_K, D, D], shared controls:
unitary_sampling_problem.jl:134-155), `UnitaryDirectSumProblem` ([U_1, D, D, U_2, D, D, ...], own controls per member:
unitary_direct_sum_problem.jl:127-130), `QuantumStateSamplingProblem` (quantum_state_sampling_problem.jl:98-122) -- as ONE
`HIPDynamics` with the fields and call shapes of `dynamics`.  `parts` holds one named tuple per state integrator in list order,
each with the derivative integrators that FOLLOW it in the list:

    (system = sys, state_name = :Ũ⃗_system_1, control_name = :a, derivative_pairs = [], pade_order = 4, exponential = false, n_kets = 0)

(only `system` and `state_name` are required).  One composed handle per part; rows and values come out interval-major, in integrator
order inside an interval (the order `QuantumDynamics` stacks them in).  The evaluations go through `qc_eval_*_list`: one upload
of `Z⃗`, one batched launch where the parts' shapes allow it, results copied straight into the result vectors.
`devices = 0:7`: every part is created over the same device list (`qc_create_multi` on its composed descriptor), so shard s of every part
covers the same intervals on the same GPU, and the list is evaluated shard by shard -- each GPU lands its slice of the result vectors
over its own PCIe link (a K-system robust-control problem is the workload that wants eight GPUs).
"""
function dynamics_list(parts, traj; device::Int=0, devices=nothing, eval_hessian::Bool=true, padded::Bool=false, result_ring::Int=0)
    (result_ring == 0 || result_ring >= 3) || error("result_ring must be 0 (fresh vectors) or at least 3")
    length(parts) >= 1 || error("dynamics_list: no state integrators")
    devs = isnothing(devices) ? Int32[] : Int32.(collect(devices))
    isempty(devs) || (device = Int(devs[1]))
    off(name) = first(traj.components[name]) - 1
    free_time = traj.timestep isa Symbol
    opt(p, k, default) = haskey(p, k) ? p[k] : default
    keep = Any[]                                               # generator matrices the descriptors point at
    function desc_of(p, place)
        sys = p.system
        dpairs = opt(p, :derivative_pairs, [])
        expo = opt(p, :exponential, false)
        G0 = Matrix{Float64}(sys.G_drift)
        Gd = reduce(hcat, [vec(Matrix{Float64}(G)) for G in sys.G_drives])
        push!(keep, G0); push!(keep, Gd)
        xs = [off(q[1]) for q in dpairs]; dxs = [off(q[2]) for q in dpairs]; dms = [length(traj.components[q[1]]) for q in dpairs]
        return QCDesc(size(G0, 1) ÷ 2, length(sys.G_drives), traj.T, traj.dim, traj.global_dim,
                      off(p.state_name), off(opt(p, :control_name, :a)), free_time ? off(traj.timestep) : -1,
                      free_time ? 0.0 : Float64(traj.timestep),
                      expo ? 1 : 0, expo ? 0 : opt(p, :pade_order, 4), length(dpairs),
                      pad8(xs), pad8(dxs), pad8(dms), pointer(G0), pointer(Gd),
                      device, 0, 0, 0, opt(p, :n_kets, 0), 1,
                      place[1], place[2], place[3], place[4], place[5], place[6], 0, place[7], pad8(Int[]),
                      block_order(nothing, 5), block_order(nothing, 8))
    end
    # pass 1: every part's own sizes (no device work), hence its slot in the shared per-interval blocks
    own = QCDims[]
    for p in parts
        d = Ref{QCDims}()
        GC.@preserve keep check(ccall((:qc_desc_dims, LIB[]), Cint, (Ref{QCDesc}, Ref{QCDims}), Ref(desc_of(p, (0, 0, 0, 0, 0, 0, 0))), d))
        push!(own, d[])
    end
    rows = sum(x.ddim for x in own); jac = sum(x.jac_nnz_interval for x in own)
    with_hess = eval_hessian && all(x.hess_nnz_interval > 0 for x in own)
    hess_own = with_hess ? sum(x.hess_nnz_interval for x in own) : 0
    al = padded ? 16 : 1                                       # `padded`: the shared Hessian block is padded as a whole, through its last handle
    hess = cld(hess_own, al) * al
    handles = Ptr{Cvoid}[]
    ro = jo = ho = 0
    for (i, (p, x)) in enumerate(zip(parts, own))
        tail = (with_hess && i == length(parts)) ? hess - hess_own : 0
        h = Ref{Ptr{Cvoid}}(C_NULL)
        place = (rows, ro, jac, jo, with_hess ? hess : 0, with_hess ? ho : 0, tail)
        if isempty(devs)
            GC.@preserve keep check(ccall((:qc_create, LIB[]), Cint, (Ref{QCDesc}, Ref{Ptr{Cvoid}}), Ref(desc_of(p, place)), h))
        else
            GC.@preserve keep devs check(ccall((:qc_create_multi, LIB[]), Cint, (Ref{QCDesc}, Int32, Ptr{Int32}, Ref{Ptr{Cvoid}}),
                                               Ref(desc_of(p, place)), length(devs), devs, h))
        end
        push!(handles, h[])
        ro += x.ddim; jo += x.jac_nnz_interval; ho += x.hess_nnz_interval
    end
    h0 = handles[1]
    n_int = Int(own[1].n_intervals)
    F_len = rows * n_int; jac_nnz = jac * n_int; hess_nnz = hess * n_int
    # structures: every handle reports its own entries with the problem's row / column numbers; interleave them per interval
    function structure(hessian::Bool, per)
        rs = Matrix{Int64}[]; cs = Matrix{Int64}[]
        for (h, n) in zip(handles, per)
            r = Vector{Int64}(undef, n * n_int); c = similar(r)
            if hessian
                check(ccall((:qc_hess_structure, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Cint), h, r, c, 1), h)
            else
                check(ccall((:qc_jac_structure, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Cint), h, r, c, 1), h)
            end
            push!(rs, reshape(r, n, n_int)); push!(cs, reshape(c, n, n_int))
        end
        return collect(zip(Int.(vec(reduce(vcat, rs))), Int.(vec(reduce(vcat, cs)))))
    end
    ∂F_structure = structure(false, [Int(x.jac_nnz_interval) for x in own])
    nh = length(handles)
    F! = function (out::AbstractVector{Float64}, Z⃗::AbstractVector{Float64})
        length(out) == F_len || error("F!: output has length $(length(out)), expected $F_len")
        GC.@preserve Z⃗ out handles check(ccall((:qc_eval_F_list, LIB[]), Cint, (Ptr{Ptr{Cvoid}}, Int32, Ptr{Float64}, Ptr{Float64}), handles, nh, Z⃗, out), h0)
        return out
    end
    ∂F! = function (out::AbstractVector{Float64}, Z⃗::AbstractVector{Float64})
        length(out) == jac_nnz || error("∂F!: output has length $(length(out)), expected $jac_nnz")
        GC.@preserve Z⃗ out handles check(ccall((:qc_eval_jac_list, LIB[]), Cint, (Ptr{Ptr{Cvoid}}, Int32, Ptr{Float64}, Ptr{Float64}), handles, nh, Z⃗, out), h0)
        return out
    end
    pinned = PinnedOwner(Ptr{Cvoid}[])
    ringF = ResultRing(pinned, F_len, result_ring); ring∂F = ResultRing(pinned, jac_nnz, result_ring)
    F = (Z⃗; fresh::Bool=false) -> F!(next!(ringF, F_len, fresh), Z⃗)
    ∂F = (Z⃗; fresh::Bool=false) -> ∂F!(next!(ring∂F, jac_nnz, fresh), Z⃗)
    μ∂²F = nothing; μ∂²F! = nothing; μ∂²F_structure = nothing
    if with_hess
        per = [Int(x.hess_nnz_interval) for x in own]; per[end] += hess - hess_own
        μ∂²F_structure = structure(true, per)
        μ∂²F! = function (out::AbstractVector{Float64}, Z⃗::AbstractVector{Float64}, μ⃗::AbstractVector{Float64})
            length(out) == hess_nnz || error("μ∂²F!: output has length $(length(out)), expected $hess_nnz")
            length(μ⃗) == F_len || error("μ∂²F!: μ has length $(length(μ⃗)), expected $F_len")
            GC.@preserve Z⃗ μ⃗ out handles check(ccall((:qc_eval_hess_list, LIB[]), Cint,
                (Ptr{Ptr{Cvoid}}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), handles, nh, Z⃗, μ⃗, out), h0)
            return out
        end
        ringH = ResultRing(pinned, hess_nnz, result_ring)
        μ∂²F = (Z⃗, μ⃗; fresh::Bool=false) -> μ∂²F!(next!(ringH, hess_nnz, fresh), Z⃗, μ⃗)
    end
    d0 = own[1]
    d = QCDims(F_len, d0.n_cols, rows, jac, hess, n_int, F_len, jac_nnz, hess_nnz, d0.Z_len, d0.kernel, 0)
    dyn = HIPDynamics(h0, d, F, ∂F, ∂F_structure, μ∂²F, μ∂²F_structure, Int(rows), F!, ∂F!, μ∂²F!, handles, pinned)
    finalizer(release!, dyn)
    return dyn
end

"Ipopt's `new_x`: `false` declares that the next host-buffer calls receive the x of the previous one (`qc_set_new_x`)."
set_new_x!(dyn::HIPDynamics, new_x::Bool) = check(ccall((:qc_set_new_x, LIB[]), Cint, (Ptr{Cvoid}, Cint), dyn.handle, new_x ? 1 : 0), dyn.handle)

"""
Uploads of a trajectory vector this handle has done so far (`qc_knot_generation`).  An evaluator that elides uploads remembers it
after the call that put ITS x on the device and passes `new_x = false` only while it is unchanged -- any other call on the same
handle in between moves it -- and goes back to `set_new_x!(dyn, true)` right after the elided call.
"""
knot_generation(dyn::HIPDynamics) = ccall((:qc_knot_generation, LIB[]), Int64, (Ptr{Cvoid},), dyn.handle)

"""
Matrix-free Jacobian products (`qc_eval_jvp` / `qc_eval_vjp`): `dF_mul!(y, dyn, Z⃗, v)` writes `y = ∂F(Z⃗) v` (length `dyn.dims.F_len`),
`dFt_mul!(w, dyn, Z⃗, λ)` writes `w = ∂F(Z⃗)ᵀ λ` (length `dyn.dims.Z_len`, every entry written) -- the counterparts of MOI's
`eval_constraint_jacobian_product` / `eval_constraint_jacobian_transpose_product` for the dynamics rows, without the values of `∂F`.
Both honour `set_new_x!`.  One handle on one device (a `dynamics_list` goes through the library's `_dev_multi` entries instead).
"""
function dF_mul!(y::Vector{Float64}, dyn::HIPDynamics, Z⃗::Vector{Float64}, v::Vector{Float64})
    length(dyn.handles) == 1 || error("dF_mul!: one handle on one device only")
    length(y) == dyn.dims.F_len || error("dF_mul!: y has length $(length(y)), expected $(dyn.dims.F_len)")
    length(v) == dyn.dims.Z_len && length(Z⃗) == dyn.dims.Z_len || error("dF_mul!: Z⃗ and v must have length $(dyn.dims.Z_len)")
    GC.@preserve Z⃗ v y check(ccall((:qc_eval_jvp, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), dyn.handle, Z⃗, v, y), dyn.handle)
    return y
end
function dFt_mul!(w::Vector{Float64}, dyn::HIPDynamics, Z⃗::Vector{Float64}, λ::Vector{Float64})
    length(dyn.handles) == 1 || error("dFt_mul!: one handle on one device only")
    length(w) == dyn.dims.Z_len && length(Z⃗) == dyn.dims.Z_len || error("dFt_mul!: Z⃗ and w must have length $(dyn.dims.Z_len)")
    length(λ) == dyn.dims.F_len || error("dFt_mul!: λ has length $(length(λ)), expected $(dyn.dims.F_len)")
    GC.@preserve Z⃗ λ w check(ccall((:qc_eval_vjp, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), dyn.handle, Z⃗, λ, w), dyn.handle)
    return w
end

"""
Matrix-free product with the Hessian of the Lagrangian of the dynamics (`qc_eval_hvp`): `mu_d2F_mul!(w, dyn, Z⃗, μ, v)` writes
`w = H v` (length `dyn.dims.Z_len`, every entry written), `H` the full symmetric matrix whose upper triangle `mu_d2F` and
`mu_d2F_structure` describe (duplicates summed, a diagonal entry counted once) -- the dynamics' part of MOI's
`eval_hessian_lagrangian_product`, without the values of `μ∂²F`.  `μ` is what `mu_d2F` takes.  Honours `set_new_x!`.  One handle on one
device.
"""
function mu_d2F_mul!(w::Vector{Float64}, dyn::HIPDynamics, Z⃗::Vector{Float64}, μ::Vector{Float64}, v::Vector{Float64})
    length(dyn.handles) == 1 || error("mu_d2F_mul!: one handle on one device only")
    length(w) == dyn.dims.Z_len && length(v) == dyn.dims.Z_len && length(Z⃗) == dyn.dims.Z_len || error("mu_d2F_mul!: Z⃗, v and w must have length $(dyn.dims.Z_len)")
    length(μ) == dyn.dims.n_rows || error("mu_d2F_mul!: μ has length $(length(μ)), expected $(dyn.dims.n_rows)")
    GC.@preserve Z⃗ μ v w check(ccall((:qc_eval_hvp, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), dyn.handle, Z⃗, μ, v, w), dyn.handle)
    return w
end

# ---------------------------------------------------------------------------------------------------------------
#  Objective terms and rollouts (SURVEY.md 8f): the same `ccall` pattern over qc_terms_* / qc_fidelity_* / qc_rollout
# ---------------------------------------------------------------------------------------------------------------


# component entries (0-based) and one weight per entry of `[(name, R), ...]`, summed where components repeat
function entries_and_weights(traj, names_and_R)
    w = Dict{Int32, Float64}()
    for (name, r) in names_and_R
        comps = collect(traj.components[name]) .- 1
        for (k, j) in enumerate(comps)
            w[Int32(j)] = get(w, Int32(j), 0.0) + (r isa Number ? Float64(r) : Float64(r[k]))
        end
    end
    idx = sort!(collect(keys(w)))
    return idx, [w[j] for j in idx]
end

"""
    regularizers(traj, names_and_R; D=0.0, smooth=[], pairwise=[], linear=[], device=0, dt_scaled=true)

`names_and_R = [(:a, R_a), (:da, R_da), (:dda, R_dda)]` (scalars or vectors, unitary_smooth_pulse_problem.jl:151-153);
`D` adds `MinimumTimeObjective(traj; D)` (unitary_minimum_time_problem.jl:67-69).  The extension terms of the same pass
(qc_terms_ext): `smooth = [(:dda, R)]` is `QuadraticSmoothnessRegularizer` (unitary_smooth_pulse_problem.jl:311-340),
`pairwise = [((:dda1, :dda2), Q), ...]` one edge of `PairwiseQuadraticRegularizer(traj, Q, graph)`
(unitary_direct_sum_problem.jl:130-169), `linear = [(:s1_Ũ⃗, R), (:s2_Ũ⃗, R)]` the cost of `L1Regularizer!` on its slacks
(_problem_templates.jl:41-54).  Returns `(L, ∇L, ∂²L, ∂²L_structure)` closures over one device handle.
"""
function regularizers(traj, names_and_R; D::Float64=0.0, smooth=[], pairwise=[], linear=[], device::Int=0, dt_scaled::Bool=true)
    idx, R = entries_and_weights(traj, names_and_R)
    sidx, sR = entries_and_weights(traj, smooth)
    lidx, lw = entries_and_weights(traj, linear)
    pa = Int32[]; pb = Int32[]; pQ = Float64[]
    for ((A, B), q) in pairwise
        a = collect(traj.components[A]) .- 1; b = collect(traj.components[B]) .- 1
        length(a) == length(b) || error("pairwise edge ($A, $B): the components differ in length")
        append!(pa, Int32.(a)); append!(pb, Int32.(b)); append!(pQ, fill(Float64(q), length(a)))
    end
    free_time = traj.timestep isa Symbol
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve idx R sidx sR lidx lw pa pb pQ begin
        desc = Ref(QCTermsDesc(traj.T, traj.dim, free_time ? first(traj.components[traj.timestep]) - 1 : -1, traj.global_dim,
                               free_time ? 0.0 : Float64(traj.timestep), length(idx), dt_scaled ? 2 : 3,   # QC_REG_DT_SCALED = 2 (templates pass timestep_name=), QC_REG_PLAIN = 3 (docstring form); 0 / 1 are retired
                               pointer(idx), pointer(R), C_NULL, D, D == 0.0 ? 0 : traj.T - 1, device, 0))
        ext = Ref(QCTermsExt(length(sidx), length(pa), length(lidx), 0, pointer(sidx), pointer(sR), pointer(pa), pointer(pb), pointer(pQ),
                             pointer(lidx), pointer(lw), (0, 0)))
        rc = ccall((:qc_terms_create_ext, LIB[]), Cint, (Ref{QCTermsDesc}, Ref{QCTermsExt}, Ref{Ptr{Cvoid}}), desc, ext, h)
        rc == 0 || error("qc_terms_create_ext: " * unsafe_string(ccall((:qc_terms_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
    end
    nnz = Ref{Int64}(0)
    ccall((:qc_terms_hess_nnz, LIB[]), Cint, (Ptr{Cvoid}, Ref{Int64}), h[], nnz)
    hr = Vector{Int64}(undef, nnz[]); hc = similar(hr)
    ccall((:qc_terms_hess_structure, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Cint), h[], hr, hc, 1)
    Zlen = traj.dim * traj.T + traj.global_dim
    ev(Z⃗, J, g, H) = ccall((:qc_terms_eval, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h[], Z⃗, J, g, H)
    L(Z⃗) = (J = Ref(0.0); GC.@preserve Z⃗ ev(Z⃗, J, C_NULL, C_NULL); J[])
    ∇L(Z⃗) = (g = Vector{Float64}(undef, Zlen); GC.@preserve Z⃗ g ev(Z⃗, C_NULL, g, C_NULL); g)          # fresh vectors: results never alias
    ∂²L(Z⃗) = (H = Vector{Float64}(undef, nnz[]); GC.@preserve Z⃗ H ev(Z⃗, C_NULL, C_NULL, H); H)
    return L, ∇L, ∂²L, collect(zip(Int.(hr), Int.(hc)))
end

"""
    robustness_objective(traj, H_error; subspace=nothing, eval_hessian=true, device=0, unitary_name=:Ũ⃗, knots=traj.T)

`UnitaryRobustnessObjective(H_error=H_error, eval_hessian=eval_hessian)` (unitary_robustness_problem.jl:46-49) on the device:
L = Re tr(R'R)/n, R = (1/τ) Σ_{t≤knots} Δt_t V_t' H V_t over the subspace block V_t of every knot.  `H_error` is an N×N matrix
(its subspace block is used), an n×n matrix with `subspace`, or anything with `operator` and `subspace` fields (an
`EmbeddedOperator`); `subspace` is 1-based, as in Julia.  Returns `(L, ∇L, ∂²L, ∂²L_structure)` closures over one device handle:
∇L is dense over Z⃗, ∂²L the dense upper triangle over the term's variables (empty with `eval_hessian=false`).
"""
function robustness_objective(traj, H_error; subspace=nothing, eval_hessian::Bool=true, device::Int=0, unitary_name::Symbol=:Ũ⃗,
                              knots::Int=traj.T)
    if hasproperty(H_error, :operator) && hasproperty(H_error, :subspace)
        H, subspace = H_error.operator, H_error.subspace
    else
        H = H_error
    end
    N = isqrt(length(traj.components[unitary_name]) ÷ 2)
    if !isnothing(subspace) && size(H, 1) == N && length(subspace) < N
        H = H[collect(subspace), collect(subspace)]
    end
    sub = isnothing(subspace) ? Int32[] : Int32.(collect(subspace) .- 1)
    Hre = Float64.(vec(real.(H))); Him = Float64.(vec(imag.(H)))
    free_time = traj.timestep isa Symbol
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve sub Hre Him begin
        desc = Ref(QCRobustDesc(traj.T, traj.dim, first(traj.components[unitary_name]) - 1, N, length(sub),
                                isempty(sub) ? C_NULL : pointer(sub), pointer(Hre), pointer(Him),
                                free_time ? first(traj.components[traj.timestep]) - 1 : -1, 0, free_time ? 0.0 : Float64(traj.timestep),
                                traj.global_dim, knots, eval_hessian ? 1 : 0, device, (0, 0)))    # hessian: QC_ROBUST_HESS_EXACT = 1
        rc = ccall((:qc_robust_create, LIB[]), Cint, (Ref{QCRobustDesc}, Ref{Ptr{Cvoid}}), desc, h)
        rc == 0 || error("qc_robust_create: " * unsafe_string(ccall((:qc_robust_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
    end
    nnz = Ref{Int64}(0)
    ccall((:qc_robust_hess_nnz, LIB[]), Cint, (Ptr{Cvoid}, Ref{Int64}), h[], nnz)
    hr = Vector{Int64}(undef, nnz[]); hc = similar(hr)
    ccall((:qc_robust_hess_structure, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Cint), h[], hr, hc, 1)
    Zlen = traj.dim * traj.T + traj.global_dim
    ev(Z⃗, L, g, H) = ccall((:qc_robust_eval, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h[], Z⃗, L, g, H)
    L(Z⃗) = (l = Ref(0.0); GC.@preserve Z⃗ ev(Z⃗, l, C_NULL, C_NULL); l[])
    ∇L(Z⃗) = (g = Vector{Float64}(undef, Zlen); GC.@preserve Z⃗ g ev(Z⃗, C_NULL, g, C_NULL); g)
    ∂²L(Z⃗) = (H = Vector{Float64}(undef, nnz[]); GC.@preserve Z⃗ H ev(Z⃗, C_NULL, C_NULL, H); H)
    return L, ∇L, ∂²L, collect(zip(Int.(hr), Int.(hc)))
end

"""
    unitary_rollout(dyn::HIPDynamics, Z⃗, Ũ⃗_init)  ->  Ũ⃗ (2N² × T)

`unitary_rollout` / `rollout` / `open_rollout` (trajectory_initialization.jl:426,493,547) with the controls and timesteps of `Z⃗`.
"""
function unitary_rollout(dyn::HIPDynamics, Z⃗::AbstractVector{Float64}, init::AbstractVector{Float64}, T::Int)
    out = Matrix{Float64}(undef, length(init), T)
    GC.@preserve Z⃗ init out check(ccall((:qc_rollout, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                        dyn.handle, Z⃗, init, out), dyn.handle)
    return out
end

"""
    rollout_sweep(init, controls, Δt, G_drift, G_drives, G_pert, θ; scale=nothing, cols, goal=nothing, fid_kind=-1,
                  subspace=nothing, squared=false, device=0, wide=false, stored_states=false, wide64=false)  ->  (finals, fids)

Final states and fidelities of ONE trajectory of controls under S perturbed systems, in one call (`qc_sweep_eval`): the loop of the
reference's robustness check, `unitary_rollout(traj.a, timesteps, systems(ζ))[:, end]` and `iso_vec_unitary_fidelity` for every ζ
(unitary_sampling_problem.jl:233-243).  Sample s evolves under G_drift + Σ_j θ[s, j] G_pert[j] + Σ_k scale[s, k] a_k G_drives[k]
(2N×2N generators: `system.G_drift`, `system.G_drives`, and e.g. `G(Z)` for a detuning).  `controls` is m×T, `Δt` a vector of T
timesteps, `θ` S×p, `scale` S×m or nothing; `fid_kind` -1 (none), 0 (unitary; `subspace` 1-based, `squared`), 1 (ket), 2 (density
operator).  `wide = true` sets `qc_sweep_desc.wide = QC_SWEEP_WIDE`: the matrix-core form up to 2N = 32 ("mfma32-sweep") instead of one
rollout per sample from 2N = 18 up.  `wide64 = true` (only with `wide`) adds `QC_SWEEP_WIDE_64` (1024): 32 < 2N ≤ 64 with up to 16 drives
(5 qubits, three coupled three-level transmons) then runs on the matrix cores too ("mfma64-sweep"; the forward sweep only, so none of the
gradient functions below takes the keyword), and nothing changes at 2N ≤ 32.  `wide_stored = true` (only with `wide` and `stored_states`) adds `QC_SWEEP_WIDE_STORED` (8) to
`qc_sweep_desc.wide`: the stored-state walk then serves 16 < 2N ≤ 32 too (two qubits with T1 / T2), in `rollout_sweep_gradient`,
`rollout_sweep_parameter_gradient` and `rollout_sweep_pullback`.  `stored_states = true` sets `qc_sweep_desc.reserved1[1] = QC_SWEEP_STORED_STATES` (C index 0): reverse
mode (`rollout_sweep_gradient`, `rollout_sweep_parameter_gradient`, `rollout_sweep_pullback`) then reads stored forward states and serves
open systems with 2N ≤ 16 -- Lindblad generators with `fid_kind = 2`, non-Hermitian effective Hamiltonians; the forward sweep itself does
not look at it.  `finals` is (2N·cols)×S.  UNTESTED here, like the rest of this file.
"""
function rollout_sweep(init::AbstractVector{Float64}, controls::AbstractMatrix{Float64}, Δt::AbstractVector{Float64}, G_drift, G_drives, G_pert,
                       θ::AbstractMatrix{Float64}; scale=nothing, cols::Int, goal=nothing, fid_kind::Int=-1, subspace=nothing,
                       squared::Bool=false, device::Int=0, wide::Bool=false, stored_states::Bool=false, wide_stored::Bool=false,
                       wide64::Bool=false)
    (wide64 && !wide) && error("rollout_sweep: wide64 = true needs wide = true")
    n = size(G_drift, 1); N = n ÷ 2
    m, T = size(controls); p = length(G_pert); S = size(θ, 1)
    G0 = Float64.(vec(G_drift))
    Gd = m == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_drives])
    Gp = p == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_pert])
    sub = isnothing(subspace) ? Int32[] : Int32.(collect(subspace) .- 1)
    g = isnothing(goal) ? Float64[] : Float64.(collect(goal))
    Z⃗ = vec(vcat(controls, reshape(Δt, 1, T)))                      # knot layout [a; Δt]
    θt = Matrix{Float64}(transpose(θ))                               # sample-major
    ct = isnothing(scale) ? Float64[] : vec(Matrix{Float64}(transpose(scale)))
    finals = Matrix{Float64}(undef, n * cols, S)
    fids = fid_kind >= 0 ? Vector{Float64}(undef, S) : Float64[]
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve G0 Gd Gp sub g begin
        desc = Ref(QCSweepDesc(T, m + 1, 0, m, N, 0.0, 0, m, cols == N ? 0 : cols, p, fid_kind,
                               pointer(G0), m == 0 ? C_NULL : pointer(Gd), p == 0 ? C_NULL : pointer(Gp),
                               squared ? 1 : 0, length(sub), isempty(g) ? C_NULL : pointer(g), isempty(sub) ? C_NULL : pointer(sub),
                               device, (wide ? 1 : 0) | (wide_stored ? 8 : 0) | (wide64 ? QC_SWEEP_WIDE_64 : 0), (stored_states ? 1 : 0, 0)))      # 8 = QC_SWEEP_WIDE_STORED
        rc = ccall((:qc_sweep_create, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Ptr{Cvoid}}), desc, h)
        rc == 0 || error("qc_sweep_create: " * unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
    end
    rc = GC.@preserve Z⃗ init θt ct finals fids ccall((:qc_sweep_eval, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        h[], Z⃗, init, S, p == 0 ? C_NULL : pointer(θt), isempty(ct) ? C_NULL : pointer(ct), finals, fid_kind >= 0 ? pointer(fids) : C_NULL)
    msg = rc == 0 ? "" : unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), h[]))
    ccall((:qc_sweep_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), h[])
    rc == 0 || error("qc_sweep_eval: " * msg)
    return finals, fids
end

"""
    rollout_sweep_gradient(init, controls, Δt, G_drift, G_drives, G_pert, θ; scale=nothing, weights=nothing, cols, goal, fid_kind=0,
                           subspace=nothing, squared=false, per_sample=false, device=0, wide=false, stored_states=false,
                           wide64=false, wide64_grad=false, wide64_stored=false)  ->  (J, fids, ∇a, ∇Δt[, grad_samples])

The adjoint of `rollout_sweep` (`qc_sweep_grad`): J = Σ_s w_s F_s (`weights`: S values, default 1/S each), the S fidelities, and the
gradient of J with respect to the controls (`∇a`, m×T) and the timesteps (`∇Δt`, T); the last knot's columns are zero.  With
`per_sample`, `grad_samples` is (m+1)×(T-1)×S: ∂F_s/∂a_{t,k}, then ∂F_s/∂Δt_t.  Served for closed systems (antisymmetric generators)
with 2N ≤ 16 (`wide = true`: 2N ≤ 32), m ≤ 8 and `fid_kind` 0 (unitary) or 1 (ket); with `stored_states = true` for ANY generators with 2N ≤ 16,
m ≤ 8 and `fid_kind` 0, 1 or 2 (density operator); everything else errors with the library's reason.  `wide = true, wide64 = true,
wide64_grad = true` sets `QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD` (3073): closed systems with 32 < 2N ≤ 64, m ≤ 16 and at
most 32 state columns in the "mfma64-sweep" form.  `wide64_stored = true` (only with `wide64_grad` and `stored_states`) adds
`QC_SWEEP_WIDE_64_STORED` (262144): ANY generators there, `fid_kind` 2 included (a five-level Lindblad model, 2N = 50), by the stored-state
walk.  Arguments as `rollout_sweep`.  UNTESTED here, like the rest of this file.
"""
function rollout_sweep_gradient(init::AbstractVector{Float64}, controls::AbstractMatrix{Float64}, Δt::AbstractVector{Float64}, G_drift, G_drives,
                                G_pert, θ::AbstractMatrix{Float64}; scale=nothing, weights=nothing, cols::Int, goal, fid_kind::Int=0,
                                subspace=nothing, squared::Bool=false, per_sample::Bool=false, device::Int=0, wide::Bool=false, stored_states::Bool=false, wide_stored::Bool=false,
                                wide64::Bool=false, wide64_grad::Bool=false, wide64_stored::Bool=false)
    (wide64_stored && !(wide64_grad && stored_states)) && error("rollout_sweep_gradient: wide64_stored = true needs wide64_grad = true and stored_states = true")
    (wide64 && !wide) && error("rollout_sweep_gradient: wide64 = true needs wide = true")
    (wide64_grad && !wide64) && error("rollout_sweep_gradient: wide64_grad = true needs wide64 = true")
    n = size(G_drift, 1); N = n ÷ 2
    m, T = size(controls); p = length(G_pert); S = size(θ, 1)
    G0 = Float64.(vec(G_drift))
    Gd = m == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_drives])
    Gp = p == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_pert])
    sub = isnothing(subspace) ? Int32[] : Int32.(collect(subspace) .- 1)
    g = Float64.(collect(goal))
    Z⃗ = vec(vcat(controls, reshape(Δt, 1, T)))                      # knot layout [a; Δt]
    θt = Matrix{Float64}(transpose(θ))                               # sample-major
    ct = isnothing(scale) ? Float64[] : vec(Matrix{Float64}(transpose(scale)))
    w = isnothing(weights) ? Float64[] : Float64.(collect(weights))
    fids = Vector{Float64}(undef, S)
    J = Ref(0.0)
    grad = Vector{Float64}(undef, (m + 1) * T)
    gs = per_sample ? Array{Float64}(undef, m + 1, T - 1, S) : Array{Float64}(undef, 0, 0, 0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve G0 Gd Gp sub g begin
        desc = Ref(QCSweepDesc(T, m + 1, 0, m, N, 0.0, 0, m, cols == N ? 0 : cols, p, fid_kind,
                               pointer(G0), m == 0 ? C_NULL : pointer(Gd), p == 0 ? C_NULL : pointer(Gp),
                               squared ? 1 : 0, length(sub), pointer(g), isempty(sub) ? C_NULL : pointer(sub),
                               device, (wide ? 1 : 0) | (wide_stored ? 8 : 0) | (wide64 ? QC_SWEEP_WIDE_64 : 0) | (wide64_grad ? QC_SWEEP_WIDE_64_GRAD : 0) |
                               (wide64_stored ? QC_SWEEP_WIDE_64_STORED : 0),
                               (stored_states ? 1 : 0, 0)))      # 8 = QC_SWEEP_WIDE_STORED
        ok = Ref{Int32}(0)
        rc = ccall((:qc_sweep_desc_grad_supported, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Int32}), desc, ok)
        (rc == 0 && ok[] == 1) || error(unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
        rc = ccall((:qc_sweep_create, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Ptr{Cvoid}}), desc, h)
        rc == 0 || error("qc_sweep_create: " * unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
    end
    rc = GC.@preserve Z⃗ init θt ct w fids grad gs ccall((:qc_sweep_grad, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}, Ptr{Float64},
         Ptr{Float64}),
        h[], Z⃗, init, S, p == 0 ? C_NULL : pointer(θt), isempty(ct) ? C_NULL : pointer(ct), isempty(w) ? C_NULL : pointer(w), fids, J, grad,
        per_sample ? pointer(gs) : C_NULL)
    msg = rc == 0 ? "" : unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), h[]))
    ccall((:qc_sweep_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), h[])
    rc == 0 || error("qc_sweep_grad: " * msg)
    G = reshape(grad, m + 1, T)
    return per_sample ? (J[], fids, G[1:m, :], G[m + 1, :], gs) : (J[], fids, G[1:m, :], G[m + 1, :])
end

"""
    rollout_noise_sweep(init, controls, Δt, G_drift, G_drives, G_pert, ξ; θ=nothing, scale=nothing, cols, goal=nothing, fid_kind=-1,
                        subspace=nothing, squared=false, device=0, wide=false, wide64=false)  ->  (finals, fids)

`rollout_sweep` with perturbation amplitudes that change from interval to interval (`qc_sweep_noise_eval`): in interval t sample s
evolves under G_drift + Σ_j (θ[s, j] + ξ[j, t, s]) G_pert[j] + Σ_k scale[s, k] a_{t,k} G_drives[k].  `ξ` is p×(T-1)×S (the library's
sample-major layout as a column-major array), `θ` S×p or nothing (zeros).  Served for 2N ≤ 16 with p ≥ 1 and m + p ≤ 8; `wide = true` sets
`qc_sweep_desc.wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_NOISE` (65): 16 < 2N ≤ 32 on the matrix cores with p ≥ 1, m ≤ 8 and no limit on
m + p.  `wide64 = true` (only with `wide`) adds `QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_NOISE` (66625 in all): 32 < 2N ≤ 64 with p ≥ 1 and m ≤ 16
in the "mfma64-sweep" form, any generators.  Everything else errors with the library's reason.  Other arguments as `rollout_sweep`.
UNTESTED here, like the rest of this file: the `wide64` path was not run.
"""
function rollout_noise_sweep(init::AbstractVector{Float64}, controls::AbstractMatrix{Float64}, Δt::AbstractVector{Float64}, G_drift, G_drives,
                             G_pert, ξ::AbstractArray{Float64,3}; θ=nothing, scale=nothing, cols::Int, goal=nothing, fid_kind::Int=-1,
                             subspace=nothing, squared::Bool=false, device::Int=0, wide::Bool=false, wide64::Bool=false)
    (!wide64 || wide) || error("rollout_noise_sweep: wide64 = true needs wide = true")
    n = size(G_drift, 1); N = n ÷ 2
    m, T = size(controls); p = length(G_pert); S = size(ξ, 3)
    size(ξ) == (p, T - 1, S) || error("rollout_noise_sweep: ξ must be $p×$(T - 1)×S")
    G0 = Float64.(vec(G_drift))
    Gd = m == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_drives])
    Gp = p == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_pert])
    sub = isnothing(subspace) ? Int32[] : Int32.(collect(subspace) .- 1)
    g = isnothing(goal) ? Float64[] : Float64.(collect(goal))
    Z⃗ = vec(vcat(controls, reshape(Δt, 1, T)))                      # knot layout [a; Δt]
    θt = isnothing(θ) ? zeros(p, S) : Matrix{Float64}(transpose(θ))  # sample-major
    ct = isnothing(scale) ? Float64[] : vec(Matrix{Float64}(transpose(scale)))
    ξv = Array{Float64}(ξ)
    finals = Matrix{Float64}(undef, n * cols, S)
    fids = fid_kind >= 0 ? Vector{Float64}(undef, S) : Float64[]
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve G0 Gd Gp sub g begin
        desc = Ref(QCSweepDesc(T, m + 1, 0, m, N, 0.0, 0, m, cols == N ? 0 : cols, p, fid_kind,
                               pointer(G0), m == 0 ? C_NULL : pointer(Gd), p == 0 ? C_NULL : pointer(Gp),
                               squared ? 1 : 0, length(sub), isempty(g) ? C_NULL : pointer(g), isempty(sub) ? C_NULL : pointer(sub),
                               device, (wide ? (QC_SWEEP_WIDE | QC_SWEEP_WIDE_NOISE) : 0) | (wide64 ? (QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_NOISE) : 0), (0, 0)))
        ok = Ref{Int32}(0)
        rc = ccall((:qc_sweep_desc_noise_supported, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Int32}), desc, ok)
        (rc == 0 && ok[] == 1) || error(unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
        rc = ccall((:qc_sweep_create, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Ptr{Cvoid}}), desc, h)
        rc == 0 || error("qc_sweep_create: " * unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
    end
    rc = GC.@preserve Z⃗ init θt ct ξv finals fids ccall((:qc_sweep_noise_eval, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        h[], Z⃗, init, S, θt, isempty(ct) ? C_NULL : pointer(ct), ξv, finals, fid_kind >= 0 ? pointer(fids) : C_NULL)
    msg = rc == 0 ? "" : unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), h[]))
    ccall((:qc_sweep_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), h[])
    rc == 0 || error("qc_sweep_noise_eval: " * msg)
    return finals, fids
end

"""
    rollout_noise_sweep_gradient(init, controls, Δt, G_drift, G_drives, G_pert, ξ; θ=nothing, scale=nothing, weights=nothing, cols, goal,
                                 fid_kind=0, subspace=nothing, squared=false, device=0, wide=false, wide64=false)  ->  (J, fids, ∇a, ∇Δt, ∇ξ)

The adjoint of `rollout_noise_sweep` (`qc_sweep_noise_grad`): J, the S fidelities and the gradient of J over the controls and timesteps
as `rollout_sweep_gradient` returns them, and `∇ξ[j, t, s]` = ∂F_s/∂ξ[j, t, s] (p×(T-1)×S, raw per-sample values): the time-resolved noise
sensitivity of every sample.  Closed systems, `fid_kind` 0 (unitary) or 1 (ket), 2N ≤ 16, p ≥ 1, m + p ≤ 8; `wide = true` sets
`qc_sweep_desc.wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_NOISE` (65): 16 < 2N ≤ 32 with p ≥ 1, m ≤ 8, no limit on m + p.  `wide64 = true` (only
with `wide`) adds `QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_NOISE` (68673 in all): closed systems with 32 < 2N ≤ 64, p ≥ 1,
m ≤ 16 and at most 32 state columns in the "mfma64-sweep" form.  UNTESTED here, like the rest of this file: the `wide64` path was not run.
"""
function rollout_noise_sweep_gradient(init::AbstractVector{Float64}, controls::AbstractMatrix{Float64}, Δt::AbstractVector{Float64}, G_drift,
                                      G_drives, G_pert, ξ::AbstractArray{Float64,3}; θ=nothing, scale=nothing, weights=nothing, cols::Int,
                                      goal, fid_kind::Int=0, subspace=nothing, squared::Bool=false, device::Int=0, wide::Bool=false,
                                      wide64::Bool=false)
    (!wide64 || wide) || error("rollout_noise_sweep_gradient: wide64 = true needs wide = true")
    n = size(G_drift, 1); N = n ÷ 2
    m, T = size(controls); p = length(G_pert); S = size(ξ, 3)
    size(ξ) == (p, T - 1, S) || error("rollout_noise_sweep_gradient: ξ must be $p×$(T - 1)×S")
    G0 = Float64.(vec(G_drift))
    Gd = m == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_drives])
    Gp = p == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_pert])
    sub = isnothing(subspace) ? Int32[] : Int32.(collect(subspace) .- 1)
    g = Float64.(collect(goal))
    Z⃗ = vec(vcat(controls, reshape(Δt, 1, T)))                      # knot layout [a; Δt]
    θt = isnothing(θ) ? zeros(p, S) : Matrix{Float64}(transpose(θ))  # sample-major
    ct = isnothing(scale) ? Float64[] : vec(Matrix{Float64}(transpose(scale)))
    w = isnothing(weights) ? Float64[] : Float64.(collect(weights))
    ξv = Array{Float64}(ξ)
    fids = Vector{Float64}(undef, S)
    J = Ref(0.0)
    grad = Vector{Float64}(undef, (m + 1) * T)
    ∇ξ = Array{Float64}(undef, p, T - 1, S)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve G0 Gd Gp sub g begin
        desc = Ref(QCSweepDesc(T, m + 1, 0, m, N, 0.0, 0, m, cols == N ? 0 : cols, p, fid_kind,
                               pointer(G0), m == 0 ? C_NULL : pointer(Gd), p == 0 ? C_NULL : pointer(Gp),
                               squared ? 1 : 0, length(sub), pointer(g), isempty(sub) ? C_NULL : pointer(sub),
                               device, (wide ? (QC_SWEEP_WIDE | QC_SWEEP_WIDE_NOISE) : 0) |
                               (wide64 ? (QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_NOISE) : 0), (0, 0)))
        rc = ccall((:qc_sweep_create, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Ptr{Cvoid}}), desc, h)
        rc == 0 || error("qc_sweep_create: " * unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
    end
    rc = GC.@preserve Z⃗ init θt ct ξv w fids grad ∇ξ ccall((:qc_sweep_noise_grad, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        h[], Z⃗, init, S, θt, isempty(ct) ? C_NULL : pointer(ct), ξv, isempty(w) ? C_NULL : pointer(w), fids, J, grad, C_NULL, ∇ξ)
    msg = rc == 0 ? "" : unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), h[]))      # out of scope: the library's reason
    ccall((:qc_sweep_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), h[])
    rc == 0 || error("qc_sweep_noise_grad: " * msg)
    G = reshape(grad, m + 1, T)
    return J[], fids, G[1:m, :], G[m + 1, :], ∇ξ
end

"""
    rollout_sweep_parameter_gradient(init, controls, Δt, G_drift, G_drives, G_pert, θ; scale=nothing, cols, goal, fid_kind=0,
                                     subspace=nothing, squared=false, device=0, stored_states=false, wide=false, wide64_stored=false, wide64_params=false)  ->  (fids, ∇θ, ∇c)

The derivatives of the S fidelities of `rollout_sweep` with respect to the SYSTEMS (`qc_sweep_grad_params`): `∇θ[s, j]` = ∂F_s/∂θ[s, j]
(S×p) and `∇c[s, k]` = ∂F_s/∂scale[s, k] (S×m; `scale = nothing`: taken at all ones), raw per-sample values from one backward walk.
Scope and arguments as `rollout_sweep_gradient` (`stored_states = true`: open systems, as there).  `wide = true` sets
`qc_sweep_desc.wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_PARAMS` (3): 2N ≤ 32 on the matrix cores, parameter gradients included.
`wide64_params = true` (only with `wide`) adds `QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_PARAMS` (11267 in all): closed
systems with 32 < 2N ≤ 64, m ≤ 16 and at most 32 state columns in the "mfma64-sweep" form, parameter gradients included;
`wide64_stored = true` (only with `wide64_params` and `stored_states`) adds `QC_SWEEP_WIDE_64_STORED` (262144): any generators there.
UNTESTED here, like the rest of this file: no Julia runs where this library is built and tested.
"""
function rollout_sweep_parameter_gradient(init::AbstractVector{Float64}, controls::AbstractMatrix{Float64}, Δt::AbstractVector{Float64}, G_drift,
                                          G_drives, G_pert, θ::AbstractMatrix{Float64}; scale=nothing, cols::Int, goal, fid_kind::Int=0,
                                          subspace=nothing, squared::Bool=false, device::Int=0, stored_states::Bool=false, wide_stored::Bool=false, wide::Bool=false,
                                          wide64_stored::Bool=false, wide64_params::Bool=false)
    (wide64_stored && !(wide64_params && stored_states)) && error("rollout_sweep_parameter_gradient: wide64_stored = true needs wide64_params = true and stored_states = true")
    (wide64_params && !wide) && error("rollout_sweep_parameter_gradient: wide64_params = true needs wide = true")
    n = size(G_drift, 1); N = n ÷ 2
    m, T = size(controls); p = length(G_pert); S = size(θ, 1)
    G0 = Float64.(vec(G_drift))
    Gd = m == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_drives])
    Gp = p == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_pert])
    sub = isnothing(subspace) ? Int32[] : Int32.(collect(subspace) .- 1)
    g = Float64.(collect(goal))
    Z⃗ = vec(vcat(controls, reshape(Δt, 1, T)))                      # knot layout [a; Δt]
    θt = Matrix{Float64}(transpose(θ))                               # sample-major
    ct = isnothing(scale) ? Float64[] : vec(Matrix{Float64}(transpose(scale)))
    fids = Vector{Float64}(undef, S)
    gθ = Matrix{Float64}(undef, p, S)                                # sample-major: column s holds sample s
    gc = Matrix{Float64}(undef, m, S)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve G0 Gd Gp sub g begin
        desc = Ref(QCSweepDesc(T, m + 1, 0, m, N, 0.0, 0, m, cols == N ? 0 : cols, p, fid_kind,
                               pointer(G0), m == 0 ? C_NULL : pointer(Gd), p == 0 ? C_NULL : pointer(Gp),
                               squared ? 1 : 0, length(sub), pointer(g), isempty(sub) ? C_NULL : pointer(sub),
                               device, (wide ? 3 : 0) | (wide_stored ? 8 : 0) | (wide64_params ? (QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_PARAMS) : 0) |
                               (wide64_stored ? QC_SWEEP_WIDE_64_STORED : 0),
                               (stored_states ? 1 : 0, 0)))      # 3 = QC_SWEEP_WIDE | QC_SWEEP_WIDE_PARAMS, 8 = QC_SWEEP_WIDE_STORED
        ok = Ref{Int32}(0)
        rc = ccall((:qc_sweep_desc_grad_supported, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Int32}), desc, ok)
        (rc == 0 && ok[] == 1) || error(unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
        rc = ccall((:qc_sweep_create, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Ptr{Cvoid}}), desc, h)
        rc == 0 || error("qc_sweep_create: " * unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
    end
    rc = GC.@preserve Z⃗ init θt ct fids gθ gc ccall((:qc_sweep_grad_params, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        h[], Z⃗, init, S, p == 0 ? C_NULL : pointer(θt), isempty(ct) ? C_NULL : pointer(ct), C_NULL, fids, C_NULL, C_NULL, C_NULL,
        p == 0 ? C_NULL : pointer(gθ), m == 0 ? C_NULL : pointer(gc))
    msg = rc == 0 ? "" : unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), h[]))
    ccall((:qc_sweep_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), h[])
    rc == 0 || error("qc_sweep_grad_params: " * msg)
    return fids, Matrix{Float64}(transpose(gθ)), Matrix{Float64}(transpose(gc))
end

"""
    rollout_sweep_pullback(init, controls, Δt, G_drift, G_drives, G_pert, θ, C̄; scale=nothing, cols, params=false, device=0,
                           wide=false, stored_states=false, wide_params=false, wide64=false, wide64_grad=false, wide64_stored=false, wide64_params=false)  ->  (finals, ∇a, ∇Δt, ∇init[, ∇θ, ∇c])

The pullback of `rollout_sweep` (`qc_sweep_vjp`): `C̄` is (2N·cols)×S, column s the cotangent of sample s's final state (the derivative
of the caller's loss with respect to it, e.g. what `Zygote.pullback` hands to an `rrule`), and with φ_s = ⟨C̄[:, s], finals[:, s]⟩ the
results are the final states themselves, Σ_s ∂φ_s/∂a (m×T) and Σ_s ∂φ_s/∂Δt (T; the last knot's columns are zero), `∇init`
(2N·cols)×S with column s = ∂φ_s/∂init (sum the columns for a shared initial state) and, with `params`, `∇θ` (S×p) and `∇c` (S×m).
Served for closed systems (antisymmetric generators) with 2N ≤ 16 (`wide = true`: 2N ≤ 32, there with `params` only if also `wide_params = true`, which sets bit 1 of
`qc_sweep_desc.wide`, QC_SWEEP_WIDE_PARAMS), m ≤ 8 and at most 16
state columns, with `stored_states = true` for any generators with 2N ≤ 16; no fidelity is involved.  `wide = true, wide64 = true,
wide64_grad = true` (3073 in `qc_sweep_desc.wide`): closed systems with 32 < 2N ≤ 64, m ≤ 16 and at most 32 state columns in the
"mfma64-sweep" form, there with `params` only if also `wide64_params = true` (bit 13, QC_SWEEP_WIDE_64_PARAMS: 11265); `wide64_stored = true` (only with `wide64_grad` and `stored_states`; bit 18,
QC_SWEEP_WIDE_64_STORED) serves any generators there by the stored-state walk.  Arguments as
`rollout_sweep`.  UNTESTED here, like the rest of this file: no Julia runs where this library is built and tested.
"""
function rollout_sweep_pullback(init::AbstractVector{Float64}, controls::AbstractMatrix{Float64}, Δt::AbstractVector{Float64}, G_drift, G_drives,
                                G_pert, θ::AbstractMatrix{Float64}, C̄::AbstractMatrix{Float64}; scale=nothing, cols::Int, params::Bool=false,
                                device::Int=0, wide::Bool=false, stored_states::Bool=false, wide_stored::Bool=false, wide_params::Bool=false,
                                wide64::Bool=false, wide64_grad::Bool=false, wide64_stored::Bool=false, wide64_params::Bool=false)
    (wide64_stored && !(wide64_grad && stored_states)) && error("rollout_sweep_pullback: wide64_stored = true needs wide64_grad = true and stored_states = true")
    (wide64_params && !wide64_grad) && error("rollout_sweep_pullback: wide64_params = true needs wide64_grad = true")
    (wide_params && !wide) && error("rollout_sweep_pullback: wide_params = true needs wide = true")
    (wide64 && !wide) && error("rollout_sweep_pullback: wide64 = true needs wide = true")
    (wide64_grad && !wide64) && error("rollout_sweep_pullback: wide64_grad = true needs wide64 = true")
    n = size(G_drift, 1); N = n ÷ 2
    m, T = size(controls); p = length(G_pert); S = size(θ, 1)
    size(C̄) == (n * cols, S) || error("rollout_sweep_pullback: C̄ must be $(n * cols)×$S")
    G0 = Float64.(vec(G_drift))
    Gd = m == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_drives])
    Gp = p == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_pert])
    Z⃗ = vec(vcat(controls, reshape(Δt, 1, T)))                      # knot layout [a; Δt]
    θt = Matrix{Float64}(transpose(θ))                               # sample-major
    ct = isnothing(scale) ? Float64[] : vec(Matrix{Float64}(transpose(scale)))
    cot = Matrix{Float64}(C̄)                                         # column s holds sample s: sample-major as it stands
    finals = Matrix{Float64}(undef, n * cols, S)
    grad = Vector{Float64}(undef, (m + 1) * T)
    ginit = Matrix{Float64}(undef, n * cols, S)
    gθ = Matrix{Float64}(undef, p, S)                                # sample-major: column s holds sample s
    gc = Matrix{Float64}(undef, m, S)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve G0 Gd Gp begin
        desc = Ref(QCSweepDesc(T, m + 1, 0, m, N, 0.0, 0, m, cols == N ? 0 : cols, p, -1,
                               pointer(G0), m == 0 ? C_NULL : pointer(Gd), p == 0 ? C_NULL : pointer(Gp),
                               0, 0, C_NULL, C_NULL, device, (wide ? 1 : 0) | (wide_params ? 2 : 0) | (wide_stored ? 8 : 0) | (wide64 ? QC_SWEEP_WIDE_64 : 0) | (wide64_grad ? QC_SWEEP_WIDE_64_GRAD : 0) | (wide64_params ? QC_SWEEP_WIDE_64_PARAMS : 0) |
                               (wide64_stored ? QC_SWEEP_WIDE_64_STORED : 0),
                               (stored_states ? 1 : 0, 0)))
        ok = Ref{Int32}(0)
        rc = ccall((:qc_sweep_desc_vjp_supported, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Int32}), desc, ok)
        (rc == 0 && ok[] == 1) || error(unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
        rc = ccall((:qc_sweep_create, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Ptr{Cvoid}}), desc, h)
        rc == 0 || error("qc_sweep_create: " * unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
    end
    rc = GC.@preserve Z⃗ init θt ct cot finals grad ginit gθ gc ccall((:qc_sweep_vjp, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        h[], Z⃗, init, S, p == 0 ? C_NULL : pointer(θt), isempty(ct) ? C_NULL : pointer(ct), cot, finals, grad, C_NULL, ginit,
        (params && p > 0) ? pointer(gθ) : C_NULL, (params && m > 0) ? pointer(gc) : C_NULL)
    msg = rc == 0 ? "" : unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), h[]))
    ccall((:qc_sweep_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), h[])
    rc == 0 || error("qc_sweep_vjp: " * msg)
    G = reshape(grad, m + 1, T)
    return params ? (finals, G[1:m, :], G[m + 1, :], ginit, Matrix{Float64}(transpose(gθ)), Matrix{Float64}(transpose(gc))) :
                    (finals, G[1:m, :], G[m + 1, :], ginit)
end

"""
    rollout_sweep_pushforward(init, controls, Δt, G_drift, G_drives, G_pert, θ; scale=nothing, cols, vZ=nothing, vinit=nothing,
                              vtheta=nothing, vscale=nothing, device=0, wide=false, wide64=false, wide64_tangent=false)  ->  (finals, tfinals)

The pushforward of `rollout_sweep` (`qc_sweep_jvp`): the final states, (2N·cols)×S, and their tangents along one direction, the same
shape.  `vZ` is an (m+1)×T matrix in the knot layout [a; Δt] (only the columns of knots 1 … T−1 act), `vinit` a 2N·cols vector, `vtheta`
S×p and `vscale` S×m (valid with `scale = nothing`: taken at all ones); whichever is `nothing` is zero, at least one must be given.
Served with 2N ≤ 16 and m ≤ 8 for ANY generators, Lindblad ones included (nothing is reversed); no fidelity is involved.  `wide = true`
sets `qc_sweep_desc.wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_TANGENT` (17): the matrix-core form up to 2N = 32 ("mfma32-sweep") with its
pushforward, e.g. two coupled three-level transmons or two qubits with T1 / T2.  `wide = true, wide64 = true, wide64_tangent = true` adds
`QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_TANGENT` (17425 in all): 32 < 2N ≤ 64 with m ≤ 16 in the "mfma64-sweep" form with its pushforward,
any generators again (5 qubits, three coupled three-level transmons, a five-level Lindblad model), states of 2N·cols ≤ 2048 entries.
Arguments as `rollout_sweep`.  UNTESTED here, like the rest of this file: the `wide64_tangent` path was not run.
"""
function rollout_sweep_pushforward(init::AbstractVector{Float64}, controls::AbstractMatrix{Float64}, Δt::AbstractVector{Float64}, G_drift,
                                   G_drives, G_pert, θ::AbstractMatrix{Float64}; scale=nothing, cols::Int, vZ=nothing, vinit=nothing,
                                   vtheta=nothing, vscale=nothing, device::Int=0, wide::Bool=false, wide64::Bool=false,
                                   wide64_tangent::Bool=false)
    (wide64 && !wide) && error("rollout_sweep_pushforward: wide64 = true needs wide = true")
    (wide64_tangent && !wide64) && error("rollout_sweep_pushforward: wide64_tangent = true needs wide64 = true")
    n = size(G_drift, 1); N = n ÷ 2
    m, T = size(controls); p = length(G_pert); S = size(θ, 1)
    G0 = Float64.(vec(G_drift))
    Gd = m == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_drives])
    Gp = p == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_pert])
    Z⃗ = vec(vcat(controls, reshape(Δt, 1, T)))                      # knot layout [a; Δt]
    θt = Matrix{Float64}(transpose(θ))                               # sample-major
    ct = isnothing(scale) ? Float64[] : vec(Matrix{Float64}(transpose(scale)))
    vz = isnothing(vZ) ? Float64[] : Float64.(vec(vZ))
    vi = isnothing(vinit) ? Float64[] : Float64.(vec(vinit))
    (isnothing(vtheta) || size(vtheta) == (S, p)) || error("rollout_sweep_pushforward: vtheta must be $S×$p")
    (isnothing(vscale) || size(vscale) == (S, m)) || error("rollout_sweep_pushforward: vscale must be $S×$m")
    (isnothing(scale) || size(scale) == (S, m)) || error("rollout_sweep_pushforward: scale must be $S×$m")
    vθ = isnothing(vtheta) ? Float64[] : vec(Matrix{Float64}(transpose(vtheta)))
    vc = isnothing(vscale) ? Float64[] : vec(Matrix{Float64}(transpose(vscale)))
    (isempty(vz) || length(vz) == (m + 1) * T) || error("rollout_sweep_pushforward: vZ must be $(m + 1)×$T")
    (isempty(vi) || length(vi) == n * cols) || error("rollout_sweep_pushforward: vinit must have $(n * cols) entries")
    finals = Matrix{Float64}(undef, n * cols, S)
    tfinals = Matrix{Float64}(undef, n * cols, S)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve G0 Gd Gp begin
        desc = Ref(QCSweepDesc(T, m + 1, 0, m, N, 0.0, 0, m, cols == N ? 0 : cols, p, -1,
                               pointer(G0), m == 0 ? C_NULL : pointer(Gd), p == 0 ? C_NULL : pointer(Gp),
                               0, 0, C_NULL, C_NULL, device, (wide ? (QC_SWEEP_WIDE | QC_SWEEP_WIDE_TANGENT) : 0) | (wide64 ? QC_SWEEP_WIDE_64 : 0) |
                               (wide64_tangent ? QC_SWEEP_WIDE_64_TANGENT : 0), (0, 0)))
        ok = Ref{Int32}(0)
        rc = ccall((:qc_sweep_desc_jvp_supported, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Int32}), desc, ok)
        (rc == 0 && ok[] == 1) || error(unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
        rc = ccall((:qc_sweep_create, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Ptr{Cvoid}}), desc, h)
        rc == 0 || error("qc_sweep_create: " * unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
    end
    rc = GC.@preserve Z⃗ init θt ct vz vi vθ vc finals tfinals ccall((:qc_sweep_jvp, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        h[], Z⃗, init, S, p == 0 ? C_NULL : pointer(θt), isempty(ct) ? C_NULL : pointer(ct), isempty(vz) ? C_NULL : pointer(vz),
        isempty(vi) ? C_NULL : pointer(vi), isempty(vθ) ? C_NULL : pointer(vθ), isempty(vc) ? C_NULL : pointer(vc), finals, C_NULL, tfinals,
        C_NULL)
    msg = rc == 0 ? "" : unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), h[]))
    ccall((:qc_sweep_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), h[])
    rc == 0 || error("qc_sweep_jvp: " * msg)
    return finals, tfinals
end

"""
    rollout_sweep_hessian_product(init, controls, Δt, G_drift, G_drives, G_pert, θ, cot; scale=nothing, cols, vZ=nothing, vinit=nothing,
                                  vtheta=nothing, vscale=nothing, vcot=nothing, device=0, wide=false)  ->  (tgrad, tgrad_samples, tgrad_init)

The tangent of the pullback of `rollout_sweep` along one direction (`qc_sweep_hvp`).  `cot` is (2N·cols)×S, one cotangent per sample;
`vZ` an (m+1)×T matrix in the knot layout [a; Δt] (only the columns of knots 1 … T−1 act), `vinit` a 2N·cols vector, `vtheta` S×p,
`vscale` S×m, `vcot` (2N·cols)×S; whichever is `nothing` is zero, at least one must be given.  Returns `tgrad`, (m+1)×T (the plain sum
over the samples, zero in the last column), `tgrad_samples`, (m+1)×(T−1)×S, and `tgrad_init`, (2N·cols)×S.  With `cot` the gradient of a
loss of the final states and `vcot` its Hessian times the pushforward's tangents, `tgrad` is the exact Hessian product of the loss.
Served for closed systems (antisymmetric generators) with 2N ≤ 16, m ≤ 8 and at most 16 columns.  `wide = true` sets
`qc_sweep_desc.wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_HESSIAN` (257): the matrix-core form up to 2N = 32 ("mfma32-sweep") with its Hessian
product, the same scope otherwise; nothing changes at 2N ≤ 16.  UNTESTED here, like the rest of this file.
"""
function rollout_sweep_hessian_product(init::AbstractVector{Float64}, controls::AbstractMatrix{Float64}, Δt::AbstractVector{Float64}, G_drift,
                                       G_drives, G_pert, θ::AbstractMatrix{Float64}, cot::AbstractMatrix{Float64}; scale=nothing, cols::Int,
                                       vZ=nothing, vinit=nothing, vtheta=nothing, vscale=nothing, vcot=nothing, device::Int=0,
                                       wide::Bool=false)
    n = size(G_drift, 1); N = n ÷ 2
    m, T = size(controls); p = length(G_pert); S = size(θ, 1)
    G0 = Float64.(vec(G_drift))
    Gd = m == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_drives])
    Gp = p == 0 ? Float64[] : reduce(vcat, [Float64.(vec(G)) for G in G_pert])
    Z⃗ = vec(vcat(controls, reshape(Δt, 1, T)))                      # knot layout [a; Δt]
    θt = Matrix{Float64}(transpose(θ))                               # sample-major
    ct = isnothing(scale) ? Float64[] : vec(Matrix{Float64}(transpose(scale)))
    size(cot) == (n * cols, S) || error("rollout_sweep_hessian_product: cot must be $(n * cols)×$S")
    (isnothing(vcot) || size(vcot) == (n * cols, S)) || error("rollout_sweep_hessian_product: vcot must be $(n * cols)×$S")
    (isnothing(vtheta) || size(vtheta) == (S, p)) || error("rollout_sweep_hessian_product: vtheta must be $S×$p")
    (isnothing(vscale) || size(vscale) == (S, m)) || error("rollout_sweep_hessian_product: vscale must be $S×$m")
    (isnothing(scale) || size(scale) == (S, m)) || error("rollout_sweep_hessian_product: scale must be $S×$m")
    cv = Float64.(vec(cot))                                          # column s is sample s: sample-major as it stands
    vcv = isnothing(vcot) ? Float64[] : Float64.(vec(vcot))
    vz = isnothing(vZ) ? Float64[] : Float64.(vec(vZ))
    vi = isnothing(vinit) ? Float64[] : Float64.(vec(vinit))
    vθ = isnothing(vtheta) ? Float64[] : vec(Matrix{Float64}(transpose(vtheta)))
    vc = isnothing(vscale) ? Float64[] : vec(Matrix{Float64}(transpose(vscale)))
    (isempty(vz) || length(vz) == (m + 1) * T) || error("rollout_sweep_hessian_product: vZ must be $(m + 1)×$T")
    (isempty(vi) || length(vi) == n * cols) || error("rollout_sweep_hessian_product: vinit must have $(n * cols) entries")
    tgrad = Matrix{Float64}(undef, m + 1, T)
    tsamp = Array{Float64}(undef, m + 1, T - 1, S)
    tginit = Matrix{Float64}(undef, n * cols, S)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve G0 Gd Gp begin
        desc = Ref(QCSweepDesc(T, m + 1, 0, m, N, 0.0, 0, m, cols == N ? 0 : cols, p, -1,
                               pointer(G0), m == 0 ? C_NULL : pointer(Gd), p == 0 ? C_NULL : pointer(Gp),
                               0, 0, C_NULL, C_NULL, device, wide ? (QC_SWEEP_WIDE | QC_SWEEP_WIDE_HESSIAN) : 0, (0, 0)))
        ok = Ref{Int32}(0)
        rc = ccall((:qc_sweep_desc_hvp_supported, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Int32}), desc, ok)
        (rc == 0 && ok[] == 1) || error(unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
        rc = ccall((:qc_sweep_create, LIB[]), Cint, (Ref{QCSweepDesc}, Ref{Ptr{Cvoid}}), desc, h)
        rc == 0 || error("qc_sweep_create: " * unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
    end
    rc = GC.@preserve Z⃗ init θt ct cv vz vi vθ vc vcv tgrad tsamp tginit ccall((:qc_sweep_hvp, LIB[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
        h[], Z⃗, init, S, p == 0 ? C_NULL : pointer(θt), isempty(ct) ? C_NULL : pointer(ct), cv, isempty(vz) ? C_NULL : pointer(vz),
        isempty(vi) ? C_NULL : pointer(vi), isempty(vθ) ? C_NULL : pointer(vθ), isempty(vc) ? C_NULL : pointer(vc),
        isempty(vcv) ? C_NULL : pointer(vcv), tgrad, tsamp, tginit)
    msg = rc == 0 ? "" : unsafe_string(ccall((:qc_sweep_last_error, LIB[]), Cstring, (Ptr{Cvoid},), h[]))
    ccall((:qc_sweep_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), h[])
    rc == 0 || error("qc_sweep_hvp: " * msg)
    return tgrad, tsamp, tginit
end

"""
    iso_vec_unitary_fidelity(Ũ⃗, Ũ⃗_goal; subspace=nothing, device=0, squared=false)          (unitary_minimum_time_problem.jl:77)
    iso_vec_unitary_free_phase_fidelity(Ũ⃗, Ũ⃗_goal, phases, phase_operators; subspace=nothing)  (unitary_minimum_time_problem.jl:86-90)

`squared = true` selects |tr|²/n² instead of the docstring's |tr|/n (INTEGRATION.md, table of unverifiable choices).
"""
function iso_vec_unitary_free_phase_fidelity(Ũ⃗::AbstractVector{Float64}, Ũ⃗_goal::AbstractVector{Float64}, phases, phase_operators;
                                             subspace=nothing, device::Int=0, squared::Bool=false)
    N = isqrt(length(Ũ⃗_goal) ÷ 2)
    sub = isnothing(subspace) ? Int32[] : Int32.(collect(subspace) .- 1)
    dims = Int32[size(Op, 1) for Op in phase_operators]
    planes = isempty(dims) ? Float64[] : reduce(vcat, [vcat(vec(Float64.(real.(Op))), vec(Float64.(imag.(Op)))) for Op in phase_operators])
    x = vcat(Ũ⃗, Float64.(collect(phases)))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve Ũ⃗_goal sub dims planes begin
        desc = Ref(QCFidelityDesc(0, N, pointer(Ũ⃗_goal), isempty(sub) ? C_NULL : pointer(sub), length(sub), squared ? 1 : 0,
                                  length(dims), device, isempty(dims) ? C_NULL : pointer(dims), isempty(planes) ? C_NULL : pointer(planes)))
        rc = ccall((:qc_fidelity_create_desc, LIB[]), Cint, (Ref{QCFidelityDesc}, Ref{Ptr{Cvoid}}), desc, h)
        rc == 0 || error("qc_fidelity_create_desc: " * unsafe_string(ccall((:qc_fidelity_last_error, LIB[]), Cstring, (Ptr{Cvoid},), C_NULL)))
    end
    F = Ref(0.0)
    GC.@preserve x ccall((:qc_fidelity_eval, LIB[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                         h[], x, F, C_NULL, C_NULL, C_NULL)
    ccall((:qc_fidelity_destroy, LIB[]), Cvoid, (Ptr{Cvoid},), h[])
    return F[]
end

iso_vec_unitary_fidelity(Ũ⃗::AbstractVector{Float64}, Ũ⃗_goal::AbstractVector{Float64}; kw...) =
    iso_vec_unitary_free_phase_fidelity(Ũ⃗, Ũ⃗_goal, Float64[], Matrix{ComplexF64}[]; kw...)

end # module
