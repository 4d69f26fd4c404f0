/*
 * qcolloc.h — C ABI of libqcolloc_hip.so: MI355X (gfx950) knot-point evaluator for the
 * direct-collocation unitary dynamics constraint of QuantumCollocation.jl.
 *
 * This header IS the drop-in boundary.  Every entry point replaces one observable piece of the
 * `QuantumDynamics` object that QuantumCollocationCore builds inside
 * `QuantumControlProblem(traj, J, integrators; ...)`
 * (reference src/problem_templates/unitary_smooth_pulse_problem.jl:181-190) and that the reference's
 * own micro-benchmark exercises (reference test/scripts/integrator_test_1qubit.jl:41-52):
 *
 *   reference (Julia)                                   this ABI
 *   -------------------------------------------------   -----------------------------------------
 *   QuantumSystem(H_drift, H_drives).G_drift/G_drives    qc_generator_from_hamiltonian
 *       (unitary_smooth_pulse_problem.jl:199)
 *   operator_to_iso_vec / iso_vec_to_operator            qc_operator_to_iso_vec / qc_iso_vec_to_operator
 *       (trajectory_initialization.jl:40-41,137,413-418)
 *   UnitaryPadeIntegrator(state, control, sys, traj;     qc_desc{integrator=QC_PADE, pade_order,...}
 *       order)  (unitary_smooth_pulse_problem.jl:165-167)
 *   UnitaryExponentialIntegrator(...)  (:168-170)        qc_desc{integrator=QC_EXPONENTIAL}
 *   QuantumStatePadeIntegrator(state, control, sys, traj)  qc_desc{state_cols = number of kets}
 *       (quantum_state_smooth_pulse_problem.jl:146-152)
 *   DerivativeIntegrator(x, dx, traj)  (:177-178)        qc_desc.deriv_{x_off,dx_off,dim}[i]
 *   QuantumDynamics(integrators, traj)                   qc_create
 *       (integrator_test_1qubit.jl:41)
 *   dynamics.F(Z.datavec)               (:45)            qc_eval_F        / qc_eval_F_dev
 *   dynamics.dF(Z.datavec)              (:46)            qc_eval_jac      / qc_eval_F_jac(_dev)
 *   dynamics.dF_structure               (:46)            qc_jac_structure
 *   dynamics.dF(Z) * v, dynamics.dF(Z)' * lam            qc_eval_jvp / qc_eval_vjp (_dev, _dev_multi): matrix-free
 *   (dynamics.mu_d2F(Z, mu), symmetric) * v               qc_eval_hvp (_dev, _dev_multi): matrix-free
 *   dynamics.mu_d2F(Z.datavec, mu)      (:52)            qc_eval_hess     / qc_eval_hess_dev
 *   dynamics.mu_d2F_structure           (:52)            qc_hess_structure
 *   shapes (Z.dims.states*(Z.T-1), Z.dim*Z.T+Z.global_dim)  (:44,48)   qc_dims
 *   K unitary integrators of a UnitarySamplingProblem    qc_eval_F_list / _jac_list / _F_jac_list / _hess_list (host buffers),
 *       (unitary_sampling_problem.jl:134-155), the           qc_eval_F_jac_dev_multi / qc_eval_hess_dev_multi (device buffers)
 *       members of a UnitaryDirectSumProblem                  (one handle per state integrator, qc_desc.rows_per_interval ...)
 *       (unitary_direct_sum_problem.jl:127-130), the kets
 *       x systems of a QuantumStateSamplingProblem
 *   UnitaryBangBangProblem's [U, D(a, da)], order 12      one handle: n_deriv = 1, pade_order = 12; the slack components only
 *       (unitary_bang_bang_problem.jl:163-175,205-215)        widen zdim
 *   DensityOperatorExponentialIntegrator                 qc_desc{N = levels^2, state_cols = 1, QC_EXPONENTIAL}
 *       (density_operator_smooth_pulse_problem.jl:104-106)   with the Lindblad generators as G_drift / G_drives
 *   iso_vec_unitary_fidelity, UnitaryInfidelityObjective,  qc_fidelity_create / qc_fidelity_eval(_dev)
 *   FinalUnitaryFidelityConstraint                           (unitary_minimum_time_problem.jl:77-84)
 *   iso_fidelity, QuantumStateObjective,                 qc_fidelity_create_kind(QC_FID_KET | QC_FID_DENSITY)
 *   DensityOperatorPureStateInfidelityObjective
 *   QuadraticRegularizer, MinimumTimeObjective           qc_terms_create / qc_terms_eval(_dev)
 *       (unitary_smooth_pulse_problem.jl:151-153, unitary_minimum_time_problem.jl:67-69)
 *   QuadraticSmoothnessRegularizer, Pairwise-            qc_terms_create_ext / qc_terms_eval(_dev)
 *   QuadraticRegularizer, L1Regularizer! (its cost)
 *       (unitary_smooth_pulse_problem.jl:311-340, unitary_direct_sum_problem.jl:130-169, _problem_templates.jl:41-54)
 *   UnitaryRobustnessObjective(H_error=...)              qc_robust_create / qc_robust_eval(_dev)
 *       (unitary_robustness_problem.jl:46-49)
 *   unitary_rollout / rollout / open_rollout             qc_rollout / qc_rollout_dev
 *       (trajectory_initialization.jl:426,493,547)
 *   unitary_rollout over systems(zeta)                   qc_sweep_create / qc_sweep_eval(_dev)
 *       (unitary_sampling_problem.jl:233-243)
 *
 * Conventions
 *   - All matrices are column-major (Julia order).  All arrays are caller-owned; nothing is retained
 *     after a call returns, except that G_drift/G_drives are copied to the device by qc_create.
 *   - Return value 0 = QC_OK, negative = error; text via qc_last_error (thread-local for
 *     handle-less calls).  Nothing throws or exits across this boundary.
 *   - A handle from qc_create is bound to ONE HIP device and evaluates the interval range [t_begin, t_end) of the
 *     T-1 intervals; a handle from qc_create_multi spreads that range over several devices inside this
 *     library (one process, N GPUs: what a Julia/Ipopt consumer needs).  Every entry
 *     point selects the handle's device itself and restores the caller's current device before returning.
 *     A handle is not thread-safe and may have ONE evaluation in flight at a time: several kernels keep
 *     scratch in the handle (lds-gws, mfma64 Hessian, rollout, batched launches), so a second "_dev"
 *     call on another stream must be ordered after the first by the caller (different handles are
 *     independent).  Non-finite inputs are evaluated, not rejected (Ipopt probes wild points).
 *   - "_dev" entry points take DEVICE pointers and a hipStream_t (passed as void*) and are
 *     asynchronous on that stream.  The plain entry points take HOST pointers and return after the
 *     results are in the caller's buffers.
 *   - Every wait of a host-buffer call on the device has a deadline (environment QC_HOST_TIMEOUT_MS, default 30 s).  A call that runs
 *     into it returns QC_ERR_HIP WITHOUT synchronising (a hung device would hang that, too): work of that call may still be queued and
 *     may still write into the output buffers it was given and into memory of qc_host_alloc.  Those buffers must stay allocated and
 *     are not to be read until the handle's next call has returned (it drains the handle's streams before it reuses anything) or the
 *     handle has been destroyed (qc_destroy drains them too).
 *   - There is no CPU fallback: without a visible gfx950 device qc_create fails with QC_ERR_NO_DEVICE.
 */
#ifndef QCOLLOC_H
#define QCOLLOC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QC_VERSION_MAJOR 0
#define QC_VERSION_MINOR 6

enum {
    QC_OK = 0,
    QC_ERR_INVALID = -1,    /* bad descriptor / argument */
    QC_ERR_NO_DEVICE = -2,  /* no HIP device, or not gfx950 */
    QC_ERR_HIP = -3,        /* a HIP runtime call failed */
    QC_ERR_UNSUPPORTED = -4 /* valid request this build cannot serve (e.g. qc_multi_all_gather_dev with two shards on one device) */
};

enum { QC_PADE = 0, QC_EXPONENTIAL = 1 };

/* Kernel selection (qc_desc.kernel). AUTO picks the MFMA path for systems with N <= 16 levels (sizes other than 8 / 16
 * levels zero-padded to the tiles) with the Pade order 4 or the exponential integrator, for up to 8 levels with any Pade
 * order, and for 17 .. 32 levels (5 qubits) with the Pade order 4; else the generic LDS/VALU path (its scratch in a global
 * workspace when it exceeds the LDS).  The Hessian of a 17 .. 32-level MFMA handle allocates 128 MiB of device scratch at
 * its first evaluation.  Forcing a path that cannot serve the descriptor is QC_ERR_UNSUPPORTED. */
enum { QC_KERNEL_AUTO = 0, QC_KERNEL_LDS = 1, QC_KERNEL_MFMA = 2 };

#define QC_MAX_DERIV 8
#define QC_HESS_ALIGN_LINE 16   /* qc_desc.hess_align of the line-aligned (padded) Hessian value layout */
enum { QC_ROWS_STACKED = 0, QC_ROWS_BY_COMPONENT = 1 };

typedef struct qc_handle qc_handle;

/* Value blocks of an interval (qc_desc.jac_block_order / hess_block_order; the enumerators' order is the default order).
 * Jacobian: d/dU_t = -I (x) F (N dense n x n blocks) | d/dU_t+1 = I (x) B (exponential integrator: the identity, s entries) | d/da
 * (s x m, column-major) | d/ddt (s; free timestep) | the derivative integrators' entries.
 * Hessian (upper triangle): (U_t, a) | (a, U_t+1) | (U_t, dt) | (dt, U_t+1) | (a, a) upper | (a, dt) | (dt, dt) | (dx, dt);
 * blocks that do not exist for a handle (fixed timestep; exponential integrator: nothing touches knot t+1) have length 0. */
enum { QC_JB_F = 0, QC_JB_B = 1, QC_JB_A = 2, QC_JB_H = 3, QC_JB_D = 4, QC_JAC_BLOCKS = 5 };
enum { QC_HB_UA = 0, QC_HB_AU = 1, QC_HB_UH = 2, QC_HB_HU = 3, QC_HB_AA = 4, QC_HB_AH = 5, QC_HB_HH = 6, QC_HB_D = 7, QC_HESS_BLOCKS = 8 };

/* Problem descriptor.  Offsets are 0-based positions inside one knot vector z_t of length zdim
 * (reference component order [U~, a, da, dda, dt]: trajectory_initialization.jl:357-382; other
 * templates order differently, e.g. integrator_test_1qubit.jl:24-30, hence parameters). */
typedef struct qc_desc {
    int32_t N;           /* Hilbert-space dimension; iso dimension n = 2N; state length s = 2N^2 */
    int32_t m;           /* number of drives (system.n_drives) */
    int64_t T;           /* number of knot points (Z.T) */
    int32_t zdim;        /* knot dimension (Z.dim) */
    int64_t global_dim;  /* trailing global variables after zdim*T (Z.global_dim); columns only */
    int32_t off_U;       /* offset of U~ (length s) */
    int32_t off_a;       /* offset of the control a (length m) */
    int32_t off_dt;      /* offset of the timestep, or -1 for a fixed timestep */
    double dt_fixed;     /* timestep when off_dt < 0 */
    int32_t integrator;  /* QC_PADE | QC_EXPONENTIAL */
    int32_t pade_order;  /* even, 2..20 (reference uses 4 by default, 12 in unitary_bang_bang_problem.jl:208) */
    int32_t n_deriv;     /* number of DerivativeIntegrators, rows appended after the unitary rows */
    int32_t deriv_x_off[QC_MAX_DERIV];
    int32_t deriv_dx_off[QC_MAX_DERIV];
    int32_t deriv_dim[QC_MAX_DERIV];
    const double* G_drift;  /* n*n, column-major:   iso(-i H_drift) */
    const double* G_drives; /* m matrices of n*n, column-major each */
    int32_t device;         /* HIP device ordinal this handle is bound to */
    int32_t kernel;         /* QC_KERNEL_* */
    int64_t t_begin;        /* first interval (0-based) this handle evaluates */
    int64_t t_end;          /* one past the last interval; t_begin = t_end = 0 means [0, T-1) */
    int32_t state_cols;     /* columns of the iso state matrix: 0 or N = a unitary U~ (2N x N, length 2N^2);
                             * K >= 1 = K kets psi~ = [Re psi; Im psi] stored back to back (2N x K, length 2NK), i.e.
                             * K QuantumStatePadeIntegrators over the same system
                             * (quantum_state_smooth_pulse_problem.jl:146-152).  off_U is the first ket's offset. */
    int32_t hess_align;     /* 0 (default) or 1: the Hessian value block of an interval holds EXACTLY the structural entries -- the
                             * reference's mu_d2F_structure, entry for entry (config 3: 1 832 per interval; observable as
                             * length(dynamics.mu_d2F_structure), test/scripts/integrator_test_1qubit.jl:48-52).  This is what every
                             * host-buffer entry point and both bindings use unless told otherwise (ABI 0.5; through ABI 0.4 the value
                             * 0 meant 16).
                             * k > 1 (QC_HESS_ALIGN_LINE = 16 doubles = 128 B for device-resident consumers): the block is padded with
                             * explicit zeros to a multiple of k doubles, so that every interval's block starts on a cache-line
                             * boundary (partial lines written by two workgroups cost 1.1 - 1.4x the HBM write traffic).
                             * The padding entries appear in the structure as duplicates of the interval's first structure entry with
                             * value 0 (COO duplicates are summed: reference test/test_utils.jl:14-20).  An opt-in of "_dev" consumers
                             * that own their sparse assembly; a host-buffer call is bound by PCIe and gains nothing from it.
                             * Ignored for composed handles (hess_per_interval > 0): see hess_tail_zeros. */
    /* Composition (all 0 = this handle is the whole dynamics).  A problem whose integrator list holds several
     * unitary integrators (UnitarySamplingProblem: one per system over a merged trajectory,
     * unitary_sampling_problem.jl:134-155) is served by one handle per unitary integrator; each handle's rows and
     * values are placed inside the problem's per-interval blocks.  Composed handles are evaluated through the "_dev" / "_dev_multi"
     * entry points (device buffers) or the "_list" entry points (host buffers), never through qc_eval_F / _jac / _hess. */
    int64_t rows_per_interval;  /* dynamics rows of the whole problem per interval (Z.dims.states) */
    int64_t row_offset;         /* first row of this handle inside that block */
    int64_t jac_per_interval;   /* Jacobian values of the whole problem per interval */
    int64_t jac_offset;
    int64_t hess_per_interval;  /* Hessian values of the whole problem per interval */
    int64_t hess_offset;
    /* Row placement.  QC_ROWS_STACKED (0): this handle's rows are [state integrator (s) | derivative integrators in
     * order], starting at row_offset.  QC_ROWS_BY_COMPONENT (1): the state integrator's rows start at row_offset and
     * derivative integrator i's rows at deriv_row_off[i] inside the per-interval block of rows_per_interval rows (which
     * must then be given): every integrator's rows sit at its state component's position among the trajectory's state
     * components, and components WITHOUT an integrator leave structurally empty rows, so that
     * n_rows == Z.dims.states * (T - 1) as the reference's own harness declares
     * (test/scripts/integrator_test_script.jl:23-44, integrator_test_1qubit.jl:24-44).  Empty rows are never written by
     * the "_dev" entry points (zero them once); the host-buffer entry points deliver them as 0. */
    int32_t row_placement;
    int32_t hess_tail_zeros;    /* composed handles only: explicit zero entries this handle appends after its own Hessian
                                 * values (the composer pads the shared per-interval block through its last handle) */
    int32_t deriv_row_off[QC_MAX_DERIV];
    /* Order of the value blocks INSIDE an interval (ABI 0.6).  The values of an interval are a sequence of blocks; which block comes
     * where is this library's choice, and the reference's own intra-knot COO order is not known here ("keep a
     * permutation hook").  Once `julia/reconcile.jl` has printed Core's order, a binding that wants the value vectors in THAT order --
     * without a 40 MB gather on the host per dF call -- names it here: a permutation of QC_JB_* / QC_HB_* (all zeros = the default
     * order, the enumerators' order).  Structures, block offsets and every kernel follow it; the order of the entries inside a block
     * (column-major) and of the derivative integrators' pieces stays.  Costs: the host-buffer Jacobian path sends one copy of the
     * replicated blocks over PCIe only in the default order (another order: the full values), and the one-call launch stores the
     * scalar Hessian entries one by one unless the four scalar kinds close the block in the default order. */
    int32_t jac_block_order[QC_JAC_BLOCKS];
    int32_t hess_block_order[QC_HESS_BLOCKS];
} qc_desc;

typedef struct qc_dims_t {
    int64_t n_rows;          /* ddim*(T-1): rows of dF, length of F and mu (whole problem) */
    int64_t n_cols;          /* zdim*T + global_dim */
    int64_t ddim;            /* dynamics rows per interval */
    int64_t jac_nnz_interval;
    int64_t hess_nnz_interval;
    int64_t n_intervals;     /* t_end - t_begin, intervals this handle owns */
    int64_t F_len;           /* rows per interval of the F vector this handle writes into (ddim, or rows_per_interval when
                              * given) * n_intervals */
    int64_t jac_nnz;         /* jac_nnz_interval * n_intervals */
    int64_t hess_nnz;        /* hess_nnz_interval * n_intervals (0 if no analytic Hessian); hess_nnz_interval includes the
                              * alignment padding (qc_desc.hess_align / hess_tail_zeros) */
    int64_t Z_len;           /* zdim*T + global_dim: length of the Z argument (always the full vector) */
    int32_t kernel;          /* QC_KERNEL_LDS or QC_KERNEL_MFMA actually selected */
    int32_t reserved;
} qc_dims_t;

/* ---- host-side helpers (no GPU needed) ------------------------------------------------------ */

/* U (N x N complex, column-major, split re/im planes) -> iso-vec of length 2N^2:
 * vec(vcat(real(U), imag(U)))  (reference trajectory_initialization.jl:137). */
int qc_operator_to_iso_vec(int32_t N, const double* U_re, const double* U_im, double* iso_vec);
int qc_iso_vec_to_operator(int32_t N, const double* iso_vec, double* U_re, double* U_im);

/* H (N x N complex Hermitian, column-major re/im planes) -> G = iso(-iH) = [[Im H, Re H],[-Re H, Im H]]
 * (2N x 2N, column-major), i.e. QuantumSystem's G_drift / G_drives entries. */
int qc_generator_from_hamiltonian(int32_t N, const double* H_re, const double* H_im, double* G);

/* Eigen-decomposition A = V diag(w) V' of a complex Hermitian d x d matrix (column-major, re / im planes), d <= 64: the
 * host-side set-up step of the free-phase fidelity (phase operators, qc_fidelity_desc), exposed so that it can be checked. */
int qc_hermitian_eig(int32_t d, const double* A_re, const double* A_im, double* w, double* V_re, double* V_im);

/* Pade coefficients c_0..c_p (p = order/2) of the diagonal approximant. out has p+1 entries. */
int qc_pade_coefficients(int32_t order, double* out);

/* Sizes implied by a descriptor, without touching a GPU (G pointers may be NULL). */
int qc_desc_dims(const qc_desc* d, qc_dims_t* out);
/* Sparsity structure implied by a descriptor, without touching a GPU.  Global COO indices of this
 * handle's slice, knot-major, in the exact order of the value vectors.  one_based != 0 gives Julia
 * indices.  rows/cols must hold jac_nnz (resp. hess_nnz) entries.  The Hessian structure is
 * upper-triangular (row <= col). */
int qc_desc_jac_structure(const qc_desc* d, int64_t* rows, int64_t* cols, int one_based);
int qc_desc_hess_structure(const qc_desc* d, int64_t* rows, int64_t* cols, int one_based);

/* ---- handle ----------------------------------------------------------------------------------- */

int qc_create(const qc_desc* d, qc_handle** out);
void qc_destroy(qc_handle* h);
/* Message of the last error on this handle (or, with h == NULL, of the last handle-less call on
 * this thread).  Never NULL. */
const char* qc_last_error(const qc_handle* h);

int qc_dims(const qc_handle* h, qc_dims_t* out);
/* Names of the device kernels this handle's evaluations run on (diagnostic; static strings, never NULL):
 * which = 0: F / F + dF ("mfma16-pade4", "mfma16-padeP", "mfma32-pade4-ell" (sparse drive generators) / "mfma32-pade4",
 * "mfma64-pade4", "mfma16-exp" / "mfma16-exp-gather" (drive generators with one entry per row), "mfma32-exp" / "mfma32-exp-gather", "lds", "lds-gws");
 * which = 1: mu_d2F ("mfma16-pade4-hess-gather" (drive generators with one entry per row) / "mfma16-pade4-hess2" /
 * "mfma16-pade4-hess", "mfma16-padeP-hess", "mfma32-pade4-hess-ell" / "mfma32-pade4-hess", "mfma64-pade4-hess", "lds-hess",
 * "lds-gws-hess"; exponential integrator: "mfma16-exp-hess", "mfma16-exp-hess-gather"
 * (drive generators with one entry per row: Pauli strings), "mfma32-exp-hess" / "mfma32-exp-hess-gather", "lds-exp-hess", "lds-gws-exp-hess");
 * which = 2: qc_eval_F_jac_hess_dev ("mfma16-pade4-fused-gather" / "mfma16-pade4-fused", "mfma32-pade4-fused-ell", or
 * "two-launches");
 * which = 3: dF v ("mfma16-pade4-jvp": the fused matrix-free kernel of the order-4 Pade integrator at 2N <= 16, up to 8 state columns
 * and 8 drives; else "generic-jvp"), which = 4: dF' lam ("generic-vjp" on every handle) -- generic: the handle's own dF launch into a
 * scratch of the handle, then a product kernel;
 * which = 5: (mu d2F) v ("generic-hvp" on every handle: the handle's own mu_d2F launch into a scratch of the handle, then a product
 * kernel; there is no fused matrix-free kernel for it). */
const char* qc_kernel_name(const qc_handle* h, int32_t which);
int qc_jac_structure(const qc_handle* h, int64_t* rows, int64_t* cols, int one_based);
int qc_hess_structure(const qc_handle* h, int64_t* rows, int64_t* cols, int one_based);

/* ---- evaluation, host buffers (what Ipopt's callbacks hand over) ------------------------------ */
/* Z: full trajectory vector (Z_len doubles).  F: F_len.  vals: jac_nnz.  mu: the FULL multiplier
 * vector of length n_rows (as MOI passes it); hvals: hess_nnz. */
int qc_eval_F(qc_handle* h, const double* Z, double* F);
int qc_eval_jac(qc_handle* h, const double* Z, double* vals);
int qc_eval_F_jac(qc_handle* h, const double* Z, double* F, double* vals);
int qc_eval_hess(qc_handle* h, const double* Z, const double* mu, double* hvals);

/* Ipopt's `new_x` flag (the C interface hands it to every callback; MOI evaluators track it themselves): new_x = 0 declares
 * that the trajectory vector of the following host-buffer calls is the one the handle's previous host-buffer call received --
 * the accepted trial point, at which Ipopt asks for the Jacobian and the Hessian after the residuals -- so the knots already
 * on the device are used and Z is not read at all.  Stays in force until qc_set_new_x(h, 1) (the default: every call copies
 * its Z).  A handle that has not seen a Z yet copies regardless.  Multi-device handles pass the flag on to their shards. */
int qc_set_new_x(qc_handle* h, int new_x);
/* How many times the handle has copied a trajectory vector's knots to the device so far (host-buffer calls with new_x = 1; -1 for a
 * NULL handle).  A binding that elides uploads remembers the value after the call that put ITS x on the device and sets new_x = 0
 * only while the value is unchanged: any other host-buffer call on the same handle in between (another closure, a second evaluator)
 * moves it.  qc_rollout keeps its trajectory vector in a buffer of its own and does not count. */
int64_t qc_knot_generation(const qc_handle* h);

/* Pinned host memory for long-lived arrays (optional).  The host-buffer calls move Z, mu, the residuals and the Hessian values between
 * the caller's arrays and the device with the GPU's copy engine; for ordinary (pageable) memory the runtime pins the pages for the
 * duration of every call.  Memory from qc_host_alloc is pinned for good (hipHostMalloc, visible to every device):
 *   - qc_eval_F writes the residuals into it straight from the kernel -- no device-to-host copy at all (config 3: 0.07 ms per call
 *     instead of 0.09, profiles/r04_f_path_probe.txt); layouts with rows no kernel writes (QC_ROWS_BY_COMPONENT) keep the copy;
 *   - every other transfer from / into it skips the per-call pinning.
 * The values are the same to the bit.  The bindings take the result vectors their closures hand out from here, an evaluator its
 * residual cache.  (Pinning arrays the CALLER allocated -- hipHostRegister -- was built first and withdrawn: under allocator churn in a
 * long-running process the GPU's writes into such ranges faulted intermittently, profiles/NOTES.md.)  Process-wide, thread-safe, not
 * tied to a handle; QC_ERR_NO_DEVICE without a GPU. */
int qc_host_alloc(int64_t bytes, void** out);
int qc_host_free(void* p);

/* ---- evaluation, device-resident (asynchronous on `stream`, a hipStream_t) --------------------- */
/* dZ: device pointer to the full Z vector (8-byte aligned).  dF may be NULL (skip residual store);
 * dvals may be NULL (residual only).  dF/dvals/dhvals point at THIS HANDLE'S slice
 * (interval t_begin first) and must be 8-byte aligned (the kernels issue 8-byte stores only). */
int qc_eval_F_jac_dev(qc_handle* h, const double* dZ, double* dF, double* dvals, void* stream);
int qc_eval_hess_dev(qc_handle* h, const double* dZ, const double* dmu, double* dhvals, void* stream);

/* dynamics.dF(Z) and dynamics.mu_d2F(Z, mu) (and F) at the same Z in one call -- what Ipopt asks for at every accepted point
 * (integrator_test_1qubit.jl:46,52).  One kernel launch where a fused kernel serves the handle (qc_kernel_name(h, 2):
 * "mfma16-pade4-fused" -- order-4 Pade, a unitary on 8 levels, Hermitian Hamiltonians, up to 6 drives: BASELINE configs 3 / 4), else
 * the two launches of qc_eval_F_jac_dev and qc_eval_hess_dev on `stream`; the values are bit-identical either way.  dF may be NULL. */
int qc_eval_F_jac_hess_dev(qc_handle* h, const double* dZ, const double* dmu, double* dF, double* dvals, double* dhvals, void* stream);

/* Matrix-free Jacobian products at Z: what a consumer that never needs the VALUES of dF asks for (augmented-Lagrangian and first-order
 * methods: grad(lam'F + rho/2 |F|^2) = dF'(lam + rho F); Krylov solves of the KKT system; adjoint checks; MOI's
 * eval_constraint_jacobian_product / _transpose_product).  Two vectors of Z_len and F_len doubles move instead of jac_nnz values.
 * Repeated calls return the same bits: no floating-point atomics, every output entry has one writer and a fixed summation order.
 * The first call on a handle that takes the generic path (qc_kernel_name(h, 3 / 4)) allocates its scratch and tables (it synchronises
 * the device and cannot be captured in a graph; call once first); one evaluation in flight per handle, as everywhere.
 * qc_desc.jac_block_order cannot change a product.  Handles from qc_create_multi: QC_ERR_UNSUPPORTED (use the shard handles). */
/* y = dF(Z) v.   v: Z_len, y: F_len (the handle's rows; rows no integrator owns -- QC_ROWS_BY_COMPONENT -- are not written, as by F) */
int qc_eval_jvp_dev(qc_handle* h, const double* dZ, const double* dv, double* dy, void* stream);
/* w = dF(Z)' lam. lam: F_len, w: Z_len, EVERY entry written: variables the handle's intervals do not touch (the last knot's
 * controls and timestep, components no integrator reads, the global_dim tail, knots outside a shard's range) are exactly 0.0 */
int qc_eval_vjp_dev(qc_handle* h, const double* dZ, const double* dlam, double* dw, void* stream);
/* host buffers; honour qc_set_new_x like their siblings (rows of y that no integrator owns are delivered as 0) */
int qc_eval_jvp(qc_handle* h, const double* Z, const double* v, double* y);
int qc_eval_vjp(qc_handle* h, const double* Z, const double* lam, double* w);
/* integrator lists on one device (sampling, direct sum: members with qc_desc placement over one merged trajectory):
 * y rows member by member; w = the SUM over members, in member order (the first member overwrites, the others add) */
int qc_eval_jvp_dev_multi(qc_handle* const* hs, int32_t count, const double* dZ, const double* dv, double* dy, void* stream);
int qc_eval_vjp_dev_multi(qc_handle* const* hs, int32_t count, const double* dZ, const double* dlam, double* dw, void* stream);

/* Matrix-free product with the Hessian of the Lagrangian of the dynamics: w = H(Z, mu) v, where H is the full symmetric Z_len x Z_len
 * matrix whose upper triangle qc_hess_structure and qc_eval_hess[_dev] of the same handle describe -- entries with equal coordinates
 * summed, a diagonal entry counted once, an off-diagonal entry (i, j) giving H_ij v_j to w_i and H_ij v_i to w_j.  What a truncated
 * Newton or Krylov method asks for beside the Jacobian products (hess(L_rho) v = hess(J) v + ((lam + rho F) d2F) v + rho dF'(dF v)),
 * and MOI's eval_hessian_lagrangian_product: two vectors of Z_len doubles move instead of hess_nnz values.
 * mu / dmu: exactly what qc_eval_hess / qc_eval_hess_dev take (the FULL multiplier vector, n_rows).  v, w: Z_len.  EVERY entry of w is
 * written; entries that no structural Hessian entry of the handle's intervals touches (state components no integrator reads, the last
 * knot's controls and timestep, the global_dim tail, knots outside a shard's range) are exactly +0.0.
 * qc_desc.hess_align, hess_tail_zeros and hess_block_order cannot change a product (the padding takes no part, the sums run in the
 * order of the coordinates).  No floating-point atomics: every entry of w has one writer and a fixed summation order, repeated calls
 * return the same bits.  The first call on a handle allocates a scratch of n_intervals x (values per interval) doubles and a table (it
 * synchronises the device and cannot be captured in a graph; call once first); both are released by qc_destroy.
 * QC_ERR_UNSUPPORTED: handles without an analytic Hessian (hess_nnz == 0), handles from qc_create_multi (use the shard handles). */
int qc_eval_hvp_dev(qc_handle* h, const double* dZ, const double* dmu, const double* dv, double* dw, void* stream);
/* host buffers; honours qc_set_new_x like its siblings */
int qc_eval_hvp(qc_handle* h, const double* Z, const double* mu, const double* v, double* w);
/* integrator lists on one device: w = the SUM over members, in member order (the first member overwrites, the others add) */
int qc_eval_hvp_dev_multi(qc_handle* const* hs, int32_t count, const double* dZ, const double* dmu, const double* dv, double* dw, void* stream);

/* Several handles over the same trajectory in ONE launch: the K unitary integrators of a `UnitarySamplingProblem`
 * (reference unitary_sampling_problem.jl:134-155), each created with its slot of the shared per-interval blocks
 * (rows_per_interval / row_offset / ...).  dF / dvals / dhvals point at the SHARED vectors.  Handles whose shapes or
 * kernels differ are evaluated one launch each, with the same result. */
int qc_eval_F_jac_dev_multi(qc_handle* const* hs, int32_t count, const double* dZ, double* dF, double* dvals, void* stream);
int qc_eval_hess_dev_multi(qc_handle* const* hs, int32_t count, const double* dZ, const double* dmu, double* dhvals, void* stream);

/* The same integrator lists with HOST buffers -- what a CPU consumer (Ipopt through the MOI evaluator) of a
 * `UnitarySamplingProblem` (unitary_sampling_problem.jl:134-155: [U_1 .. U_K, D, D], shared controls), a
 * `UnitaryDirectSumProblem` (unitary_direct_sum_problem.jl:127-130: [U_1, D, D, U_2, D, D, ...], own controls per member) or
 * a `QuantumStateSamplingProblem` (quantum_state_sampling_problem.jl:98-122) calls as dynamics.F(Z), dynamics.dF(Z),
 * dynamics.mu_d2F(Z, mu).  `hs` = the composed handles of the list in integrator order, all on one device over one
 * trajectory and interval range.  Z is uploaded once, the handles are evaluated as in the "_dev_multi" calls, and F / vals /
 * hvals receive the whole problem's vectors: rows_per_interval, jac_per_interval, hess_per_interval values per interval,
 * interval-major.  The calls return when the arrays are complete.  qc_set_new_x(hs[0], 0) / qc_knot_generation(hs[0])
 * apply to the list (hs[0] owns the staging).  Errors are recorded on hs[0]. */
int qc_eval_F_list(qc_handle* const* hs, int32_t count, const double* Z, double* F);
int qc_eval_jac_list(qc_handle* const* hs, int32_t count, const double* Z, double* vals);
int qc_eval_F_jac_list(qc_handle* const* hs, int32_t count, const double* Z, double* F, double* vals);
int qc_eval_hess_list(qc_handle* const* hs, int32_t count, const double* Z, const double* mu, double* hvals);

/* ---- one handle over several GPUs ("n_gpus, device_ids[]"; 8e) ------------------------------------ */
/* The reference's consumer is ONE process (Julia + Ipopt, unitary_smooth_pulse_problem.jl:181-190, solve! at :219), so
 * the knot sharding of SURVEY 8(e) lives behind this boundary: qc_create_multi splits the descriptor's interval range
 * [t_begin, t_end) into n_shards contiguous chunks of ceil(len / n_shards) intervals (trailing shards may be short or
 * empty), shard i bound to HIP device device_ids[i] (ordinals may repeat: several shards on one device).  The result
 * is an ordinary qc_handle: qc_dims / qc_*_structure / qc_eval_F / qc_eval_jac / qc_eval_F_jac / qc_eval_hess /
 * qc_rollout behave exactly as on a single-device handle over the same range and return bit-identical arrays; every
 * shard has its own host thread, stream and pinned staging, copies only its knots (+ 1 halo knot) to its device and
 * writes its contiguous slice of the caller's arrays, so the N PCIe links run in parallel.  There is no collective on
 * this path (a CPU consumer needs none).  The "_dev" entry points take ONE device's pointers: use them on the shard
 * handles (qc_multi_shard), or qc_multi_eval_F_jac_dev / qc_multi_all_gather_dev below. */
int qc_create_multi(const qc_desc* d, int32_t n_shards, const int32_t* device_ids, qc_handle** out);
/* Number of shards of a multi-device handle (0 for a single-device handle). */
int32_t qc_multi_count(const qc_handle* h);
/* Borrowed pointer to shard i's single-device handle (owned by h; NULL if out of range).  Its interval range, device and
 * sizes are in its qc_dims; its device ordinal via qc_multi_shard_info. */
qc_handle* qc_multi_shard(qc_handle* h, int32_t i);
int qc_multi_shard_info(const qc_handle* h, int32_t i, int32_t* device, int64_t* t_begin, int64_t* t_end);
/* Device-resident evaluation of every shard, each on its own device and internal stream, asynchronous; dZ[i] / dF[i] /
 * dvals[i] are DEVICE pointers on shard i's device: dZ[i] the full Z vector, dF[i] / dvals[i] FULL-LENGTH vectors of
 * the multi handle's range (shard i writes its slice at its offset; a chunk-padded length, qc_multi_padded_len, is
 * needed for the all-gather).  dF or dvals may be NULL.  qc_multi_sync waits for all shards.
 * Ordering: the launches go out on each shard's INTERNAL stream, which knows nothing of the streams that produced dZ[i] / dmu[i]:
 * the inputs must be complete on their devices before these calls (synchronise the producing streams or devices first), and the
 * outputs may be read after qc_multi_sync. */
int qc_multi_eval_F_jac_dev(qc_handle* h, const double* const* dZ, double* const* dF, double* const* dvals);
int qc_multi_eval_hess_dev(qc_handle* h, const double* const* dZ, const double* const* dmu, double* const* dhvals);
int qc_multi_sync(qc_handle* h);
/* RCCL all-gather over xGMI of the per-shard slices (north_star / SURVEY 8e: "ncclAllGather on the per-GPU value
 * blocks when a device-resident full Jacobian is wanted"): in place on the full-length vectors, bufs[i] on shard i's
 * device holding that shard's slice at offset i * chunk * per_interval; afterwards every device holds all slices.
 * per_interval = doubles per interval (jac_nnz_interval, ddim or hess_nnz_interval); every buffer must hold
 * qc_multi_padded_len(h, per_interval) doubles.  Needs distinct devices (one RCCL rank per device; librccl is loaded
 * on first use, QC_ERR_UNSUPPORTED when it is absent or devices repeat).  Ordered after the shards' evaluations on their
 * internal streams; qc_multi_sync waits for it. */
int64_t qc_multi_padded_len(const qc_handle* h, int64_t per_interval);
int qc_multi_all_gather_dev(qc_handle* h, double* const* bufs, int64_t per_interval);

/* sizeof of the ABI structs as this build sees them: a binding asserts them against its own mirror at load time. */
int64_t qc_sizeof_desc(void);
int64_t qc_sizeof_dims(void);
int64_t qc_sizeof_terms_desc(void);

/* ---- fidelity of the final knot (SURVEY 8f "next" row 1) -------------------------------------------- */
/* F(U~) = |tr(U_goal' U)| / n over the subspace block (`iso_vec_unitary_fidelity(U_T, U_G, subspace=...)`,
 * reference unitary_minimum_time_problem.jl:77) and the loss l = |1 - F| of `UnitaryInfidelityObjective`
 * (docstring unitary_smooth_pulse_problem.jl:23-28); `FinalUnitaryFidelityConstraint` (:80-84) is F - F_min >= 0.
 * grad: dF/dU~ (length 2N^2); hess: d2F/dU~2, dense upper triangle, column-major (entry (i<=j) at j(j+1)/2 + i).
 * For the loss: grad l = -sign(1-F) grad F, hess l = -sign(1-F) hess F.  The normalisation (|tr|/n) follows the
 * docstring; PiccoloQuantumObjects 0.3's own definition could not be inspected. */
typedef struct qc_fidelity qc_fidelity;
int qc_fidelity_create(int32_t N, const double* goal_iso, const int32_t* subspace /* 0-based, or NULL */, int32_t n_sub,
                       int32_t device, qc_fidelity** out);
/* Ket and density-operator states (quantum_state_smooth_pulse_problem.jl:133 `QuantumStateObjective`,
 * quantum_state_minimum_time_problem.jl:50-62 `iso_fidelity` / `FinalQuantumStateFidelityConstraint`,
 * density_operator_smooth_pulse_problem.jl:55 `DensityOperatorPureStateInfidelityObjective`):
 *   QC_FID_KET      state psi~ (2N),      F = |<psi_goal|psi>|^2
 *   QC_FID_DENSITY  state rho~ (2N^2),    F = psi_goal' rho psi_goal   (linear)
 * goal_ket_iso = [Re psi_goal; Im psi_goal] in both cases; loss |1 - F|, gradients / Hessians as for the unitary kind. */
#define QC_FID_UNITARY 0
#define QC_FID_KET 1
#define QC_FID_DENSITY 2
int qc_fidelity_create_kind(int32_t kind, int32_t N, const double* goal_ket_iso, int32_t device, qc_fidelity** out);
/* Descriptor form: everything above plus the two choices that PiccoloQuantumObjects 0.3 (not vendored) makes and this
 * repository cannot inspect, and the free-phase fidelity of the minimum-time / smooth-pulse templates:
 *   form      QC_FID_FORM_ABS   F = |tr(U_goal' U)| / n      (the reference's docstring, unitary_smooth_pulse_problem.jl:23-28; default)
 *             QC_FID_FORM_ABS2  F = |tr(U_goal' U)|^2 / n^2
 *   n_phases  K > 0: `iso_vec_unitary_free_phase_fidelity(U, U_goal, phases, phase_operators; subspace)` and
 *             `FinalUnitaryFreePhaseFidelityConstraint` (unitary_minimum_time_problem.jl:86-100, phases = global
 *             variables `traj.global_data[phase_name]`, trajectory_initialization.jl:370-380):
 *                 F(U, phi) = |tr(U_goal' R(phi) U)| / n,   R(phi) = (x)_k exp(i phi_k Op_k)   (Julia's reduce(kron, ...)),
 *             Op_k Hermitian d_k x d_k with prod d_k = subspace size (Paulis Z for virtual-Z corrections,
 *             unitary_smooth_pulse_problem.jl:345-346).  The evaluation input is then [U~ (2N^2) ; phi (K)], gradient and
 *             Hessian cover all 2N^2 + K variables (qc_fidelity_input_len). */
#define QC_FID_FORM_ABS 0
#define QC_FID_FORM_ABS2 1
typedef struct qc_fidelity_desc {
    int32_t kind;               /* QC_FID_UNITARY | QC_FID_KET | QC_FID_DENSITY (subspace / form / phases: unitary only) */
    int32_t N;
    const double* goal_iso;     /* unitary: iso-vec of U_goal (2N^2); ket / density: [Re psi_goal; Im psi_goal] */
    const int32_t* subspace;    /* 0-based level indices, or NULL = all levels */
    int32_t n_sub;
    int32_t form;               /* QC_FID_FORM_* */
    int32_t n_phases;           /* K, 0..16 */
    int32_t device;
    const int32_t* phase_dims;  /* K dimensions d_k */
    const double* phase_ops;    /* operator k after operator k-1: d_k x d_k real plane, then d_k x d_k imaginary plane, column-major */
} qc_fidelity_desc;
int qc_fidelity_create_desc(const qc_fidelity_desc* d, qc_fidelity** out);
int32_t qc_fidelity_input_len(const qc_fidelity* h);   /* 2N^2 + K (state length for kets / density operators) */
void qc_fidelity_destroy(qc_fidelity* h);
const char* qc_fidelity_last_error(const qc_fidelity* h);
/* host buffers; any of fidelity / infidelity / grad / hess may be NULL */
int qc_fidelity_eval(qc_fidelity* h, const double* U_iso, double* fidelity, double* infidelity, double* grad, double* hess);
/* device buffers, asynchronous on `stream`: dval2 = {F, |1-F|}; dgrad / dhess may be NULL */
int qc_fidelity_eval_dev(qc_fidelity* h, const double* dU, double* dval2, double* dgrad, double* dhess, void* stream);

/* ---- rollouts (SURVEY 8f "next" row 4) -------------------------------------------------------------- */
/* x_{t+1} = exp(dt_t G(a_t)) x_t for t = 0 .. T-2 from x_0 = init (2N x cols, column-major), controls and timesteps read
 * from Z at the handle's offsets; out receives the (2N cols) x T state matrix, one column per knot: `unitary_rollout`,
 * `rollout`, `open_rollout` (reference call sites trajectory_initialization.jl:426,493,547; `unitary_rollout_fidelity`,
 * unitary_smooth_pulse_problem.jl:218, is this followed by qc_fidelity_eval on the last column).  The propagator is the
 * matrix exponential whatever integrator the handle was created with (the reference's default `expv`); the whole
 * trajectory is covered whatever the handle's shard.  2N <= 64. */
int qc_rollout(qc_handle* h, const double* Z, const double* init, double* out);
int qc_rollout_dev(qc_handle* h, const double* dZ, const double* dinit, double* dout, void* stream);

/* ---- trajectory cost terms (SURVEY 8f "next" row 3) ----------------------------------------------- */
/* J(Z) = sum_t 1/2 sum_k R_k (sc_t (v_tk - b_tk))^2 + D sum_{t < min_time_knots} dt_t,   sc_t = 1 (default) or dt_t:
 * the `QuadraticRegularizer(name, traj, R; baseline, timestep_name)` terms on a / da / dda (reference call sites
 * unitary_smooth_pulse_problem.jl:151-153) flattened into one list of regularised scalar entries of a knot, plus
 * `MinimumTimeObjective(traj; D)` (unitary_minimum_time_problem.jl:67-69; the last knot's timestep drives no
 * interval, hence min_time_knots = T-1 there).  QC_REG_DT_SCALED (2, the default of every binding) puts the timestep
 * inside the square: every problem template hands the regulariser the timestep's name
 * (`QuadraticRegularizer(name, traj, R; timestep_name=timestep_name)`, unitary_smooth_pulse_problem.jl:151-153,
 * unitary_sampling_problem.jl:116-118, quantum_state_sampling_problem.jl:82-84), which only a definition that reads dt_t
 * needs, and that is how QuantumCollocationCore 0.3 is recalled to define it (not vendored, SURVEY 8c;
 * julia/reconcile.jl settles it).  QC_REG_PLAIN (3) is the docstring's "1/2 sum_t R_a a_t^2 + ..."
 * (unitary_smooth_pulse_problem.jl:13).  The values 0 and 1 are RETIRED (ABI 0.1 - 0.3 gave them both meanings in turn): a
 * descriptor that carries one of them is refused with QC_ERR_INVALID, so a binding built against an older header fails loudly
 * instead of computing the other regulariser; bindings also compare qc_abi_version() at load time.
 * Gradient: dense, Z_len entries (zeros included).  Hessian: upper triangle, per knot
 * [ (v_k,v_k) k=0..n_reg-1 | (v_k,dt) k=0..n_reg-1 | (dt,dt) ]; the last two groups exist only for QC_REG_DT_SCALED
 * with a free timestep. */
#define QC_REG_DT_SCALED 2
#define QC_REG_PLAIN 3
typedef struct qc_terms_desc {
    int64_t T;
    int32_t zdim;
    int32_t off_dt;              /* offset of the timestep inside a knot, -1: fixed */
    int64_t global_dim;
    double dt_fixed;
    int32_t n_reg;               /* number of regularised scalar entries of a knot */
    int32_t weighting;           /* QC_REG_DT_SCALED | QC_REG_PLAIN */
    const int32_t* reg_index;    /* n_reg offsets inside a knot, strictly increasing, != off_dt */
    const double* reg_R;         /* n_reg weights */
    const double* reg_baseline;  /* NULL, or n_reg x T (entry-fastest) values subtracted before squaring */
    double min_time_D;           /* 0: no minimum-time term */
    int64_t min_time_knots;      /* timesteps of knots 0..min_time_knots-1 are summed */
    int32_t device;
    int32_t reserved0;
} qc_terms_desc;
typedef struct qc_terms qc_terms;
int qc_terms_desc_hess_nnz(const qc_terms_desc* d, int64_t* nnz);
int qc_terms_desc_hess_structure(const qc_terms_desc* d, int64_t* rows, int64_t* cols, int one_based);
int qc_terms_create(const qc_terms_desc* d, qc_terms** out);
void qc_terms_destroy(qc_terms* h);
const char* qc_terms_last_error(const qc_terms* h);
int qc_terms_hess_nnz(const qc_terms* h, int64_t* nnz);
int qc_terms_hess_structure(const qc_terms* h, int64_t* rows, int64_t* cols, int one_based);
/* host buffers; J / grad / hvals may be NULL */
int qc_terms_eval(qc_terms* h, const double* Z, double* J, double* grad, double* hvals);
/* device buffers, asynchronous on `stream`; dgrad / dhvals may be NULL */
int qc_terms_eval_dev(qc_terms* h, const double* dZ, double* dJ, double* dgrad, double* dhvals, void* stream);
/* Extension terms of the same pass (x_t[j] = entry j of knot t, sc_t as above):
 *   smoothness  1/2 sum_{t<T-1} sum_k R_k (x_{t+1}[s_k] - x_t[s_k])^2       `QuadraticSmoothnessRegularizer(name, traj, R)`
 *                (no timestep inside the square; unitary_smooth_pulse_problem.jl:311-340)
 *   pairwise    sum_t sum_p 1/2 Q_p sc_t^2 (x_t[a_p] - x_t[b_p])^2          `PairwiseQuadraticRegularizer(traj, Q, graph)`
 *                (unitary_direct_sum_problem.jl:130-169; the edges of the graph flattened into scalar pairs, one Q per pair)
 *   linear      sum_t sum_k w_k x_t[l_k]                                     the cost of `L1Regularizer!` on its slack entries
 *                (_problem_templates.jl:41-54); the slack rows and s >= 0 stay with the caller
 * All three are how QuantumCollocationCore 0.3 is recalled to define them (not vendored; julia/reconcile.jl).
 * Indices lie inside the knot and are not the timestep; s_k and l_k do not repeat; a_p != b_p; an entry may appear in the
 * regulariser list, the smoothness list and any number of pairs at once (gradient and Hessian are the sums).
 * Hessian: the layout above is an exact prefix; after it come
 *   smoothness  per knot t: [ (s_k,s_k) k=0..n_smooth-1 | (x_t[s_k], x_{t+1}[s_k]) k=0..n_smooth-1 (t < T-1 only) ],
 *               n_smooth (2T - 1) values
 *   pairwise    per knot: [ (a_p,a_p) | (b_p,b_p) | (min(a_p,b_p), max(a_p,b_p)) | (a_p,dt) | (b_p,dt) | (dt,dt) ], p = 0..n_pair-1
 *               in each group; the last three groups exist only for QC_REG_DT_SCALED with a free timestep
 * all upper-triangular (row <= col).  Entries repeat across blocks; a consumer sums duplicates (as MOI specifies).
 * A NULL extension, or one with all three counts zero, gives a handle identical to qc_terms_create. */
typedef struct qc_terms_ext {
    int32_t n_smooth;
    int32_t n_pair;
    int32_t n_lin;
    int32_t reserved0;
    const int32_t* smooth_index; /* n_smooth offsets inside a knot */
    const double* smooth_R;      /* n_smooth weights */
    const int32_t* pair_a;       /* n_pair offsets inside a knot */
    const int32_t* pair_b;       /* n_pair offsets inside a knot, pair_b[p] != pair_a[p] */
    const double* pair_Q;        /* n_pair weights */
    const int32_t* lin_index;    /* n_lin offsets inside a knot */
    const double* lin_w;         /* n_lin weights */
    int64_t reserved1[2];
} qc_terms_ext;
int64_t qc_sizeof_terms_ext(void);
int qc_terms_desc_ext_hess_nnz(const qc_terms_desc* d, const qc_terms_ext* ext, int64_t* nnz);
int qc_terms_desc_ext_hess_structure(const qc_terms_desc* d, const qc_terms_ext* ext, int64_t* rows, int64_t* cols, int one_based);
int qc_terms_create_ext(const qc_terms_desc* d, const qc_terms_ext* ext, qc_terms** out);

/* ---- robustness objective (UnitaryRobustnessObjective, reference unitary_robustness_problem.jl:46-49) ---------------- */
/* A whole-trajectory term over the subspace block V_t = U_t[S, S] (n x n) of every knot t < K (n_knots):
 *     A_t = V_t' H V_t,   tau = sum_{t<K} dt_t,   R = (1/tau) sum_{t<K} dt_t A_t,   L = Re tr(R'R) / n
 * with H the n x n error operator (`unembed(H_error)`; complex, need not be Hermitian).  Its variables are the 2n^2 subspace
 * entries of the unitary of every knot t < K, plus each such knot's timestep when off_dt >= 0: V = K (2n^2 [+1]), listed in
 * increasing global index by qc_robust_vars.  Gradient: dense, Z_len entries (zeros included).  Hessian
 * (QC_ROBUST_HESS_EXACT): dense over the V variables, the column-major upper triangle -- entry (i <= j) at j(j+1)/2 + i --
 * refused with QC_ERR_UNSUPPORTED when V(V+1)/2 > 2^27.  2N <= 64.  The mathematics: the header comment of qc_robust.hip. */
#define QC_ROBUST_HESS_NONE 0
#define QC_ROBUST_HESS_EXACT 1
typedef struct qc_robust_desc {
    int64_t T;
    int32_t zdim;
    int32_t off_state;           /* offset of the unitary's iso-vec (2N^2 entries) inside a knot */
    int32_t N;
    int32_t n_sub;               /* subspace size n (0 with subspace = NULL: all N levels) */
    const int32_t* subspace;     /* n distinct 0-based levels, or NULL */
    const double* H_re;          /* n x n, column-major */
    const double* H_im;          /* n x n, column-major, or NULL (real H) */
    int32_t off_dt;              /* offset of the timestep inside a knot, -1: fixed */
    int32_t reserved0;
    double dt_fixed;
    int64_t global_dim;
    int64_t n_knots;             /* K, 1 .. T: knots 0 .. K-1 enter the sum */
    int32_t hessian;             /* QC_ROBUST_HESS_NONE | QC_ROBUST_HESS_EXACT */
    int32_t device;
    int64_t reserved1[2];
} qc_robust_desc;
typedef struct qc_robust qc_robust;
/* device-free: validate the descriptor (QC_ERR_INVALID with a message) and describe the term */
int qc_robust_desc_n_vars(const qc_robust_desc* d, int64_t* n_vars);
int qc_robust_desc_vars(const qc_robust_desc* d, int64_t* vars);
int qc_robust_desc_hess_nnz(const qc_robust_desc* d, int64_t* nnz);
int qc_robust_desc_hess_structure(const qc_robust_desc* d, int64_t* rows, int64_t* cols, int one_based);
int64_t qc_sizeof_robust_desc(void);
int qc_robust_create(const qc_robust_desc* d, qc_robust** out);
void qc_robust_destroy(qc_robust* h);
const char* qc_robust_last_error(const qc_robust* h);
int qc_robust_n_vars(const qc_robust* h, int64_t* n_vars);
int qc_robust_vars(const qc_robust* h, int64_t* vars);
int qc_robust_hess_nnz(const qc_robust* h, int64_t* nnz);
int qc_robust_hess_structure(const qc_robust* h, int64_t* rows, int64_t* cols, int one_based);
/* host buffers; L / grad / hvals may be NULL */
int qc_robust_eval(qc_robust* h, const double* Z, double* L, double* grad, double* hvals);
/* device buffers, asynchronous on `stream` (no host synchronisation; scratch owned by the handle); dL / dgrad / dhvals may be NULL */
int qc_robust_eval_dev(qc_robust* h, const double* dZ, double* dL, double* dgrad, double* dhvals, void* stream);

/* ---- rollout sweeps: final states and fidelities over perturbed systems ------------------------------------------------ */
/* One trajectory of controls, S systems that differ by a few parameters, one call: the loop of the reference's robustness check
 * (unitary_sampling_problem.jl:204-244: `unitary_rollout(traj.a, timesteps, systems(zeta))[:, end]` and `iso_vec_unitary_fidelity`
 * for every zeta of a grid; `UnitarySamplingProblem(system::Function, distribution, num_samples, ...)`, :186-200, draws its systems
 * the same way).  Sample s is the base system plus n_pert additive perturbation generators, with a factor per drive:
 *     G_s(a) = G_drift + sum_{j < n_pert} theta[s, j] P_j + sum_{k < m} c[s, k] a_k G_k
 *     x_{t+1} = exp(dt_t G_s(a_t)) x_t,   t = 0 .. T-2,   x_0 = init (2N x cols, column-major)
 * theta: S x n_pert, sample-major; c (`scale`): S x m, sample-major, or NULL = all ones.  The reference's systems(zeta) is
 * G_drift = 0, P_0 = iso(-i Z), theta[s, 0] = zeta_s; a relative amplitude error eps on drive k is c[s, k] = 1 + eps.  The matrices
 * are whatever the caller passes, as in qc_desc: iso generators of Hamiltonians, or Lindblad generators with N = levels^2
 * (`open_rollout`).  The propagator is the matrix exponential, as in qc_rollout.  Only the controls and timesteps are read from Z.
 * Kernels: 2N <= 16 with up to 8 drives runs on the f64 matrix cores, one wavefront per (sample, chunk of intervals)
 * ("mfma16-sweep"); larger systems run the rollout kernels once per sample ("rollout-per-sample": correctness, not speed).
 * With wide = QC_SWEEP_WIDE the matrix cores serve 16 < 2N <= 32 (up to 8 drives) as well ("mfma32-sweep": 2 x 2 tiles a matrix, the same
 * work item and chunk rule); 2N <= 16 is "mfma16-sweep" as before, everything else the per-sample form.  wide = 0 is the routing of the
 * two sentences above, unchanged.  wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_PARAMS (3) is wide = QC_SWEEP_WIDE in every respect but one:
 * an "mfma32-sweep" handle then serves the parameter gradients (qc_sweep_grad_params*) and the parameter cotangents of the pullback
 * (qc_sweep_vjp*: grad_theta, grad_scale).  Bit 3, QC_SWEEP_WIDE_STORED (wide = 9, or 11 with the parameter bit), likewise changes one
 * thing only: an "mfma32-sweep" handle whose descriptor also sets reserved1[0] = QC_SWEEP_STORED_STATES then serves reverse mode by the
 * stored-state walk on 2 x 2 tiles (below); without reserved1[0], or where the handle takes another form, the bit does nothing.  Bit 4,
 * QC_SWEEP_WIDE_TANGENT (wide = 17, 19, 25 or 27), likewise changes one thing only: an "mfma32-sweep" handle then serves the pushforward
 * (qc_sweep_jvp*, below) with any generators; the forward sweep, gradients, pullbacks, the launch and the kernel name are untouched, and
 * where the handle takes another form the bit does nothing.  Bit 6, QC_SWEEP_WIDE_NOISE (any of the odd values | 64), likewise changes
 * one thing only: an "mfma32-sweep" handle then serves the noise-trajectory sweeps and their gradients (qc_sweep_noise_*, below); form,
 * launch, kernel name, every other *_supported answer and every other entry point's output are bit-identical to the same descriptor
 * without the bit, and where the handle takes another form (2N <= 16 with its own noise kernels and tile rule, rollout-per-sample) the bit
 * does nothing.  Bit 8, QC_SWEEP_WIDE_HESSIAN (any of the sixteen odd values | 256), likewise changes one thing only: an "mfma32-sweep"
 * handle whose descriptor passes the closed scope (antisymmetric drift / drives / perturbations, at most 16 state columns) then serves the
 * Hessian product (qc_sweep_hvp*, below; qc_sweep32_hvp.hip).  It does not need QC_SWEEP_WIDE_TANGENT: the call launches the tangent
 * totals itself.  Form, launch, kernel name, every other *_supported answer and every other entry point's output are bit-identical to the
 * same descriptor without the bit, and at 2N <= 16 (whose Hessian product needs no bit) and in the rollout-per-sample form it does nothing.
 * The valid values are 0, 1, 3, 9, 11, 17, 19, 25 and 27, each of the eight odd ones | 64 (65 .. 91), and each of those sixteen odd
 * values | 256; any other value (bit 1, 3, 4, 6 or 8 without bit 0, bit 2, 5 and 7 among them) is QC_ERR_INVALID.
 * Bit 10, QC_SWEEP_WIDE_64 (any of those thirty-two odd values | 1024; 1024 alone and bit 9 are QC_ERR_INVALID), takes the matrix cores
 * up to 2N = 64: a descriptor with 32 < 2N <= 64 and up to 16 drives (5 qubits: N = 32 with 10 drives; three coupled three-level
 * transmons: 2N = 54; a Lindblad model of a five-level system: N = 25) then takes a third matrix-core form, "mfma64-sweep"
 * (qc_sweep64.hip): 4 x 4 tiles a matrix, the matrices in LDS, one WORKGROUP of 16 wavefronts per (sample, chunk of intervals), and the
 * chunk rule with that item's fill constant (n_chunks = 1 once S >= 256, one workgroup per compute unit; else ceil(256 / S) chunks, at
 * most ceil(sqrt(T-1))).  The mathematics is the family's.  That form serves the FORWARD sweep only, qc_sweep_eval*: final states
 * and fidelities.  qc_sweep_grad*, qc_sweep_grad_params*, qc_sweep_vjp*, qc_sweep_jvp*, qc_sweep_hvp* and qc_sweep_noise_* return
 * QC_ERR_UNSUPPORTED on such a handle, whatever bits 1 .. 8 say (bit 11, below, adds gradients and pullbacks, bit 14 pushforwards, bit 16 noise sweeps), and the qc_sweep_desc_*_supported queries answer 0 with a reason
 * that names the form and the size ("... the mfma64-sweep form (2N = 54) ...").  Descriptors with 2N <= 32 ignore the bit completely:
 * form, launch, kernel name, every *_supported answer and every output bit are those of the same descriptor without it.  Without the
 * bit nothing changes anywhere.  Not in that form: more than 16 drives (rollout-per-sample), a state-action form that skips the
 * propagator for kets, 2N > 64 (QC_ERR_UNSUPPORTED as before).
 * Bit 11, QC_SWEEP_WIDE_64_GRAD (any valid value that has bits 0 and 10, | 2048; without both of them QC_ERR_INVALID), changes one thing
 * only: an "mfma64-sweep" handle then also serves qc_sweep_grad* (fids, J, grad, grad_samples) and qc_sweep_vjp* (finals, grad,
 * grad_samples, grad_init) of CLOSED systems -- antisymmetric generators, the same 64-eps test -- with states of up to 32 columns, by the
 * closed adjoint walk on 4 x 4 tiles (qc_sweep64_grad.hip; one workgroup per (sample, chunk), the forward form's chunk rule).  The
 * fidelities and final states carry the bits of qc_sweep_eval on the same handle.  Still QC_ERR_UNSUPPORTED there, with a reason that
 * names the form and 2N: parameter gradients and parameter cotangents, reserved1[0] = QC_SWEEP_STORED_STATES, qc_sweep_jvp* (served
 * with bit 14, below), qc_sweep_hvp* and qc_sweep_noise_* (served with bit 16, below).  Form, launch, kernel name and every output bit of qc_sweep_eval* are those of the same descriptor
 * without the bit; descriptors with 2N <= 32 ignore it completely, as they ignore bit 10.
 * Bit 13, QC_SWEEP_WIDE_64_PARAMS (any valid value that has bits 0, 10 and 11, | 8192; without all three of them QC_ERR_INVALID; bit 12
 * is not assigned), changes one thing only: such a handle then also serves qc_sweep_grad_params* (grad_theta, grad_scale) and the
 * grad_theta / grad_scale of qc_sweep_vjp*, in the scope of bit 11, by the parameter flavour of the same walk (per (sample, chunk) the
 * p + m chunk shares in a fixed order, then the reduction of the smaller forms; no atomics).  The other outputs of a parameter call carry
 * the bits of qc_sweep_grad / qc_sweep_vjp on the same handle, and a call without parameter outputs launches exactly what it launched
 * without the bit.  The stored-state flag, qc_sweep_jvp* (served with bit 14), qc_sweep_hvp* and qc_sweep_noise_* (served with bit 16) stay QC_ERR_UNSUPPORTED
 * there; descriptors with 2N <= 32 ignore the bit completely.
 * Bit 14, QC_SWEEP_WIDE_64_TANGENT (any valid value that has bits 0 and 10, | 16384; without both of them QC_ERR_INVALID; it needs
 * neither bit 11 nor bit 13, because nothing is reversed), changes one thing only: an "mfma64-sweep" handle then also serves qc_sweep_jvp*
 * (finals, fids, tfinals, tfids along vZ, vinit, vtheta, vscale) with ANY generators, Lindblad ones included (N = 25: 2N = 50), any
 * fid_kind, for states of ns = 2N x state_cols <= 2048 entries -- every full unitary of the form (N = 32: 2048), and more columns than
 * reverse mode's 32 below the bound (N = 17 with 33 columns) -- by the paired exponential on 4 x 4 tiles (qc_sweep64_jvp.hip; one
 * workgroup per (sample, chunk), the forward form's chunk rule) and the finish kernel of qc_sweep_jvp.hip at ld = 64, whose LDS sets the
 * bound; above it QC_ERR_UNSUPPORTED with a reason that names the form, 2N and ns.  finals / fids carry the bits of qc_sweep_eval on the
 * same handle.  With bits 11 and 13 as well the pullback and the pushforward together give Gauss-Newton products.  qc_sweep_hvp*,
 * qc_sweep_noise_* (served with bit 16, below) and the stored-state flag stay QC_ERR_UNSUPPORTED there.  Form, launch, kernel name, every other *_supported answer and
 * every other entry point's output are those of the same descriptor without the bit; descriptors with 2N <= 32 ignore it completely.
 * Bit 16, QC_SWEEP_WIDE_64_NOISE (any valid value that has bits 0 and 10, | 65536; without both of them QC_ERR_INVALID; it needs none of
 * bits 11, 13 and 14; bits 15 and 20 are not assigned), changes one thing only: an "mfma64-sweep" handle then also serves the
 * noise-trajectory sweeps (qc_sweep_noise_*, below; qc_sweep64_noise.hip) with m <= 16 drives and 1 <= n_pert <= 8 perturbations, up to
 * 24 generators (nothing is resident per generator there: no tile limit).  qc_sweep_noise_eval* serves ANY generators, Lindblad ones
 * included, any fid_kind or none and any state_cols the forward sweep serves; qc_sweep_noise_grad* needs the gradient's closed scope
 * of this form as well -- bit 11, antisymmetric generators, at most 32 state columns, a unitary or ket fidelity -- and without it answers
 * QC_ERR_UNSUPPORTED with the gradient's own reason.  At noise = +0.0 the outputs carry the bits of qc_sweep_eval / qc_sweep_grad on the
 * same handle.  qc_sweep_hvp* and the stored-state flag stay QC_ERR_UNSUPPORTED there.  Form, launch, kernel name, every other
 * *_supported answer and every other entry point's output are those of the same descriptor without the bit; descriptors with 2N <= 32
 * ignore it completely.
 * Bit 18, QC_SWEEP_WIDE_64_STORED (any valid value that has bits 0, 10 and 11, | 262144; without all three of them QC_ERR_INVALID, as
 * bit 13; bit 17 and everything from bit 19 up are not assigned), matters only on an "mfma64-sweep" handle that also has reserved1[0] =
 * QC_SWEEP_STORED_STATES: qc_sweep_grad* and qc_sweep_vjp* then serve ANY generators there -- a Lindblad model of a five-level system
 * (N = 25, 2N = 50) with QC_FID_DENSITY, non-Hermitian effective Hamiltonians -- with states of up to 32 columns, by the stored-state walk
 * on 4 x 4 tiles (qc_sweep64_open_grad.hip: a store launch and a walk, one workgroup per (sample, chunk) each, the forward form's chunk
 * rule); such a handle takes that walk whatever its generators, antisymmetric ones included.  qc_sweep_grad_params* and the grad_theta /
 * grad_scale of qc_sweep_vjp* are served when bit 13 is set as well and keep their refusal without it.  The state buffer is
 * S x (T-1) x 2N x cols doubles: 50 doubles a knot for the five-level Lindblad state, 432 for eight columns at 27 levels.  fids / finals
 * carry the bits of qc_sweep_eval on the same handle.  Still refused there: qc_sweep_hvp* (Hessian products are not served in this form),
 * qc_sweep_noise_grad* of open systems (it keeps its closed scope and its kernels) and states of more than 32 columns.  Without the bit
 * the stored-state flag stays QC_ERR_UNSUPPORTED in this form, message for message; qc_sweep_eval*, qc_sweep_jvp*, qc_sweep_noise_eval*
 * and the launch rule do not look at the bit; descriptors with 2N <= 32 ignore it completely.
 * reserved1[0] = QC_SWEEP_STORED_STATES chooses reverse mode by the STORED-STATE walk: qc_sweep_grad*, qc_sweep_grad_params* and
 * qc_sweep_vjp* then keep the forward states x_0 .. x_{T-2} of every sample in handle scratch (S x (T-1) x 2N x cols doubles) and read
 * them on the way back instead of reversing the step, which serves ANY generators in the "mfma16-sweep" form: Lindblad generators
 * (N = levels^2) with QC_FID_DENSITY, non-Hermitian effective Hamiltonians.  The "mfma32-sweep" form (two qubits with T1 / T2: levels^2 = 16,
 * 2N = 32; a three-level transmon: 2N = 18) serves it for descriptors that also set QC_SWEEP_WIDE_STORED in `wide`.  The buffer is
 * S x (T-1) x 2N x cols doubles: 32 doubles a knot for a two-qubit Lindblad state (250 MiB at S = 1024, T = 1000), 512 doubles a knot
 * for a 16-level unitary (4 GiB at S = 1024, T = 1000); an allocation that fails is QC_ERR_HIP, and the handle stays usable.  A handle with the flag takes that walk whatever its
 * generators, antisymmetric ones included.  reserved1[0] = 0 is everything as it was, bit for bit; any other value is QC_ERR_INVALID;
 * reserved1[1] is ignored.  qc_sweep_eval*, qc_sweep_jvp*, qc_sweep_noise_eval* do not look at the flag, and qc_sweep_hvp* /
 * qc_sweep_noise_grad* keep their scope (antisymmetric generators) and their kernels with it.
 * Results do not depend on scheduling: repeated calls return the same bits.  Non-finite inputs are evaluated, not rejected.
 * Gradients with respect to the controls and timesteps (qc_sweep_grad*) and to the samples' own parameters theta and `scale`
 * (qc_sweep_grad_params*), both below, are served for closed systems in the MFMA forms (parameter gradients: "mfma16-sweep", "mfma32-sweep" with QC_SWEEP_WIDE_PARAMS, "mfma64-sweep" with QC_SWEEP_WIDE_64_PARAMS), and
 * with reserved1[0] = QC_SWEEP_STORED_STATES for open systems in the "mfma16-sweep" form and, with QC_SWEEP_WIDE_STORED, the "mfma32-sweep" form.
 * ("mfma64-sweep": with QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_STORED.)
 * Derivatives of the final states themselves, contracted with cotangents the caller chooses (qc_sweep_vjp*, below), carry any function
 * of the final states: leakage, the free-phase fidelity, several kets at once, a loss written elsewhere.
 * The forward-mode counterpart, the tangent of the final states and fidelities along one direction (qc_sweep_jvp*, below), is served
 * for "mfma16-sweep" handles, for "mfma32-sweep" handles whose `wide` has QC_SWEEP_WIDE_TANGENT, and for "mfma64-sweep" handles whose
 * `wide` has QC_SWEEP_WIDE_64_TANGENT (states of at most 2048 entries), with any generators, Lindblad ones
 * included (no flag, no state buffer: nothing is reversed); with the pullback it gives Gauss-Newton products of any loss.
 * The tangent of the pullback along one direction (qc_sweep_hvp*, below) gives exact Hessian products of any loss of the final states
 * where both of them are served (closed systems; "mfma16-sweep", and "mfma32-sweep" handles whose `wide` has QC_SWEEP_WIDE_HESSIAN).
 * Noise-trajectory sweeps (qc_sweep_noise_*, below) are served for "mfma16-sweep" handles, for "mfma32-sweep" handles whose `wide` has
 * QC_SWEEP_WIDE_NOISE, and for "mfma64-sweep" handles whose `wide` has QC_SWEEP_WIDE_64_NOISE.
 * Out of scope: per-knot outputs, open-system gradients in the "mfma32-sweep" form without QC_SWEEP_WIDE_STORED (their directional
 * derivatives are not served there at all), checkpointing inside a chunk, Hessian products and noise gradients of open
 * systems, pushforwards on "mfma32-sweep" and "rollout-per-sample" handles (the former unless `wide` has QC_SWEEP_WIDE_TANGENT), Hessian
 * products on "rollout-per-sample" handles and on "mfma32-sweep" handles without QC_SWEEP_WIDE_HESSIAN, several directions per
 * call, tangents of grad_theta / grad_scale, several devices; in the "mfma64-sweep" form everything but the forward sweep, with
 * QC_SWEEP_WIDE_64_GRAD gradients and pullbacks of closed systems, with QC_SWEEP_WIDE_64_PARAMS their parameter outputs and with
 * QC_SWEEP_WIDE_64_TANGENT pushforwards of states of at most 2048 entries and with QC_SWEEP_WIDE_64_NOISE noise sweeps (Hessian products
 * are not served in that form). */
#define QC_MAX_PERT 8
#define QC_SWEEP_FID_NONE (-1)   /* qc_sweep_desc.fid_kind: final states only */
#define QC_SWEEP_WIDE 1          /* qc_sweep_desc.wide, bit 0 */
#define QC_SWEEP_WIDE_PARAMS 2   /* qc_sweep_desc.wide, bit 1: the mfma32-sweep form serves parameter gradients and parameter cotangents; only together with QC_SWEEP_WIDE */
#define QC_SWEEP_WIDE_STORED 8   /* qc_sweep_desc.wide, bit 3: the mfma32-sweep form serves the stored-state walk; only together with QC_SWEEP_WIDE */
#define QC_SWEEP_WIDE_TANGENT 16 /* qc_sweep_desc.wide, bit 4: the mfma32-sweep form serves pushforwards (qc_sweep_jvp*); only together with QC_SWEEP_WIDE */
#define QC_SWEEP_WIDE_NOISE 64   /* qc_sweep_desc.wide, bit 6: the mfma32-sweep form serves noise-trajectory sweeps and their gradients (qc_sweep_noise_*); only together with QC_SWEEP_WIDE */
#define QC_SWEEP_WIDE_HESSIAN 256 /* qc_sweep_desc.wide, bit 8: the mfma32-sweep form serves Hessian products of closed systems (qc_sweep_hvp*); only together with QC_SWEEP_WIDE */
#define QC_SWEEP_WIDE_64_GRAD 2048 /* qc_sweep_desc.wide, bit 11: the mfma64-sweep form serves sweep gradients and pullbacks of closed systems (qc_sweep_grad*, qc_sweep_vjp*; qc_sweep64_grad.hip); ignored at 2N <= 32; only together with QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 */
#define QC_SWEEP_WIDE_64_PARAMS 8192 /* qc_sweep_desc.wide, bit 13: the mfma64-sweep form serves parameter gradients and parameter cotangents of closed systems (qc_sweep_grad_params*, grad_theta / grad_scale of qc_sweep_vjp*; the flavour <true> of qc_sweep64_grad.hip's walk); ignored at 2N <= 32; only together with QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD */
#define QC_SWEEP_WIDE_64_TANGENT 16384 /* qc_sweep_desc.wide, bit 14: the mfma64-sweep form serves pushforwards (qc_sweep_jvp*; qc_sweep64_jvp.hip), any generators, 2N x state_cols <= 2048; ignored at 2N <= 32; only together with QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 */
#define QC_SWEEP_WIDE_64_NOISE 65536 /* qc_sweep_desc.wide, bit 16: the mfma64-sweep form serves noise-trajectory sweeps and, with QC_SWEEP_WIDE_64_GRAD, their gradients (qc_sweep_noise_*; qc_sweep64_noise.hip); ignored at 2N <= 32; only together with QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 */
#define QC_SWEEP_WIDE_64_STORED 262144 /* qc_sweep_desc.wide, bit 18: with reserved1[0] = QC_SWEEP_STORED_STATES the mfma64-sweep form serves the stored-state walk, any generators, at most 32 state columns (qc_sweep_grad*, qc_sweep_vjp*; qc_sweep64_open_grad.hip); ignored at 2N <= 32; only together with QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD */
#define QC_SWEEP_WIDE_64 1024    /* qc_sweep_desc.wide, bit 10: 32 < 2N <= 64 with up to 16 drives takes the matrix cores ("mfma64-sweep", qc_sweep_eval* only); ignored at 2N <= 32; only together with QC_SWEEP_WIDE */
#define QC_SWEEP_STORED_STATES 1 /* qc_sweep_desc.reserved1[0]: reverse mode by the stored-state walk */
typedef struct qc_sweep_desc {
    int64_t T;
    int32_t zdim;
    int32_t off_a;               /* offset of the controls (m entries) inside a knot */
    int32_t off_dt;              /* offset of the timestep inside a knot, -1: fixed */
    int32_t N;                   /* iso dimension n = 2N */
    double dt_fixed;
    int64_t global_dim;
    int32_t m;                   /* drives */
    int32_t state_cols;          /* as qc_desc.state_cols: 0 or N = a unitary (2N x N); K >= 1 = K kets (2N x K) */
    int32_t n_pert;              /* 0 .. QC_MAX_PERT */
    int32_t fid_kind;            /* QC_SWEEP_FID_NONE | QC_FID_UNITARY | QC_FID_KET (state_cols = 1) | QC_FID_DENSITY (state_cols = 1, N = levels^2) */
    const double* G_drift;       /* n x n, column-major */
    const double* G_drives;      /* m matrices of n x n */
    const double* G_pert;        /* n_pert matrices of n x n (NULL when n_pert = 0) */
    int32_t fid_form;            /* QC_FID_FORM_* (unitary only) */
    int32_t n_sub;
    const double* goal_iso;      /* as qc_fidelity_desc.goal_iso */
    const int32_t* subspace;     /* unitary only: 0-based levels, or NULL = all */
    int32_t device;
    int32_t wide;                /* bit field; valid: 0, QC_SWEEP_WIDE (1): the matrix-core form up to 2N = 32 ("mfma32-sweep"), or QC_SWEEP_WIDE | QC_SWEEP_WIDE_PARAMS (3): that form, and qc_sweep_grad_params* / the grad_theta, grad_scale of qc_sweep_vjp* are served in it (form, launch, kernel name and every *_supported answer as with 1; harmless where the handle takes another form); either of them | QC_SWEEP_WIDE_STORED (9, 11): that form also serves reverse mode by the stored-state walk when reserved1[0] = QC_SWEEP_STORED_STATES (nothing else changes); any of those | QC_SWEEP_WIDE_TANGENT (17, 19, 25, 27): that form also serves qc_sweep_jvp*; any of the eight | QC_SWEEP_WIDE_NOISE (64): that form also serves qc_sweep_noise_*; any of the sixteen | QC_SWEEP_WIDE_HESSIAN (256): that form also serves qc_sweep_hvp* for closed systems; any of the thirty-two | QC_SWEEP_WIDE_64 (1024): 32 < 2N <= 64 with m <= 16 takes the matrix-core form "mfma64-sweep" (forward sweep only), nothing changes at 2N <= 32; any of those | QC_SWEEP_WIDE_64_GRAD (2048): that form also serves qc_sweep_grad* and qc_sweep_vjp* of closed systems; any of those | QC_SWEEP_WIDE_64_PARAMS (8192): and their parameter outputs; any value that has QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_TANGENT (16384): that form also serves qc_sweep_jvp*, any generators; anything else is QC_ERR_INVALID */
    int64_t reserved1[2];        /* [0]: 0, or QC_SWEEP_STORED_STATES: reverse mode reads stored forward states (any generators; "mfma16-sweep", and "mfma32-sweep" with QC_SWEEP_WIDE_STORED in `wide`); anything else is QC_ERR_INVALID.  [1]: ignored */
} qc_sweep_desc;
typedef struct qc_sweep qc_sweep;
int64_t qc_sizeof_sweep_desc(void);
/* device-free: QC_ERR_INVALID with a message (qc_sweep_last_error(NULL)); QC_ERR_UNSUPPORTED for 2N > 64 */
int qc_sweep_desc_validate(const qc_sweep_desc* d);
/* device-free: the launch a handle of this descriptor takes for S samples -- mfma: 1 = "mfma16-sweep", "mfma32-sweep" or "mfma64-sweep", 0 = "rollout-per-sample";
 * chunk / n_chunks: intervals per wavefront ("mfma64-sweep": per workgroup) and chunks per sample of the MFMA form (n_chunks = 1 once S
 * alone fills the device, more for few samples; n_chunks = 0 for the per-sample form).  Outputs may be NULL. */
int qc_sweep_desc_launch(const qc_sweep_desc* d, int64_t S, int32_t* mfma, int64_t* chunk, int64_t* n_chunks);
int qc_sweep_create(const qc_sweep_desc* d, qc_sweep** out);
void qc_sweep_destroy(qc_sweep* h);
const char* qc_sweep_last_error(const qc_sweep* h);
/* "mfma16-sweep", "mfma32-sweep" (wide descriptors, 16 < 2N <= 32), "mfma64-sweep" (descriptors with QC_SWEEP_WIDE | QC_SWEEP_WIDE_64,
 * 32 < 2N <= 64, m <= 16) or "rollout-per-sample" (static strings; "none" for a NULL handle) */
const char* qc_sweep_kernel_name(const qc_sweep* h);
/* host buffers.  Z: the full trajectory vector (zdim T + global_dim); init: 2N x cols; theta: S x n_pert (NULL when n_pert = 0);
 * scale: S x m or NULL; finals: S x (2N cols), sample-major; fids: S values.  Either output may be NULL, not both. */
int qc_sweep_eval(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale, double* finals,
                  double* fids);
/* device buffers, asynchronous on `stream`, no host synchronisation -- except that scratch is owned by the handle and grown at the
 * first call that needs it: a call with a larger S than any before frees and allocates device memory, which synchronises the device
 * and cannot be captured in a graph (call once with the largest S first).  One evaluation in flight per handle.  The per-sample
 * form issues its launches (about six per sample) from a host loop inside the call. */
int qc_sweep_eval_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                      double* dfinals, double* dfids, void* stream);

/* ---- sweep gradients: the adjoint of the sweep -------------------------------------------------------------------------- */
/* dF_s/da_{t,k} and dF_s/ddt_t of every sample's fidelity, and J = sum_s w_s F_s with its dense gradient over Z.  One backward walk
 * with one Frechet-derivative chain per interval: the cost is a small constant times the forward sweep, whatever the number of drives.
 * Served where ALL of these hold; everything else returns QC_ERR_UNSUPPORTED with a message that names the reason:
 *   - the handle takes the "mfma16-sweep" form (2N <= 16, m <= 8) or, with wide = QC_SWEEP_WIDE, the "mfma32-sweep" form (2N <= 32, m <= 8);
 *   - fid_kind is QC_FID_UNITARY (either form, with or without subspace) or QC_FID_KET;
 *   - at most 16 state columns;
 *   - G_drift, every drive and every perturbation are antisymmetric, max |G + G^T| <= 64 eps max |G| (closed systems: iso generators
 *     of Hermitian operators; Lindblad generators are not).
 * With reserved1[0] = QC_SWEEP_STORED_STATES the scope is instead: the "mfma16-sweep" form (2N <= 16, m <= 8), at most 16 state columns,
 * a fidelity on the handle -- QC_FID_DENSITY included (F = Re t is linear: lambda_{T-1} = g_r) -- and ANY generators.  A wide handle
 * in the "mfma32-sweep" form with the flag is refused ("stored-state gradients are not served in the mfma32-sweep form") unless its
 * `wide` has QC_SWEEP_WIDE_STORED (9 or 11): then the same scope holds with 2N <= 32 (the 2 x 2-tile stored-state walk, whatever the
 * generators, antisymmetric ones included).
 * The last knot's controls and timestep enter no interval: their derivatives are exactly +0.0, as is every entry of `grad` that is
 * neither a control nor a timestep.  The |tr| / n form is not special-cased at tr = 0 (NaN there, as qc_fidelity_eval).
 * `fids` carry the bits of qc_sweep_eval; repeated calls return the same bits (no atomics, sums in a fixed order). */
/* device-free: *supported = 1 / 0; when 0, qc_sweep_last_error(NULL) says why.  An invalid descriptor returns its own error. */
int qc_sweep_desc_grad_supported(const qc_sweep_desc* d, int32_t* supported);
/* device buffers, asynchronous on `stream`.  weights: S values or NULL (= 1/S each); fids: S values or NULL; J: one double or NULL;
 * grad: zdim T + global_dim values or NULL; grad_samples: S x (T-1) x (m + (off_dt >= 0)), sample-major, per interval the drives then
 * the timestep, or NULL.  At least one output must be non-NULL.  Scratch and the one-in-flight rule as qc_sweep_eval_dev (without
 * grad_samples the handle keeps a buffer of that size itself).  Non-finite inputs are evaluated, not rejected. */
int qc_sweep_grad_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                      const double* dweights, double* dfids, double* dJ, double* dgrad, double* dgrad_samples, void* stream);
/* the same on host buffers (synchronous) */
int qc_sweep_grad(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale,
                  const double* weights, double* fids, double* J, double* grad, double* grad_samples);

/* The derivatives with respect to the SYSTEMS: grad_theta[s, j] = dF_s/dtheta[s, j] (S x n_pert) and grad_scale[s, k] = dF_s/dc[s, k]
 * (S x m), sample-major as theta / scale, raw per-sample values (no weights):
 *     dF_s/dtheta[s, j] = sum_t dt_t <lambda_{t+1} x_t^T, L(dt_t G; P_j)>,   dF_s/dc[s, k] = sum_t a_{t,k} dt_t <lambda_{t+1} x_t^T, L(dt_t G; G_k)>
 * over the intervals t = 0 .. T-2, from the same backward walk (one per call, whatever is requested): the per-interval tile of the
 * walk is summed over a chunk and contracted with the perturbation tiles once, the drive contractions are weighted with the controls
 * before the factor c[s, k] is applied (no division by c: defined at c = 0; scale = NULL: the derivative at c = 1).  The chunk
 * shares are added in ascending chunk order: no atomics, repeated calls return the same bits, and grad_theta / grad_scale do not
 * depend on which other outputs were requested.  Every other argument, the scope (qc_sweep_desc_grad_supported), the scratch and the
 * one-in-flight rule are those of qc_sweep_grad_dev, and fids / J / grad / grad_samples carry its bits; without grad and
 * grad_samples the S x (T-1) x (m + (off_dt >= 0)) per-interval buffer is neither allocated nor written.  Every output is optional,
 * at least one must be non-NULL; grad_theta on a handle with n_pert = 0, or grad_scale with m = 0, is QC_ERR_INVALID.
 * On an "mfma32-sweep" handle made with wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_PARAMS both entry points behave exactly as on an
 * "mfma16-sweep" handle (the parameter flavour of the 2 x 2-tile walk; scope, checks and outputs as above, fids / J / grad / grad_samples
 * with the bits of qc_sweep_grad on the same handle).  On one made with wide = QC_SWEEP_WIDE alone both return QC_ERR_UNSUPPORTED
 * ("parameter gradients are not served in the mfma32-sweep form"), with or without QC_SWEEP_WIDE_STORED: the stored-state walk's
 * parameter flavour on 2 x 2 tiles needs wide = 11.
 * On an "mfma64-sweep" handle made with QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_PARAMS both entry points serve closed systems with at
 * most 32 state columns (the parameter flavour of the 4 x 4-tile walk: du before the factor c_k, so grad_scale is defined at c = 0;
 * fids / J / grad / grad_samples with the bits of qc_sweep_grad on the same handle); on one made without QC_SWEEP_WIDE_64_PARAMS both
 * return QC_ERR_UNSUPPORTED ("parameter gradients are not served in the mfma64-sweep form (2N = ...)"). */
int qc_sweep_grad_params_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                             const double* dweights, double* dfids, double* dJ, double* dgrad, double* dgrad_samples,
                             double* dgrad_theta, double* dgrad_scale, void* stream);
/* the same on host buffers (synchronous) */
int qc_sweep_grad_params(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale,
                         const double* weights, double* fids, double* J, double* grad, double* grad_samples,
                         double* grad_theta, double* grad_scale);

/* ---- sweep pullbacks: gradients of any function of the final states ------------------------------------------------------ */
/* The pullback of (Z, init, theta, c) -> x_final[s]: the caller hands in one cotangent C_s per sample (the derivative of their loss
 * with respect to that sample's final state) and receives the derivatives of phi_s = <C_s, x_final[s]>.  It is the adjoint walk of
 * qc_sweep_grad with lambda_{T-1} = C_s in place of the fidelity's own seed, so a call costs what a gradient call costs; the final
 * state being linear in the initial one, dphi_s/dinit = lambda_0 comes from one more transposed product of the seed. */
/* device-free: may the pullback serve this descriptor?  Scope = the gradient's scope WITHOUT its two fidelity conditions: an MFMA form
 * ("mfma16-sweep", or "mfma32-sweep" with wide = QC_SWEEP_WIDE), antisymmetric drift / drives / perturbations (the same 64-eps test),
 * at most 16 state columns; with reserved1[0] = QC_SWEEP_STORED_STATES the "mfma16-sweep" form (or "mfma32-sweep" with
 * QC_SWEEP_WIDE_STORED in `wide`), at most 16 state columns, any generators.  fid_kind may be anything, QC_SWEEP_FID_NONE and QC_FID_DENSITY included.  When 0,
 * qc_sweep_last_error(NULL) says why, prefixed "qc_sweep pullback: ".  An invalid descriptor returns its own error. */
int qc_sweep_desc_vjp_supported(const qc_sweep_desc* d, int32_t* supported);
/* phi_s = <cot[s], x_final[s]>.  cot: S x (2N cols), the layout of `finals`.  Outputs, each optional, at least one non-NULL:
 *   finals        S x (2N cols)      the bits of qc_sweep_eval
 *   grad          Z_len              sum_s dphi_s/dZ (plain sum, ascending s), +0.0 outside controls / timesteps of knots 0..T-2
 *   grad_samples  S x (T-1) x nd     dphi_s/d(a_t, dt_t), the layout of qc_sweep_grad
 *   grad_init     S x (2N cols)      dphi_s/dinit = (E_{T-2} ... E_0)^T cot[s]
 *   grad_theta    S x n_pert, grad_scale  S x m   ("mfma16-sweep", and "mfma32-sweep" handles made with wide = QC_SWEEP_WIDE |
 *                                    QC_SWEEP_WIDE_PARAMS; on an "mfma32-sweep" handle without that bit QC_ERR_UNSUPPORTED,
 *                                    "parameter cotangents are not served in the mfma32-sweep form"; "mfma64-sweep" handles
 *                                    made with QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_PARAMS, without the latter
 *                                    QC_ERR_UNSUPPORTED, "... not served in the mfma64-sweep form (2N = ...)")
 * cot must not overlap any output.  Scratch and the one-in-flight rule as qc_sweep_grad_dev.  Repeated calls return the same bits, and
 * no output's bits depend on which other outputs were requested.  Non-finite cotangents are evaluated, not rejected: they reach
 * their own sample's outputs and `grad`, nothing else. */
int qc_sweep_vjp_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                     const double* dcot, double* dfinals, double* dgrad, double* dgrad_samples, double* dgrad_init,
                     double* dgrad_theta, double* dgrad_scale, void* stream);
/* the same on host buffers (synchronous) */
int qc_sweep_vjp(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale,
                 const double* cot, double* finals, double* grad, double* grad_samples, double* grad_init,
                 double* grad_theta, double* grad_scale);

/* ---- sweep pushforwards: tangents of the final states and fidelities along one direction --------------------------------- */
/* The pushforward of (Z, init, theta, c) -> x_final[s] along the direction (vZ, vinit, vtheta, vscale):
 *     d(hG)_t = vh_t G_s(a_t) + h_t ( sum_j vtheta[s,j] P_j + sum_k ( vscale[s,k] a_{t,k} + c[s,k] va_{t,k} ) G_k )
 *     xdot_0 = vinit,   xdot_{t+1} = E_t xdot_t + L(h_t G; d(hG)_t) x_t   (L: the Frechet derivative of exp),   t = 0 .. T-2
 *     tfinals[s] = xdot_{T-1},   tfids[s] = <dF/dx(x_final[s]), xdot_{T-1}>   (the |tr| / n form is not special-cased at tr = 0).
 * One forward walk that differentiates every product beside itself: 108 + 12 sq matrix-core instructions per interval against the
 * sweep's 36 + 4 sq ("mfma32-sweep": 864 + 96 sq against 288 + 32 sq; "mfma64-sweep": (27 + 3 sq) x 256 against (9 + sq) x 256).  Nothing is reversed, so antisymmetry is not asked for: Lindblad
 * generators (QC_FID_DENSITY handles) are served.
 * With one pullback call it gives the Gauss-Newton product J^T (d2 loss) J v of any loss of the final states. */
/* device-free: may the pushforward serve this descriptor?  Scope: the "mfma16-sweep" form (2N <= 16, m <= 8), or the "mfma32-sweep" form
 * (16 < 2N <= 32, m <= 8) of a descriptor whose `wide` has QC_SWEEP_WIDE_TANGENT, or the "mfma64-sweep" form (32 < 2N <= 64, m <= 16) of
 * one whose `wide` has QC_SWEEP_WIDE_64_TANGENT, there with 2N x state_cols <= 2048; any generators, any state_cols and fid_kind the sweep
 * serves there.  When 0, qc_sweep_last_error(NULL) says why, prefixed "qc_sweep pushforward: "
 * ("... not served in the mfma32-sweep form", the mfma64-sweep form with 2N -- and, above the bound, ns --, or the rollout-per-sample
 * form with its cause).  An invalid descriptor returns its own error. */
int qc_sweep_desc_jvp_supported(const qc_sweep_desc* d, int32_t* supported);
/* Directions, each optional (NULL = zero: the same bits as an explicit zero array), at least one non-NULL:
 *   vZ       Z_len, the layout of Z, shared by the samples.  ONLY the controls and timesteps of knots 0 .. T-2 are read: whatever
 *            stands anywhere else (a NaN included) has no effect
 *   vinit    2N x cols, shared by the samples
 *   vtheta   S x n_pert (QC_ERR_INVALID when n_pert = 0)
 *   vscale   S x m (QC_ERR_INVALID when m = 0); valid with scale = NULL, which means c = 1
 * Outputs, each optional, at least one non-NULL:
 *   finals   S x (2N cols), fids  S     the bits of qc_sweep_eval on the same handle
 *   tfinals  S x (2N cols), tfids S     the tangents (fids / tfids on a handle without a fidelity: QC_ERR_INVALID)
 * Directions must not overlap outputs.  S in 1 .. 2^24.  Scratch and the one-in-flight rule as qc_sweep_eval_dev.  Repeated calls
 * return the same bits, and no output's bits depend on which other outputs were requested.  Non-finite inputs are evaluated, not
 * rejected: a non-finite entry of vtheta[s] or vscale[s] stays inside sample s (the number of squarings never depends on the direction). */
int qc_sweep_jvp_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                     const double* dvZ, const double* dvinit, const double* dvtheta, const double* dvscale,
                     double* dfinals, double* dfids, double* dtfinals, double* dtfids, void* stream);
/* the same on host buffers (synchronous) */
int qc_sweep_jvp(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale,
                 const double* vZ, const double* vinit, const double* vtheta, const double* vscale,
                 double* finals, double* fids, double* tfinals, double* tfids);

/* ---- sweep Hessian products: the tangent of the sweep pullback along one direction --------------------------------------- */
/* With phi_s = <cot[s], x_final[s]>, g_s = dphi_s/d(a_t, dt_t) (qc_sweep_vjp's grad_samples[s]) and q_s = dphi_s/dinit (its grad_init[s]):
 *     tgrad_samples[s] = d/de g_s(Z + e vZ, init + e vinit, theta + e vtheta, c + e vscale; cot + e vcot) at e = 0
 *     tgrad_init[s]    = d/de q_s = Wdot^T cot[s] + W^T vcot[s]              (W: the sample's propagator, Wdot its tangent)
 *     tgrad            = sum_s tgrad_samples[s] (plain sum, ascending s) in the layout of Z.
 * With cot = d loss/dX and vcot = (d2 loss/dX2) Xdot, Xdot = qc_sweep_jvp's tfinals along vZ, tgrad is the EXACT Hessian product of
 * loss(X(Z)) with vZ; with vcot = NULL it is the curvature of the sweep map alone, sum_s <cot[s], d2 x_s/dZ2 vZ>: what the Gauss-Newton
 * product of qc_sweep_jvp + qc_sweep_vjp drops, and the whole Hessian of a loss that is linear in the final states.
 * One tangent forward walk (qc_sweep_jvp's, for the chunk totals) and one backward walk that differentiates every product of the
 * gradient walk beside itself with a degree-10 series: 408 + 36 sq matrix-core instructions per interval against the pullback's 112 + 12 sq
 * ("mfma32-sweep" handles with QC_SWEEP_WIDE_HESSIAN: the same two walks on 2 x 2 tiles, 3120 + 288 sq against 848 + 96 sq). */
/* device-free: may the Hessian product serve this descriptor?  Scope: the closed scope of the pullback -- antisymmetric drift / drives /
 * perturbations, at most 16 state columns, any fid_kind (QC_SWEEP_FID_NONE included) -- in the "mfma16-sweep" form (2N <= 16, m <= 8),
 * or in the "mfma32-sweep" form (16 < 2N <= 32, m <= 8) of a descriptor whose `wide` has QC_SWEEP_WIDE_HESSIAN (QC_SWEEP_WIDE_TANGENT is
 * not needed).  When 0, qc_sweep_last_error(NULL) says why, prefixed "qc_sweep Hessian product: ": the pullback's reason first
 * (antisymmetry, more than 16 columns, the rollout-per-sample form with its cause), then "... not served in the mfma32-sweep form" (that
 * form without the bit).  An invalid descriptor returns its own error. */
int qc_sweep_desc_hvp_supported(const qc_sweep_desc* d, int32_t* supported);
/* cot: S x (2N cols), required.  Directions, each optional (NULL = zero: the same bits as an explicit zero array), at least one non-NULL:
 *   vZ       Z_len; ONLY the controls and timesteps of knots 0 .. T-2 are read (a NaN anywhere else has no effect)
 *   vinit    2N x cols, shared by the samples
 *   vtheta   S x n_pert (QC_ERR_INVALID when n_pert = 0)
 *   vscale   S x m (QC_ERR_INVALID when m = 0); valid with scale = NULL, which means c = 1
 *   vcot     S x (2N cols)
 * Outputs, each optional, at least one non-NULL:
 *   tgrad          Z_len            +0.0 outside the controls / timesteps of knots 0 .. T-2
 *   tgrad_samples  S x (T-1) x nd   the layout of qc_sweep_grad's grad_samples
 *   tgrad_init     S x (2N cols)
 * Inputs must not overlap outputs.  S in 1 .. 2^24.  Scratch and the one-in-flight rule as qc_sweep_eval_dev.  No atomics: repeated calls
 * return the same bits, and no output's bits depend on which other outputs were requested.  Non-finite entries of cot[s], vcot[s],
 * vtheta[s], vscale[s] are evaluated, not rejected: they reach sample s's outputs and tgrad, nothing else (the number of squarings never
 * depends on a direction). */
int qc_sweep_hvp_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                     const double* dcot, const double* dvZ, const double* dvinit, const double* dvtheta, const double* dvscale,
                     const double* dvcot, double* dtgrad, double* dtgrad_samples, double* dtgrad_init, void* stream);
/* the same on host buffers (synchronous) */
int qc_sweep_hvp(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale,
                 const double* cot, const double* vZ, const double* vinit, const double* vtheta, const double* vscale,
                 const double* vcot, double* tgrad, double* tgrad_samples, double* tgrad_init);

/* ---- noise-trajectory sweeps: perturbations that change from interval to interval, and their gradients ------------------- */
/* The sweep above holds theta[s, j] constant for the whole pulse.  Here every sample also carries a trajectory of perturbation
 * amplitudes: in interval t = 0 .. T-2, for sample s,
 *     G_{s,t} = G_drift + sum_j (theta[s, j] + noise[s, t, j]) P_j + sum_k c[s, k] a_{t,k} G_k,     x_{t+1} = exp(dt_t G_{s,t}) x_t.
 * noise: S x (T-1) x n_pert doubles, sample-major, then interval, then perturbation: noise[(s (T-1) + t) n_pert + j].  A detuning that
 * drifts during the pulse (Ornstein-Uhlenbeck, 1/f), additive noise on a drive line (P_j = G_k), S realisations of a stochastic
 * average: one call in place of S single-sample calls that each carry the noise in a Z of their own.  The handle is an ordinary
 * qc_sweep handle; in the "mfma16-sweep" form the perturbation tiles sit in registers beside the drive tiles, their coefficients read
 * per sample and interval.  An "mfma32-sweep" handle (16 < 2N <= 32: two coupled three-level transmons with drifting detunings, a 4-qubit
 * register, two qubits with T1 / T2 whose decay rate fluctuates) serves both entry-point families when its descriptor sets
 * QC_SWEEP_WIDE_NOISE in `wide`: that form keeps no generator resident (every image is read again per interval), so the only limits
 * there are m <= 8 and n_pert <= QC_MAX_PERT, up to 16 generators.  An "mfma64-sweep" handle (32 < 2N <= 64: three coupled three-level
 * transmons whose detunings drift, a 5-qubit register with noisy drive lines, a five-level Lindblad model) serves them when its
 * descriptor sets QC_SWEEP_WIDE_64_NOISE (qc_sweep64_noise.hip): m <= 16 and n_pert <= QC_MAX_PERT, up to 24 generators; its gradient
 * needs QC_SWEEP_WIDE_64_GRAD as well and serves states of up to 32 columns.  Every contract below holds in all three forms.
 * At noise = +0.0 the outputs equal those of qc_sweep_eval / qc_sweep_grad on the same handle value for value (a -0.0 may come out
 * as +0.0, nothing else).
 * Out of scope: "mfma32-sweep" handles without QC_SWEEP_WIDE_NOISE, "mfma64-sweep" handles without QC_SWEEP_WIDE_64_NOISE and
 * "rollout-per-sample" handles;
 * pullbacks, pushforwards and Hessian products with noise (and with them the autograd function of the Python layer); noise gradients of
 * open systems; several devices. */
/* device-free: may the noise sweep serve this descriptor?  Scope of the evaluation: the "mfma16-sweep" form with n_pert >= 1 and
 * m + n_pert <= 8, or the "mfma32-sweep" form of a descriptor whose `wide` has QC_SWEEP_WIDE_NOISE with n_pert >= 1 (no condition on
 * m + n_pert), or the "mfma64-sweep" form of a descriptor whose `wide` has QC_SWEEP_WIDE_64_NOISE with n_pert >= 1 (m <= 16 by the
 * form); any generators (Lindblad ones included), any state_cols and fid_kind the sweep serves there.  When 0,
 * qc_sweep_last_error(NULL) says why, prefixed "qc_sweep noise: ": "... not served in the mfma32-sweep form" (that form without the
 * bit), the mfma64-sweep form without its bit (the form's sentence with 2N), the rollout-per-sample form with its cause, n_pert = 0, or ("mfma16-sweep") m + n_pert > 8 with the two numbers.  An invalid
 * descriptor returns its own error. */
int qc_sweep_desc_noise_supported(const qc_sweep_desc* d, int32_t* supported);
/* The arguments and rules of qc_sweep_eval / qc_sweep_eval_dev, plus `noise` (required; it must not overlap an output:
 * QC_ERR_INVALID).  finals: S x (2N cols); fids: S; either may be NULL, not both.  Scratch, the one-in-flight rule and S in 1 .. 2^24
 * as qc_sweep_eval_dev.  Two launches: the chunk totals with m + n_pert tiles, and the sweep's own final-state / fidelity launch.
 * Non-finite entries of noise[s] are evaluated, not rejected: they reach sample s's outputs, nothing else. */
int qc_sweep_noise_eval(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale,
                        const double* noise, double* finals, double* fids);
int qc_sweep_noise_eval_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                            const double* dnoise, double* dfinals, double* dfids, void* stream);
/* The arguments, layouts, weights rule and outputs of qc_sweep_grad / qc_sweep_grad_dev (every output optional, at least one
 * non-NULL), plus `noise` as above and one more output:
 *   grad_noise   S x (T-1) x n_pert, the layout of noise: dF_s/dnoise[s, t, j] = dt_t <lambda_{t+1} x_t^T, L(dt_t G_{s,t}; P_j)>, raw
 *                per-sample values (no weights) -- the time-resolved noise sensitivity of every sample, from the per-interval tile the
 *                backward walk forms anyway (qc_sweep_grad_params sums it over t: at noise = 0, sum_t grad_noise[s, t, j] = grad_theta[s, j]).
 * Scope: the noise scope and the gradient's together (closed systems, a unitary or ket fidelity, at most 16 state columns; in the
 * "mfma64-sweep" form QC_SWEEP_WIDE_64_GRAD and at most 32); a refusal
 * is prefixed "qc_sweep noise: " and carries the noise scope's reason, else the gradient's own.  Without grad_samples the handle
 * keeps the per-interval buffer itself when `grad` needs it.  No atomics: repeated calls return the same bits, and no output's bits
 * depend on which other outputs were requested.  Non-finite entries of noise[s] reach sample s's outputs and `grad` / `J`, nothing else. */
int qc_sweep_noise_grad(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale,
                        const double* noise, const double* weights, double* fids, double* J, double* grad, double* grad_samples,
                        double* grad_noise);
int qc_sweep_noise_grad_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                            const double* dnoise, const double* dweights, double* dfids, double* dJ, double* dgrad,
                            double* dgrad_samples, double* dgrad_noise, void* stream);

/* Diagnostic only: when the environment variable QC_STAMPS=1 is set at qc_create, the MFMA kernel
 * records 16 s_memrealtime (100 MHz) checkpoints per interval; this copies them out (synchronises the
 * device).  Not part of the evaluated path; a handle created without QC_STAMPS returns
 * QC_ERR_UNSUPPORTED. */
int qc_debug_read_stamps(qc_handle* h, uint64_t* out, int64_t count);

/* Diagnostic only: the rate (GB/s of values written) at which this host replicates the compact Jacobian form of handle h into a
 * full value array with the library's own worker team -- no GPU work, no transfer; the host-side bound of qc_eval_jac that
 * bench.py reports next to the PCIe bound.  QC_ERR_UNSUPPORTED when the handle's Jacobian has no replicated blocks. */
int qc_debug_host_expand_rate(qc_handle* h, int32_t reps, double* GBps);

/* Diagnostic only: would the entry points evaluate this list with ONE launch (gridDim.y = count) rather than one per member?
 * what = 0: F + dF of qc_eval_F_jac_dev_multi; 1: mu_d2F of qc_eval_hess_dev_multi; 2: the Jacobian values of the host-buffer list
 * calls (qc_eval_jac_list, qc_eval_F_jac_list), whose members write one block per interval for a single copy to the host.  Returns 1
 * or 0 from the functions those entry points decide with -- nothing is launched or allocated -- or a QC_ERR_* code: a NULL handle,
 * handles bound to different devices, a multi-device handle, for what = 2 handles that do not describe one problem.  The results do
 * not depend on the answer. */
int qc_debug_list_shares_launch(qc_handle* const* hs, int32_t count, int32_t what);

/* Library/build identification: "qcolloc-hip <major>.<minor> (gfx950, ...)" */
const char* qc_version(void);
/* QC_VERSION_MAJOR * 1000 + QC_VERSION_MINOR of the build.  A binding compares it with the header version it mirrors when
 * it loads the library (struct sizes alone do not reveal a renumbered constant). */
int32_t qc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* QCOLLOC_H */
