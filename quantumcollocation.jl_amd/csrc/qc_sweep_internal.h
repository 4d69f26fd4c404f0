// What qc_sweep.hip (forward sweep; its 4 x 4-tile form: qc_sweep64.hip), qc_sweep_grad.hip (its adjoint), qc_sweep_open_grad.hip and qc_sweep32_open_grad.hip (the adjoint on stored states), qc_sweep_vjp.hip (the pullback of the final states),
// qc_sweep_jvp.hip (their pushforward), qc_sweep_hvp.hip and qc_sweep32_hvp.hip (the tangent of the pullback) and qc_sweep_noise.hip (noise trajectories) share: the handle with its scratch and staging buffers, the descriptor and argument checks, the launch
// parameters of the (sample, chunk) kernels (SweepParams, qc_sweep_params), the preamble of every launch of chunk totals (qc_sweep_plan_totals: chunk rule, scratch, parameters) and those launches.  Not part of the ABI.
#pragma once

#include <string>

#include "qc_side.h"

struct qc_sweep : qc_side {
    qc_sweep_desc d;             // caller-owned arrays are not retained (pointers nulled)
    bool mfma = false;
    bool mfma32 = false;         // the 2 x 2-tile form of a wide descriptor ("mfma32-sweep", qc_sweep32.hip); mfma is set as well
    bool mfma64 = false;         // the 4 x 4-tile form of a descriptor with QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 ("mfma64-sweep", qc_sweep64.hip): the forward sweep, and with wide64_grad its closed adjoint; mfma is set as well
    bool wide64_grad = false;    // mfma64 and wide has QC_SWEEP_WIDE_64_GRAD: gradients and pullbacks of closed systems are served (qc_sweep64_grad.hip)
    bool wide64_par = false;     // wide64_grad and wide has QC_SWEEP_WIDE_64_PARAMS: parameter gradients and cotangents are served (the flavour <true> of qc_sweep64_grad.hip's walk)
    bool wide64_stored = false;  // wide64_grad and wide has QC_SWEEP_WIDE_64_STORED: with `stored`, reverse mode by the 4 x 4-tile stored-state walk, any generators (qc_sweep64_open_grad.hip)
    bool wide64_tangent = false; // mfma64 and wide has QC_SWEEP_WIDE_64_TANGENT: pushforwards are served, any generators, ns <= 2048 (qc_sweep64_jvp.hip)
    bool wide64_noise = false;   // mfma64 and wide has QC_SWEEP_WIDE_64_NOISE: noise trajectories are served, any generators; their gradients with wide64_grad (qc_sweep64_noise.hip)
    bool wide_par = false;       // mfma32 and wide has QC_SWEEP_WIDE_PARAMS: parameter gradients and cotangents are served (qc_sweep32_grad.hip)
    bool wide_stored = false;    // mfma32 and wide has QC_SWEEP_WIDE_STORED: with `stored`, reverse mode by the 2 x 2-tile stored-state walk (qc_sweep32_open_grad.hip)
    bool wide_tangent = false;   // mfma32 and wide has QC_SWEEP_WIDE_TANGENT: pushforwards are served (qc_sweep32_jvp.hip)
    bool wide_noise = false;     // mfma32 and wide has QC_SWEEP_WIDE_NOISE: noise trajectories are served (qc_sweep32_noise.hip)
    bool wide_hessian = false;   // mfma32 and wide has QC_SWEEP_WIDE_HESSIAN: Hessian products of closed systems are served (qc_sweep32_hvp.hip)
    bool stored = false;         // reserved1[0] = QC_SWEEP_STORED_STATES: reverse mode by the stored-state walk (qc_sweep_open_grad.hip)
    bool grad_ok = false;        // the gradient's scope (qc_sweep_grad.hip), decided at create from the caller's matrices
    std::string grad_why;        // when not: the reason
    bool vjp_ok = false;         // the pullback's scope (qc_sweep_vjp.hip): the gradient's without its fidelity conditions
    std::string vjp_why;
    bool jvp_ok = false;         // the pushforward's scope (qc_sweep_jvp.hip): "mfma16-sweep" handles, "mfma32-sweep" ones with wide_tangent, "mfma64-sweep" ones with wide64_tangent and ns <= 2048; any generators
    std::string jvp_why;
    bool hvp_ok = false;         // the Hessian product's scope (qc_sweep_hvp.hip): the closed scope in the "mfma16-sweep" form, and in the "mfma32-sweep" form with wide_hessian
    std::string hvp_why;
    bool noise_ok = false;       // the noise sweep's scope (qc_sweep_noise.hip): "mfma16-sweep", n_pert >= 1, m + n_pert <= 8 tiles; "mfma32-sweep" with wide_noise, n_pert >= 1; "mfma64-sweep" with wide64_noise, n_pert >= 1
    std::string noise_why;
    bool noise_grad_ok = false;  // its gradient's scope: the noise scope and the gradient's together
    std::string noise_grad_why;  // the noise scope's reason, else the gradient's own
    int n = 0, nc = 0, ns = 0, fid_n = 0;
    int64_t Zlen = 0;
    double* dG = nullptr;        // (1 + m + p) matrices, column-major (per-sample form)
    double* dImg = nullptr;      // their A-layout images (MFMA form)
    double *dgr = nullptr, *dgi = nullptr;
    // Scratch of the "_dev" entry points, grown at the first call that needs it.  Largest request of a call, and who makes it:
    qc_buf dTot;         // chunk totals, S x n_chunks x 256 (mfma32: 1024, mfma64: 4096)             eval, grad, vjp, noise
    qc_buf dFin;         // per-sample form: final states, S x ns                             eval
    double *dGs = nullptr, *dRE = nullptr, *dRQ = nullptr, *dRS = nullptr, *dRout = nullptr;      // per-sample form, sized at create
    qc_buf dXs, dLs;     // x and lambda at the chunk ends, S x n_chunks x ns each            grad, vjp, noise_grad
    qc_buf dGsamp;       // per-interval derivatives when the caller keeps none, S x (T-1) x nd   grad, vjp, noise_grad
    qc_buf dGfid;        // fidelities when the caller keeps none, S                         grad, noise_grad
    qc_buf dXall;        // stored-state walk: x_t of knots 0 .. T-2, S x (T-1) x ns                  grad, vjp (stored handles)
    qc_buf dPart;        // chunk shares of the parameter gradients, S x n_chunks x (p + m)  grad_params, vjp
    qc_buf dTotJ;        // chunk totals and their tangents, S x n_chunks x 512 (mfma32: 2048, mfma64: 8192) jvp, hvp
    qc_buf dXsT, dLsT;   // xdot and lambdadot at the chunk ends, S x n_chunks x ns each      hvp (x and lambda: dXs, dLs)
    qc_buf dTGsamp;      // per-interval tangents when the caller keeps none, S x (T-1) x nd  hvp
    // Staging of the host-buffer entry points (qc_stage): one buffer per argument, shared by every entry point that has the argument.
    qc_buf sZ, sInit;    // Zlen, ns: allocated at create                                     every entry
    qc_buf sTheta;       // S x p                                                             every entry
    qc_buf sScale;       // S x m                                                             every entry
    qc_buf sFinals;      // S x ns                                                            eval, vjp, jvp
    qc_buf sFids;        // S                                                                 eval, grad, jvp
    qc_buf sW;           // weights, S                                                        grad
    qc_buf sJ;           // 1                                                                 grad
    qc_buf sGrad;        // the dense gradient, Zlen                                          grad, vjp
    qc_buf sGradS;       // per-sample gradients, S x (T-1) x nd                              grad, vjp
    qc_buf sGth;         // grad_theta, S x p                                                 grad_params, vjp
    qc_buf sGsc;         // grad_scale, S x m                                                 grad_params, vjp
    qc_buf sCot;         // cotangents, S x ns                                                vjp, hvp
    qc_buf sGinit;       // grad_init, S x ns                                                 vjp
    qc_buf sVZ, sVinit;  // directions, Zlen and ns                                           jvp, hvp
    qc_buf sVth, sVsc;   // directions, S x p and S x m                                       jvp, hvp
    qc_buf sTfin, sTfid; // tangents, S x ns and S                                            jvp
    qc_buf sVcot;        // the direction of the cotangents, S x ns                           hvp
    qc_buf sTgrad;       // the dense tangent of the gradient, Zlen                           hvp
    qc_buf sTgradS;      // its per-sample form, S x (T-1) x nd                               hvp
    qc_buf sTginit;      // the tangent of grad_init, S x ns                                  hvp
    qc_buf sNoise;       // noise, S x (T-1) x p                                              noise_eval, noise_grad
    qc_buf sGnoise;      // grad_noise, S x (T-1) x p                                         noise_grad
};

// The launch parameters of every kernel of the MFMA forms that runs one wavefront per (sample, chunk of consecutive intervals)
struct SweepParams {
    int n, nc, m, p, zdim, off_a, off_dt, n_int, chunk, n_chunks, nd;   // nd = m + (off_dt >= 0): derivatives per interval
    long long items;             // S * n_chunks
    double dt_fixed;
    const double* img;           // A-layout images, 256 doubles a matrix ("mfma32-sweep": 1024; "mfma64-sweep": column-major, 4096): drift, m drives, p perturbations
};

inline SweepParams qc_sweep_params(const qc_sweep* h, int64_t S, int64_t chunk, int64_t n_chunks) {
    SweepParams P;
    P.n = h->n; P.nc = h->nc; P.m = h->d.m; P.p = h->d.n_pert; P.zdim = h->d.zdim; P.off_a = h->d.off_a; P.off_dt = h->d.off_dt;
    P.n_int = (int)(h->d.T - 1); P.chunk = (int)chunk; P.n_chunks = (int)n_chunks; P.nd = h->d.m + (h->d.off_dt >= 0 ? 1 : 0);
    P.items = S * n_chunks;
    P.dt_fixed = h->d.dt_fixed;
    P.img = h->dImg;
    return P;
}

// records the message in the handle (when there is one) and in the slot qc_sweep_last_error(NULL) returns
int qc_sweep_fail(qc_side* h, int code, const std::string& msg);
std::string* qc_sweep_err_slot();
// The argument checks every entry point shares, in the order of the tables of qcolloc.h: the NULL handle; the entry's scope
// (`ok`: the handle's flag, NULL for qc_sweep_eval; refused as `scope` + the handle's reason `why`); NULL Z / init; `missing`, the name
// of a further input that is NULL (the pullback's "cot"), else NULL; the range of S; theta against n_pert.  The entry's own lines follow.
int qc_sweep_check(qc_sweep* h, const char* who, const bool qc_sweep::*ok, const char* scope, const std::string qc_sweep::*why, const void* Z,
                   const void* init, const char* missing, int64_t S, const void* theta);
// the M of the kernels templated on the drive tiles a wave keeps in registers: LAUNCH(M) for the smallest of 1, 2, 4, 6, 8 that holds m
#define QC_SWEEP_FOR_M(m, LAUNCH)      \
    do {                               \
        if ((m) <= 1) LAUNCH(1);       \
        else if ((m) <= 2) LAUNCH(2);  \
        else if ((m) <= 4) LAUNCH(4);  \
        else if ((m) <= 6) LAUNCH(6);  \
        else LAUNCH(8);                \
    } while (0)
int qc_sweep_validate_desc(const qc_sweep_desc* d);
bool qc_sweep_desc_is_mfma(const qc_sweep_desc* d);
// The form a descriptor takes: "rollout-per-sample", "mfma16-sweep", "mfma32-sweep" (wide descriptors with 16 < 2N <= 32) or "mfma64-sweep"
// (descriptors with QC_SWEEP_WIDE | QC_SWEEP_WIDE_64, 32 < 2N <= 64, m <= 16: the forward sweep only)
enum qc_sweep_form { QC_SWEEP_FORM_PER_SAMPLE = 0, QC_SWEEP_FORM_16 = 1, QC_SWEEP_FORM_32 = 2, QC_SWEEP_FORM_64 = 3 };
qc_sweep_form qc_sweep_desc_form(const qc_sweep_desc* d);
// QC_SWEEP_FORM_64: "the handle takes the mfma64-sweep form (2N = ...), which serves the forward sweep only", the reason of every other scope there
std::string qc_sweep_form64_why(const qc_sweep_desc* d);
// QC_SWEEP_FORM_64: the reason of a scope that the form does not serve.  Without QC_SWEEP_WIDE_64_GRAD the sentence above; with it "the
// handle takes the mfma64-sweep form (2N = ...), which does not serve <what>"
std::string qc_sweep_form64_unserved(const qc_sweep_desc* d, const char* what);
// QC_SWEEP_FORM_PER_SAMPLE: "the handle takes the rollout-per-sample form (...)" with its cause, the reason of every scope that needs an MFMA form
std::string qc_sweep_per_sample_why(const qc_sweep_desc* d);
// the chunk rule of the MFMA forms: `form` chooses the fill constant (QC_SWEEP_FORM_64: one workgroup per compute unit; _16 and _32: a couple of waves per SIMD)
void qc_sweep_chunks(qc_sweep_form form, int64_t S, int64_t T, int64_t* chunk, int64_t* n_chunks);
// What every launch of chunk totals starts with: the chunk rule for S samples, `buf` grown to S x n_chunks x doubles_per_item, the launch
// parameters in *P, the rule's result in *chunk, *n_chunks; QC_OK or the failed allocation's code.  qc_sweep_grid: workgroups of `waves` waves.
int qc_sweep_plan_totals(qc_sweep* h, int64_t S, qc_buf& buf, size_t doubles_per_item, SweepParams* P, int64_t* chunk, int64_t* n_chunks);
inline unsigned qc_sweep_grid(const SweepParams& P, int waves) { return (unsigned)((P.items + waves - 1) / waves); }
// "mfma16-sweep" handles: grows h->dTot and launches qc_sweep_mfma16_kernel on `st` (S x n_chunks tiles of 256 doubles)
int qc_sweep_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, hipStream_t st, int64_t* chunk,
                           int64_t* n_chunks);
// "mfma32-sweep" handles (qc_sweep32.hip): the A-layout image of one n x n matrix (1024 doubles), and the launch of qc_sweep_mfma32_kernel
// (S x n_chunks column-major 32 x 32 totals of 1024 doubles in h->dTot)
void qc_sweep32_image(const double* G, int n, double* img);
int qc_sweep32_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, hipStream_t st, int64_t* chunk,
                             int64_t* n_chunks);
// "mfma64-sweep" handles (qc_sweep64.hip): the zero-padded column-major 64 x 64 image of one n x n matrix (4096 doubles), and the launch of
// qc_sweep_mfma64_kernel, one workgroup per (sample, chunk) (S x n_chunks column-major 64 x 64 totals of 4096 doubles in h->dTot)
// (hidden: the library exports no symbol of this form)
__attribute__((visibility("hidden"))) void qc_sweep64_image(const double* G, int n, double* img);
__attribute__((visibility("hidden"))) int qc_sweep64_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, hipStream_t st, int64_t* chunk,
                             int64_t* n_chunks);
// "mfma64-sweep" handles with `wide64_grad` (qc_sweep64_grad.hip): the backward walk qc_sweep64_grad_kernel<false>, one workgroup per (sample, chunk)
// (gs: S x (T-1) x nd; x and lambda at the chunk ends from h->dXs / h->dLs), or with `par` (handles with `wide64_par`) the parameter flavour
// <true>, which also writes the chunk shares S x n_chunks x (p + m) into `part` (gs may then be NULL); the caller runs
// qc_sweep_launch_par_reduce behind it.  QC_OK or the launch's code
__attribute__((visibility("hidden"))) int qc_sweep64_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, int64_t chunk,
                                                                  int64_t n_chunks, double* gs, bool par, double* part, hipStream_t st);
// "mfma64-sweep" handles with `stored` and `wide64_stored` (qc_sweep64_open_grad.hip): qc_sweep64_open_store_kernel writes x_t of every knot
// 0 .. T-2 into h->dXall (grown by the caller) from `dinit` and the chunk ends of h->dXs, then qc_sweep64_open_grad_kernel<par> walks every chunk
// backwards from h->dLs; arguments, outputs and what the caller runs behind it as qc_sweep64_launch_walk.  QC_OK or a launch's code
__attribute__((visibility("hidden"))) int qc_sweep64_open_launch_walk(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta,
                                                                       const double* dscale, int64_t chunk, int64_t n_chunks, double* gs, bool par, double* part,
                                                                       hipStream_t st);
// "mfma32-sweep" gradients (qc_sweep32_grad.hip): the backward walk qc_sweep32_grad_kernel<false> (gs: S x (T-1) x nd), or with `par` the
// parameter flavour <true> (gs may be NULL) and qc_sweep_par_reduce_kernel out of h->dPart; scratch is the caller's
void qc_sweep32_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, int64_t chunk, int64_t n_chunks,
                            double* gs, bool par, double* dgrad_theta, double* dgrad_scale, hipStream_t st);
// "mfma16-sweep" handles (qc_sweep_grad.hip): the backward walk qc_sweep_grad_kernel<M, false> (gs: S x (T-1) x nd), or with `par` the
// parameter flavour <M, true> (gs may be NULL) and qc_sweep_par_reduce_kernel out of h->dPart; scratch is the caller's
void qc_sweep16_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, int64_t chunk, int64_t n_chunks,
                            double* gs, bool par, double* dgrad_theta, double* dgrad_scale, hipStream_t st);
// grad_theta / grad_scale out of the chunk shares in h->dPart (qc_sweep_grad.hip: qc_sweep_par_reduce_kernel)
void qc_sweep_launch_par_reduce(qc_sweep* h, int64_t S, int64_t n_chunks, double* dgrad_theta, double* dgrad_scale, hipStream_t st);
// Stored-state handles (qc_sweep_open_grad.hip): qc_sweep_open_store_kernel<M> writes x_t of every knot 0 .. T-2 into h->dXall (grown by
// the caller) from `dinit` and the chunk ends of h->dXs, then qc_sweep_open_grad_kernel<M, par> walks every chunk backwards from h->dLs;
// arguments and outputs as qc_sweep16_launch_walk
void qc_sweep_open_launch_walk(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                               int64_t chunk, int64_t n_chunks, double* gs, bool par, double* dgrad_theta, double* dgrad_scale, hipStream_t st);
// "mfma32-sweep" handles with `stored` and `wide_stored` (qc_sweep32_open_grad.hip): the same two steps on 2 x 2 tiles,
// qc_sweep32_open_store_kernel and qc_sweep32_open_grad_kernel<par>; arguments and outputs as qc_sweep_open_launch_walk
void qc_sweep32_open_launch_walk(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                                 int64_t chunk, int64_t n_chunks, double* gs, bool par, double* dgrad_theta, double* dgrad_scale, hipStream_t st);
// what reverse mode asks of a descriptor: reserved1[0] = 0, the closed scope; QC_SWEEP_STORED_STATES, the "mfma16-sweep" form (or the
// "mfma32-sweep" form of a descriptor whose wide has QC_SWEEP_WIDE_STORED) and at most 16 state columns, any generators; the "mfma64-sweep" form
// of a descriptor whose wide has QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_STORED and at most 32 state columns, any generators.  qc_sweep_closed_grad_scope: the gradient's scope of reserved1[0] = 0, for the noise gradient.
bool qc_sweep_reverse_scope(const qc_sweep_desc* d, std::string* why);
bool qc_sweep_closed_grad_scope(const qc_sweep_desc* d, std::string* why);
// device-free: is this (valid) descriptor inside the gradient's scope?  `why` receives the reason when it is not.
bool qc_sweep_grad_scope(const qc_sweep_desc* d, std::string* why);
// what the gradient and the pullback ask alike (an MFMA form -- "mfma64-sweep" only with QC_SWEEP_WIDE_64_GRAD --, antisymmetric matrices, at most
// 16 state columns, in the "mfma64-sweep" form 32), and the pullback's scope
bool qc_sweep_closed_scope(const qc_sweep_desc* d, std::string* why);
bool qc_sweep_vjp_scope(const qc_sweep_desc* d, std::string* why);
// the pushforward's scope (qc_sweep_jvp.hip): the "mfma16-sweep" form, and the "mfma32-sweep" form of a descriptor whose wide has
// QC_SWEEP_WIDE_TANGENT, whatever the generators; the "mfma64-sweep" form of a descriptor whose wide has QC_SWEEP_WIDE_64_TANGENT with
// ns = 2N x state_cols <= 2048 (the finish kernel's LDS at ld = 64)
bool qc_sweep_jvp_scope(const qc_sweep_desc* d, std::string* why);
// "mfma64-sweep" handles with `wide64_tangent` (qc_sweep64_jvp.hip): grows h->dTotJ and launches qc_sweep64_jvp_kernel on `st`, one workgroup
// per (sample, chunk) (S x n_chunks x 2 column-major 64 x 64 matrices of 4096 doubles: the chunk totals and their tangents)
__attribute__((visibility("hidden"))) int qc_sweep64_jvp_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale,
                                                                        const double* dvZ, const double* dvtheta, const double* dvscale, hipStream_t st,
                                                                        int64_t* chunk, int64_t* n_chunks);
// "mfma32-sweep" handles with `wide_tangent` (qc_sweep32_jvp.hip): grows h->dTotJ and launches qc_sweep32_jvp_kernel on `st`
// (S x n_chunks x 2 column-major 32 x 32 matrices of 1024 doubles: the chunk totals and their tangents)
int qc_sweep32_jvp_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dvZ,
                                 const double* dvtheta, const double* dvscale, hipStream_t st, int64_t* chunk, int64_t* n_chunks);
// grows h->dTotJ and launches the chunk totals and their tangents along (vZ, vtheta, vscale), each NULL = zero, on `st`: on "mfma16-sweep"
// handles qc_sweep_jvp_kernel<M> (S x n_chunks x 2 tiles of 256 doubles), on "mfma32-sweep" handles qc_sweep32_jvp_launch_totals, on
// "mfma64-sweep" handles qc_sweep64_jvp_launch_totals
int qc_sweep_jvp_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dvZ,
                               const double* dvtheta, const double* dvscale, hipStream_t st, int64_t* chunk, int64_t* n_chunks);
// the plain sum over the samples of a per-interval buffer (qc_sweep_vjp.hip: qc_sweep_vjp_reduce_kernel), launched on `st`
void qc_sweep_launch_plain_sum(qc_sweep* h, int64_t S, const double* gs, double* dgrad, hipStream_t st);
// the Hessian product's scope (qc_sweep_hvp.hip): the pullback's closed scope, within the "mfma16-sweep" form or the "mfma32-sweep" form
// of a descriptor whose wide has QC_SWEEP_WIDE_HESSIAN
bool qc_sweep_hvp_scope(const qc_sweep_desc* d, std::string* why);
// "mfma32-sweep" handles with `wide_hessian` (qc_sweep32_hvp.hip): qc_sweep32_hvp_kernel walks every chunk backwards from the four states
// at the chunk ends (h->dXs, h->dLs, h->dXsT, h->dLsT, written by the seed of qc_sweep_hvp.hip at ld = 32); tgs: S x (T-1) x nd
void qc_sweep32_hvp_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dvZ,
                                const double* dvtheta, const double* dvscale, int64_t chunk, int64_t n_chunks, double* tgs, hipStream_t st);
// the second launch of an evaluation on an MFMA form (qc_sweep.hip): qc_sweep_finish_kernel on the chunk totals in h->dTot
int qc_sweep_launch_finish(qc_sweep* h, int64_t S, int64_t n_chunks, const double* dinit, double* dfinals, double* dfids, hipStream_t st);
// launches 2 and 4 of a gradient call (qc_sweep_grad.hip): the fidelity's seed (reads h->dTot; writes h->dXs / h->dLs, grown by the caller,
// and the S fidelities), and grad = sum_s w_s gsamp[s] / J = sum_s w_s fids[s] (either may be NULL)
void qc_sweep_launch_fid_seed(qc_sweep* h, int64_t S, int64_t n_chunks, const double* dinit, double* dfids, hipStream_t st);
void qc_sweep_launch_weighted(qc_sweep* h, int64_t S, const double* gsamp, const double* dweights, const double* dfids, double* dgrad, double* dJ,
                              hipStream_t st);
// the noise sweep's scope (qc_sweep_noise.hip): the "mfma16-sweep" form with n_pert >= 1 and m + n_pert <= 8, and the "mfma32-sweep" form
// of a descriptor whose wide has QC_SWEEP_WIDE_NOISE with n_pert >= 1 (nothing is resident there: no tile limit), and the "mfma64-sweep"
// form of one whose wide has QC_SWEEP_WIDE_64_NOISE with n_pert >= 1 (likewise)
bool qc_sweep_noise_scope(const qc_sweep_desc* d, std::string* why);
// "mfma32-sweep" handles with `wide_noise` (qc_sweep32_noise.hip): grows h->dTot and launches qc_sweep32_noise_kernel on `st` (totals as
// qc_sweep32_launch_totals), and the backward walk qc_sweep32_noise_grad_kernel (gs: S x (T-1) x nd, gn: S x (T-1) x p, either may be
// NULL; x and lambda at the chunk ends from h->dXs / h->dLs)
int qc_sweep32_noise_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dnoise,
                                   hipStream_t st, int64_t* chunk, int64_t* n_chunks);
void qc_sweep32_noise_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dnoise,
                                  int64_t chunk, int64_t n_chunks, double* gs, double* gn, hipStream_t st);
// "mfma64-sweep" handles with `wide64_noise`: grows h->dTot and launches qc_sweep_mfma64_kernel<true> on `st` (qc_sweep64.hip), one workgroup
// per (sample, chunk) (totals as qc_sweep64_launch_totals), and the backward walk qc_sweep64_noise_grad_kernel (qc_sweep64_noise.hip; gs: S x (T-1) x nd,
// gn: S x (T-1) x p, either may be NULL; x and lambda at the chunk ends from h->dXs / h->dLs).  QC_OK or the launch's code
__attribute__((visibility("hidden"))) int qc_sweep64_noise_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale,
                                                                          const double* dnoise, hipStream_t st, int64_t* chunk, int64_t* n_chunks);
__attribute__((visibility("hidden"))) int qc_sweep64_noise_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale,
                                                                        const double* dnoise, int64_t chunk, int64_t n_chunks, double* gs, double* gn,
                                                                        hipStream_t st);
