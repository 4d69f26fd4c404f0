// What qc_sweep.hip (forward sweep), qc_sweep_grad.hip (its adjoint), qc_sweep_vjp.hip (the pullback of the final states) and
// qc_sweep_jvp.hip (their pushforward) share: the handle, the descriptor checks and the launch of the forward chunk totals (with it
// the chunk rule).  Not part of the ABI.
#pragma once

#include <string>

#include "qc_side.h"

struct qc_sweep : qc_side {
    qc_sweep_desc d;             // caller-owned arrays are not retained (pointers nulled)
    bool mfma = false;
    bool mfma32 = false;         // the 2 x 2-tile form of a wide descriptor ("mfma32-sweep", qc_sweep32.hip); mfma is set as well
    bool grad_ok = false;        // the gradient's scope (qc_sweep_grad.hip), decided at create from the caller's matrices
    std::string grad_why;        // when not: the reason
    bool vjp_ok = false;         // the pullback's scope (qc_sweep_vjp.hip): the gradient's without its fidelity conditions
    std::string vjp_why;
    bool jvp_ok = false;         // the pushforward's scope (qc_sweep_jvp.hip): "mfma16-sweep" handles, any generators
    std::string jvp_why;
    int n = 0, nc = 0, ns = 0, fid_n = 0;
    int64_t Zlen = 0;
    double* dG = nullptr;        // (1 + m + p) matrices, column-major (per-sample form)
    double* dImg = nullptr;      // their A-layout images (MFMA form)
    double *dgr = nullptr, *dgi = nullptr;
    // scratch of the "_dev" entry point, grown at the first call that needs it
    double* dTot = nullptr;  size_t capTot = 0;
    double* dFin = nullptr;  size_t capFin = 0;
    double *dGs = nullptr, *dRE = nullptr, *dRQ = nullptr, *dRS = nullptr, *dRout = nullptr;
    // staging of the host-buffer entry point
    double *sZ = nullptr, *sInit = nullptr;
    double* sTheta = nullptr;  size_t capTheta = 0;
    double* sScale = nullptr;  size_t capScale = 0;
    double* sFinals = nullptr; size_t capFinals = 0;
    double* sFids = nullptr;   size_t capFids = 0;
    // gradient: states and adjoints at the chunk ends, per-sample derivatives, fidelities; staging of its host-buffer entry point
    double* dXs = nullptr;   size_t capXs = 0;
    double* dLs = nullptr;   size_t capLs = 0;
    double* dGsamp = nullptr; size_t capGsamp = 0;
    double* dGfid = nullptr; size_t capGfid = 0;
    double* sW = nullptr;    size_t capW = 0;
    double* sGradS = nullptr; size_t capGradS = 0;
    double *sGrad = nullptr, *sJ = nullptr;
    // parameter gradients: the chunk shares S x n_chunks x (n_pert + m); staging of the host-buffer entry point
    double* dPart = nullptr; size_t capPart = 0;
    double* sGth = nullptr;  size_t capGth = 0;
    double* sGsc = nullptr;  size_t capGsc = 0;
    // pullback (qc_sweep_vjp.hip): staging of the cotangents and of grad_init in its host-buffer entry point (finals: sFinals above)
    double* sCot = nullptr;   size_t capCot = 0;
    double* sGinit = nullptr; size_t capGinit = 0;
    // pushforward (qc_sweep_jvp.hip): the chunk totals and their tangents, S x n_chunks x 2 tiles; staging of the directions and of the
    // tangent outputs in its host-buffer entry point (finals, fids: sFinals, sFids above)
    double* dTotJ = nullptr;  size_t capTotJ = 0;
    double *sVZ = nullptr, *sVinit = nullptr;
    double* sVth = nullptr;   size_t capVth = 0;
    double* sVsc = nullptr;   size_t capVsc = 0;
    double* sTfin = nullptr;  size_t capTfin = 0;
    double* sTfid = nullptr;  size_t capTfid = 0;
};

// records the message in the handle (when there is one) and in the slot qc_sweep_last_error(NULL) returns
int qc_sweep_fail(qc_side* h, int code, const std::string& msg);
std::string* qc_sweep_err_slot();
int qc_sweep_validate_desc(const qc_sweep_desc* d);
bool qc_sweep_desc_is_mfma(const qc_sweep_desc* d);
// 0: "rollout-per-sample", 1: "mfma16-sweep", 2: "mfma32-sweep" (wide descriptors with 16 < 2N <= 32)
int qc_sweep_desc_form(const qc_sweep_desc* d);
// the chunk rule of the MFMA forms
void qc_sweep_chunks(int64_t S, int64_t T, int64_t* chunk, int64_t* n_chunks);
// "mfma16-sweep" handles: grows h->dTot and launches qc_sweep_mfma16_kernel on `st` (S x n_chunks tiles of 256 doubles)
int qc_sweep_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, hipStream_t st, int64_t* chunk,
                           int64_t* n_chunks);
// "mfma32-sweep" handles (qc_sweep32.hip): the A-layout image of one n x n matrix (1024 doubles), and the launch of qc_sweep_mfma32_kernel
// (S x n_chunks column-major 32 x 32 totals of 1024 doubles in h->dTot)
void qc_sweep32_image(const double* G, int n, double* img);
int qc_sweep32_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, hipStream_t st, int64_t* chunk,
                             int64_t* n_chunks);
// "mfma32-sweep" gradients (qc_sweep32_grad.hip): qc_sweep32_seed_kernel (x and lambda at every chunk end, fidelities) and the backward walk
// qc_sweep32_grad_kernel (gs: S x (T-1) x nd); scratch is the caller's
void qc_sweep32_launch_seed(qc_sweep* h, int64_t S, int64_t n_chunks, const double* dinit, double* dfids, hipStream_t st);
void qc_sweep32_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, int64_t chunk, int64_t n_chunks,
                            double* gs, hipStream_t st);
// "mfma16-sweep" handles (qc_sweep_grad.hip): the backward walk qc_sweep_grad_kernel<M, false> (gs: S x (T-1) x nd), or with `par` the
// parameter flavour <M, true> (gs may be NULL) and qc_sweep_par_reduce_kernel out of h->dPart; scratch is the caller's
void qc_sweep16_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, int64_t chunk, int64_t n_chunks,
                            double* gs, bool par, double* dgrad_theta, double* dgrad_scale, hipStream_t st);
// device-free: is this (valid) descriptor inside the gradient's scope?  `why` receives the reason when it is not.
bool qc_sweep_grad_scope(const qc_sweep_desc* d, std::string* why);
// what the gradient and the pullback ask alike (an MFMA form, antisymmetric matrices, at most 16 state columns), and the pullback's scope
bool qc_sweep_closed_scope(const qc_sweep_desc* d, std::string* why);
bool qc_sweep_vjp_scope(const qc_sweep_desc* d, std::string* why);
// the pushforward's scope (qc_sweep_jvp.hip): the "mfma16-sweep" form, whatever the generators
bool qc_sweep_jvp_scope(const qc_sweep_desc* d, std::string* why);
