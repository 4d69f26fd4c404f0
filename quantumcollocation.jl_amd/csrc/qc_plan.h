// Which kernel serves a handle: one function answers it for the launches, for qc_kernel_name and for the host-buffer paths.
// Host only.  DESIGN.md "Which kernel serves a handle" is this file's table in words.
#pragma once

#include "qc_internal.h"

// The run-time switches that choose between families, read once per process (A/B diagnostics; none is set in normal use).
struct QcSwitches {
    bool no_fused;         // QC_NO_FUSED=1: dF + mu_d2F always as two launches
    bool ell_jac;          // QC_ELL_JAC=0: F + dF at 2N = 32 from the dense images although the row-gather tables exist
    bool hess_g2;          // QC_HESS_G2=0: never qc_mfma_hess_g2.hip
    bool hess_ell;         // QC_HESS_ELL=0: no row-gather form of mu_d2F at 2N = 16
    bool hess_two_waves;   // QC_HESS_TWO_WAVES=0: never qc_mfma_hess2.hip
    int fused_ell;         // QC_FUSED_ELL=0 / 1: the one-call kernel's row-gather form never / always (-1: by length)
    bool exp_ell;          // QC_EXP_ELL=0: the exponential kernels' dense-image forms
    bool list_batch;       // QC_LIST_BATCH=0: the host-buffer list calls launch member by member
};
const QcSwitches& qc_switches();
// ... and the two that act through the facts of a handle, read whenever one is created (the tests create handles either way in one process)
struct QcCreateSwitches {
    bool no_ell;           // QC_NO_ELL=1: no row-gather tables are built at all
    bool no_antisym;       // QC_NO_ANTISYM=1: the generators are treated as not antisymmetric
    bool no_head;          // QC_NO_HEAD=1: the 2N = 16 F + dF launch never takes its HEAD instantiation (A/B runs, tests)
    bool no_product_mfma;  // QC_NO_PRODUCT_MFMA=1: dF v takes the generic path although the fused kernel serves the handle (A/B runs, tests)
};
QcCreateSwitches qc_create_switches();

// Pure.  `P` is a handle's own parameter block or a copy with another n_int / t_begin / copies (chunks, the compact host layout).
QcPlan qc_plan(const QcParams& P, const QcClass& cls, const QcSwitches& sw = qc_switches());
// ... and its three answers one by one (a launch on a copy of the parameters asks one)
QcJacKernel qc_plan_jac(const QcParams& P, const QcClass& cls, const QcSwitches& sw = qc_switches());
QcHessKernel qc_plan_hess(const QcParams& P, const QcClass& cls, const QcSwitches& sw = qc_switches());
QcFusedKernel qc_plan_fused(const QcParams& P, const QcClass& cls, const QcSwitches& sw = qc_switches());
QcProductKernel qc_plan_product(const QcParams& P, const QcClass& cls);      // dF v (dF' lam always takes the generic path)
bool qc_plan_mfma_serves(const QcParams& P);      // some MFMA kernel writes F + dF of this descriptor (qc_create: MFMA or LDS)

// Can the members of a list share ONE launch (gridDim.y = count, each workgroup reading its member's parameter block from device
// memory)?  The whole condition, for the three places such a launch starts from: the device-resident F + dF and mu_d2F entry points
// ("_dev_multi") and the host-buffer Jacobian path, which launches the members' landing layouts.  Pure; `plans[i]` is qc_plan of
// `members[i]` (a landing layout changes the placement and the copies of a member, none of the fields read here).
enum QcListLaunch { QC_LIST_F_JAC = 0, QC_LIST_HESS = 1, QC_LIST_LANDING = 2, QC_LIST_LAUNCHES };
bool qc_plan_list(const QcParams* const* members, const QcPlan* const* plans, int count, QcListLaunch what);

const char* qc_jac_kernel_name(QcJacKernel k);     // what qc_kernel_name returns
const char* qc_hess_kernel_name(QcHessKernel k);
const char* qc_fused_kernel_name(QcFusedKernel k);
const char* qc_jvp_kernel_name(QcProductKernel k);   // qc_kernel_name(h, 3)
const char* qc_vjp_kernel_name(QcProductKernel k);   // qc_kernel_name(h, 4)
const char* qc_hvp_kernel_name(QcProductKernel k);   // qc_kernel_name(h, 5)
const char* qc_jac_kernel_id(QcJacKernel k);       // the enumerator without its prefix (tests/kernel_plan_test.cpp)
const char* qc_hess_kernel_id(QcHessKernel k);
const char* qc_fused_kernel_id(QcFusedKernel k);
