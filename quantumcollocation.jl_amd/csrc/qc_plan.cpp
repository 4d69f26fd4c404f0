// Which kernel serves a handle (qc_plan.h).  The ORDER OF PREFERENCE between the kernel families lives here and nowhere else; what a
// single family can serve -- limits tied to constants of its own file -- is a predicate next to that kernel, called from here only.
#include "qc_plan.h"

#include <stdlib.h>

namespace {

int env_int(const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
}

QcSwitches read_switches() {
    QcSwitches s;
    s.no_fused = env_int("QC_NO_FUSED", 0) != 0;
    s.ell_jac = env_int("QC_ELL_JAC", 1) != 0;
    s.hess_g2 = env_int("QC_HESS_G2", 1) != 0;
    s.hess_ell = env_int("QC_HESS_ELL", 1) != 0;
    s.hess_two_waves = env_int("QC_HESS_TWO_WAVES", 1) != 0;
    s.fused_ell = env_int("QC_FUSED_ELL", -1);
    s.exp_ell = env_int("QC_EXP_ELL", 1) != 0;
    s.list_batch = env_int("QC_LIST_BATCH", 1) != 0;
    return s;
}

struct Name { const char *id, *name; };
const Name kJacNames[QC_JAC_KERNELS] = {
    {"LDS", "lds"}, {"LDS_GWS", "lds-gws"},
    {"EXP16", "mfma16-exp"}, {"EXP16_GATHER", "mfma16-exp-gather"}, {"EXP32", "mfma32-exp"}, {"EXP32_GATHER", "mfma32-exp-gather"},
    {"PADEP16", "mfma16-padeP"}, {"PADE4_64", "mfma64-pade4"}, {"PADE4_32_ELL", "mfma32-pade4-ell"}, {"PADE4_32", "mfma32-pade4"},
    {"PADE4_16", "mfma16-pade4"},
};
const Name kHessNames[QC_HESS_KERNELS] = {
    {"LDS", "lds-hess"}, {"LDS_GWS", "lds-gws-hess"}, {"LDS_EXP", "lds-exp-hess"}, {"LDS_GWS_EXP", "lds-gws-exp-hess"},
    {"EXP16", "mfma16-exp-hess"}, {"EXP16_GATHER", "mfma16-exp-hess-gather"}, {"EXP32", "mfma32-exp-hess"}, {"EXP32_GATHER", "mfma32-exp-hess-gather"},
    {"PADEP16", "mfma16-padeP-hess"}, {"PADE4_64", "mfma64-pade4-hess"}, {"PADE4_32_ELL", "mfma32-pade4-hess-ell"}, {"PADE4_32", "mfma32-pade4-hess"},
    // (two kernels behind one name: qc_mfma_hess_g2.hip and the one-wave kernel's row-gather form)
    {"PADE4_16_G2", "mfma16-pade4-hess-gather"}, {"PADE4_16_GATHER", "mfma16-pade4-hess-gather"}, {"PADE4_16_TWO_WAVES", "mfma16-pade4-hess2"},
    {"PADE4_16", "mfma16-pade4-hess"},
};
const Name kFusedNames[QC_FUSED_KERNELS] = {
    {"TWO_LAUNCHES", "two-launches"}, {"PADE4_16", "mfma16-pade4-fused"}, {"PADE4_16_GATHER", "mfma16-pade4-fused-gather"},
    {"PADE4_32_ELL", "mfma32-pade4-fused-ell"},
};

const Name kJvpNames[QC_PROD_KERNELS] = {{"GENERIC", "generic-jvp"}, {"PADE4_16", "mfma16-pade4-jvp"}};
const Name kVjpNames[QC_PROD_KERNELS] = {{"GENERIC", "generic-vjp"}, {"PADE4_16", "generic-vjp"}};      // (there is no fused transposed kernel)
const Name kHvpNames[QC_PROD_KERNELS] = {{"GENERIC", "generic-hvp"}, {"PADE4_16", "generic-hvp"}};      // (... and no fused Hessian-product kernel)

// The two-wave mu_d2F kernel (qc_mfma_hess2.hip) serves launches of up to one round of the device (four workgroups per CU): measured
// against the one-wave kernel (profiles/r03_hess2_ab.txt) 6.1 - 6.8 / 7.0 / 8.6 us against 7.1 / 7.5 / 8.7 at T = 250 / 500 / 1000; beyond
// one round the one-wave kernel's persistent grid is faster (T = 2000: 15.1 against 17.3 us; T = 8000: 47.7 against 52.9).
constexpr int kTwoWavesMaxIntervals = 1024;

// The one-call kernel's row-gather form serves trajectories of one to four device rounds (four workgroups per CU: 1024 intervals a
// round): there the matrix pipes decide how fast workgroups retire and make room -- T = 1500 / 2000 / 3000 / 4000: 21.6 / 25.5 / 36.3 /
// 44.0 us against 22.7 / 26.4 / 37.3 / 45.9 with the dense images, on every box measured -- while a single round follows its store stream
// and is 0.3 - 0.7 us FASTER with the images (T = 1000: 12.8 against 13.5), and long streams are decided by the box: T = 6000 ... 32000
// lose 2 - 4 % with the gathers on two boxes and win 6 - 8 % (T = 16000: 143 - 148 against 155 - 156 us) on a third
// (profiles/r05_fused_ell16.txt: A/B inside one process on the same buffers, profiles/fused_ab.py -- across processes long streams are
// bimodal).
constexpr int kFusedGatherMinIntervals = 1025, kFusedGatherMaxIntervals = 4096;

// F + dF of an MFMA handle before the row-gather forms are considered, or -1: no MFMA kernel writes it
int mfma_jac(const QcParams& P) {
    if (qc_mfma_exp_supported(P)) return QC_JAC_EXP16;
    if (qc_mfma32_exp_supported(P)) return QC_JAC_EXP32;
    if (qc_mfma16_padeP_supported(P)) return QC_JAC_PADEP16;
    if (qc_mfma64_supported(P)) return QC_JAC_PADE4_64;
    if (qc_mfma_pade4_supported(P)) return P.n > 16 ? QC_JAC_PADE4_32 : QC_JAC_PADE4_16;
    return -1;
}

}  // namespace

QcJacKernel qc_plan_jac(const QcParams& P, const QcClass& cls, const QcSwitches& sw) {
    const int k = cls.kernel == QC_KERNEL_MFMA ? mfma_jac(P) : -1;
    const bool exp_rows = cls.ell16 && sw.exp_ell;      // drive generators with one entry per row: the row-gather form of the Horner steps
    switch (k) {
        case QC_JAC_EXP16: return exp_rows ? QC_JAC_EXP16_GATHER : QC_JAC_EXP16;
        case QC_JAC_EXP32: return exp_rows ? QC_JAC_EXP32_GATHER : QC_JAC_EXP32;
        case QC_JAC_PADE4_32: return P.ell_R > 0 && sw.ell_jac ? QC_JAC_PADE4_32_ELL : QC_JAC_PADE4_32;      // sparse drive generators: qc_mfma32_ell.hip
        case -1: return P.use_ws ? QC_JAC_LDS_GWS : QC_JAC_LDS;
        default: return (QcJacKernel)k;
    }
}

QcHessKernel qc_plan_hess(const QcParams& P, const QcClass& cls, const QcSwitches& sw) {
    if (cls.kernel == QC_KERNEL_MFMA) {
        const bool exp_rows = cls.ell16 && sw.exp_ell;
        if (qc_mfma_exp_hess_supported(P)) return exp_rows ? QC_HESS_EXP16_GATHER : QC_HESS_EXP16;
        if (qc_mfma32_exp_hess_supported(P)) return exp_rows ? QC_HESS_EXP32_GATHER : QC_HESS_EXP32;
        if (qc_mfma16_padeP_hess_supported(P)) return QC_HESS_PADEP16;
        if (qc_mfma64_hess_supported(P)) return QC_HESS_PADE4_64;
        if (qc_mfma32_hess_supported(P)) return P.ell_R > 0 ? QC_HESS_PADE4_32_ELL : QC_HESS_PADE4_32;
        if (qc_mfma16_hess_supported(P)) {
            // Drive generators with one entry per row (cls.ell16): qc_mfma_hess_g2.hip (round 6) first, then the row-gather form of the
            // one-wave kernel.  mu_d2F alone takes that form wherever the handle's drives allow it: the launch is a latency chain per
            // interval, mostly the 68 dependent f64 MFMAs -- 20 with the gathers -- and, holding no drive image through stage B, the form
            // keeps its stage-A tiles in registers instead of LDS: 14 KB of LDS and 217 registers, EIGHT workgroups per CU (the
            // dense-image form: six; round 4: four).  T = 1000 / 2000 / 4000 / 8000 / 32000: 8.1 / 11.5 / 20.4 / 38.1 / 120 us against 8.7
            // (two-wave kernel) / 15.7 / 23.9 / 42.3 / 140 with the gathers but six per CU, and 8.7 / 15.4 / 25.9 / 47.2 / 173 in round 4
            // (profiles/r05_hess_long.txt).
            const bool rows = cls.ell16 && sw.hess_ell;
            if (rows && sw.hess_g2 && qc_mfma16_hess_g2_supported(P, cls)) return QC_HESS_PADE4_16_G2;
            if (rows && qc_mfma16_hess_gather_supported(P, cls)) return QC_HESS_PADE4_16_GATHER;
            // Two waves per interval up to one round of the device (qc_mfma_hess2.hip) -- behind the row-gather form, which keeps eight
            // workgroups per CU resident and is faster at every length (T = 750 / 1000: 7.85 / 8.12 against 8.08 / 8.74 us)
            if (sw.hess_two_waves && P.n_int <= kTwoWavesMaxIntervals && qc_mfma16_hess2_supported(P, cls)) return QC_HESS_PADE4_16_TWO_WAVES;
            return QC_HESS_PADE4_16;
        }
    }
    // (an MFMA handle with more drives than its Hessian kernel holds ends here too)
    if (P.integrator != QC_PADE) return P.use_ws ? QC_HESS_LDS_GWS_EXP : QC_HESS_LDS_EXP;
    return P.use_ws ? QC_HESS_LDS_GWS : QC_HESS_LDS;
}

QcFusedKernel qc_plan_fused(const QcParams& P, const QcClass& cls, const QcSwitches& sw) {
    if (sw.no_fused || cls.kernel != QC_KERNEL_MFMA) return QC_FUSED_TWO_LAUNCHES;
    if (qc_mfma16_fused_supported(P, cls)) {
        const bool by_length = P.n_int >= kFusedGatherMinIntervals && P.n_int <= kFusedGatherMaxIntervals;
        return cls.ell16 && sw.fused_ell != 0 && (sw.fused_ell == 1 || by_length) ? QC_FUSED_PADE4_16_GATHER : QC_FUSED_PADE4_16;
    }
    if (P.ell_R > 0 && P.hess_nnz) return QC_FUSED_PADE4_32_ELL;      // sparse drive generators at 2N = 32: qc_mfma32_ell.hip
    return QC_FUSED_TWO_LAUNCHES;
}

// dF v: the fused matrix-free kernel where it serves the handle (order-4 Pade, 2N <= 16, up to 8 state columns and 8 drives:
// qc_mfma_products.hip), else the generic path -- the handle's own dF launch into a scratch, then a product kernel (qc_products.hip).
// dF' lam: always the generic path.  A fused transposed kernel (one wave per knot) was built and measured at config 3 ABOVE the
// F + dF launch that a fused product has to beat (profiles/products_summary.txt), so it is not part of the library.
QcProductKernel qc_plan_product(const QcParams& P, const QcClass& cls) { return qc_mfma16_products_supported(P, cls) ? QC_PROD_PADE4_16 : QC_PROD_GENERIC; }

const QcSwitches& qc_switches() {
    static QcSwitches s = read_switches();
#ifdef QC_FUSED_ELL_DYNAMIC      /* experiment builds: this switch is read at every launch (A/B inside one process, on the same buffers) */
    s.fused_ell = env_int("QC_FUSED_ELL", -1);
#endif
    return s;
}

QcCreateSwitches qc_create_switches() { return QcCreateSwitches{env_int("QC_NO_ELL", 0) != 0, env_int("QC_NO_ANTISYM", 0) != 0, env_int("QC_NO_HEAD", 0) != 0,
                                                                      env_int("QC_NO_PRODUCT_MFMA", 0) != 0}; }

bool qc_plan_mfma_serves(const QcParams& P) { return mfma_jac(P) >= 0; }

QcPlan qc_plan(const QcParams& P, const QcClass& cls, const QcSwitches& sw) {
    QcPlan p;
    p.jac = qc_plan_jac(P, cls, sw);
    p.hess = qc_plan_hess(P, cls, sw);
    p.fused = qc_plan_fused(P, cls, sw);
    p.compact = p.jac == QC_JAC_PADE4_32_ELL || p.jac == QC_JAC_PADE4_32 || p.jac == QC_JAC_PADE4_16;      // the order-4 kernels up to 2N = 32
    p.batch_jac = cls.kernel == QC_KERNEL_MFMA && qc_mfma16_batchable(P, cls);
    p.batch_hess = p.batch_jac && P.m <= 8 && P.hess_nnz > 0 && p.hess >= QC_HESS_EXP16;
    p.hess_chunks = p.hess >= QC_HESS_PADE4_32_ELL;      // the order-4 kernels up to 2N = 32
    p.hess_scratch_doubles = p.hess == QC_HESS_PADE4_64 ? qc_mfma64_hess_scratch_doubles(P) : 0;      // (128 MiB)
    p.jvp = qc_plan_product(P, cls);
    p.vjp = QC_PROD_GENERIC;
    p.hvp = QC_PROD_GENERIC;      // (mu d2F) v: the handle's own mu_d2F launch into a scratch, then the product kernel of qc_products.hip
    return p;
}

// One launch for a list: every member may join the batched launch of its kind (QcPlan.batch_jac / batch_hess; the landing layout is
// written by the kernels that honour QcParams.copies), and everything the launch takes from the leader alone is the same for all of
// them -- the grid (n_int), the instantiation (drive-count class from m, masked or unmasked tile from n and nc; mu_d2F: the kernel for
// antisymmetric generators or the general one) -- as is the trajectory they read (zdim, t_begin).  gridDim.y is a 16-bit quantity.
bool qc_plan_list(const QcParams* const* members, const QcPlan* const* plans, int count, QcListLaunch what) {
    if (count < 2 || count > 65535) return false;
    const QcParams& P0 = *members[0];
    for (int i = 0; i < count; ++i) {
        const QcParams& P = *members[i];
        const QcPlan& p = *plans[i];
        if (!(what == QC_LIST_HESS ? p.batch_hess : p.batch_jac)) return false;
        if (what == QC_LIST_LANDING && !p.compact) return false;
        if (what == QC_LIST_HESS && P.antisym != P0.antisym) return false;
        if (P.n_int != P0.n_int || P.t_begin != P0.t_begin || P.zdim != P0.zdim || P.m != P0.m || P.n != P0.n || P.nc != P0.nc) return false;
    }
    return true;
}

const char* qc_jac_kernel_name(QcJacKernel k) { return kJacNames[k].name; }
const char* qc_hess_kernel_name(QcHessKernel k) { return kHessNames[k].name; }
const char* qc_fused_kernel_name(QcFusedKernel k) { return kFusedNames[k].name; }
const char* qc_jvp_kernel_name(QcProductKernel k) { return kJvpNames[k].name; }
const char* qc_vjp_kernel_name(QcProductKernel k) { return kVjpNames[k].name; }
const char* qc_hvp_kernel_name(QcProductKernel k) { return kHvpNames[k].name; }
const char* qc_jac_kernel_id(QcJacKernel k) { return kJacNames[k].id; }
const char* qc_hess_kernel_id(QcHessKernel k) { return kHessNames[k].id; }
const char* qc_fused_kernel_id(QcFusedKernel k) { return kFusedNames[k].id; }
