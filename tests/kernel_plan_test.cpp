// Which kernels serve a handle, as a table: one line per descriptor of a sweep over integrators, sizes, state kinds, drive counts,
// generator kinds, trajectory lengths and the forced kernel classes, printed by the device-free half of qc_create
// (qc_blueprint_build) and the plan function (qc_plan, qc_plan.cpp).  No GPU: tests/test_kernel_plan.py builds this file against
// libqcolloc_hip.so, runs it and compares the output byte for byte with tests/golden/kernel_selection.txt, which was recorded
// from the predicate chains the library had before it had a plan function.  After the cases: every name qc_kernel_name gave for a kernel.
// usage: kernel_plan_test full | switches | enumerators
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "qc_internal.h"
#include "qc_plan.h"

namespace {

enum GKind { G_DENSE = 0, G_PERM = 1, G_NONANTI = 2 };
const char* const kGName[] = {"dense", "perm", "nonanti"};
enum SKind { S_UNITARY = 0, S_KETS = 1, S_DENSITY = 2 };
const char* const kSName[] = {"unitary", "kets", "density"};

struct Case {
    int order;      // Pade order, 0 = the exponential integrator
    int N, m, gkind, skind;
    bool free_dt;
    int n_int, kernel;
    int chunk;      // > 0: the parameters of one chunk of the direct host path (copies = 1, `chunk` intervals)
};

// (m + 1) generators, column-major n x n, drift first
std::vector<double> generators(int n, int m, int gkind) {
    std::vector<double> G((size_t)(m + 1) * n * n, 0.0);
    auto at = [&](int k, int r, int c) -> double& { return G[(size_t)k * n * n + (size_t)c * n + r]; };
    for (int k = 0; k <= m; ++k) {
        if (k == 0 || gkind != G_PERM) {                     // dense, exactly antisymmetric
            for (int c = 0; c < n; ++c)
                for (int r = 0; r < c; ++r) {
                    const double v = 0.125 * ((r * 7 + c * 3 + k * 5) % 11 + 1);
                    at(k, r, c) = v;
                    at(k, c, r) = -v;
                }
        } else {                                             // one entry per row: a signed permutation (a Pauli string's generator)
            const double w = 0.25 * k;
            if (k & 1) for (int r = 0; r < n / 2; ++r) { at(k, r, r + n / 2) = w; at(k, r + n / 2, r) = -w; }
            else for (int r = 0; r < n; r += 2) { at(k, r, r + 1) = w; at(k, r + 1, r) = -w; }
        }
    }
    if (gkind == G_NONANTI) at(m > 0 ? 1 : 0, 0, 1) += 0.5;
    return G;
}

const char* kernel_class_name(int k) { return k == QC_KERNEL_AUTO ? "auto" : (k == QC_KERNEL_MFMA ? "mfma" : "lds"); }

struct Setup { qc_handle h; };

int setup(const qc_desc* d, const std::vector<double>&, Setup* S) {
    qc_blueprint B;
    std::string err;
    const int rc = qc_blueprint_build(d, &B, &err);
    if (rc) return rc;
    S->h.prm = B.prm;
    S->h.dims = B.dims;
    S->h.cls = B.cls;
    return QC_OK;
}

struct Row { const char *jac, *hess, *fused; bool compact, batch_jac, batch_hess, hess_chunks; size_t scratch; };

Row row_of(const Setup& S) {
    const QcPlan& p = S.h.plan;
    return Row{qc_jac_kernel_id(p.jac), qc_hess_kernel_id(p.hess), qc_fused_kernel_id(p.fused), p.compact, p.batch_jac, p.batch_hess, p.hess_chunks,
               p.hess_scratch_doubles};
}
const char* class_of(const Setup& S) { return S.h.cls.kernel == QC_KERNEL_MFMA ? "mfma" : "lds"; }


std::set<std::string> g_names;

void run_case(const Case& c) {
    const int N = c.N, n = 2 * N, m = c.m;
    const int nc = c.skind == S_UNITARY ? N : (c.skind == S_KETS ? std::max(1, N / 2) : 1);
    const int s = n * nc;
    const std::vector<double> G = generators(n, m, c.gkind);
    qc_desc d;
    memset(&d, 0, sizeof(d));
    d.N = N;
    d.m = m;
    d.T = c.n_int + 1;
    d.zdim = s + m + (c.free_dt ? 1 : 0);
    d.off_U = 0;
    d.off_a = s;
    d.off_dt = c.free_dt ? s + m : -1;
    d.dt_fixed = 0.1;
    d.integrator = c.order ? QC_PADE : QC_EXPONENTIAL;
    d.pade_order = c.order;
    d.G_drift = G.data();
    d.G_drives = G.data() + (size_t)n * n;
    d.kernel = c.kernel;
    d.state_cols = c.skind == S_UNITARY ? 0 : nc;
    char what[96];
    snprintf(what, sizeof(what), "%s%d N=%d %s %s m=%d %s n=%d %s c=%d", c.order ? "pade" : "exp", c.order, N, kSName[c.skind], c.free_dt ? "free" : "fixed", m,
             kGName[c.gkind], c.n_int, kernel_class_name(c.kernel), c.chunk);
    Setup S;
    const int rc = setup(&d, G, &S);
    if (rc) { printf("%s | refused %d\n", what, rc); return; }
    if (c.chunk > 0) {      // a chunk of the direct host path: one copy of the replicated blocks, `chunk` intervals from the middle
        S.h.prm.copies = 1;
        S.h.prm.t_begin += c.chunk;
        S.h.prm.n_int = c.chunk;
    }
    S.h.plan = qc_plan(S.h.prm, S.h.cls);      // (qc_kernel_name reads the handle's plan)
    const Row r = row_of(S);
    // class | F + dF, mu_d2F, one call | compact, batched F + dF, batched mu_d2F, Hessian chunks; scratch doubles
    printf("%s | %s %s %s %s | %d%d%d%d %zu\n", what, class_of(S), r.jac, r.hess, r.fused, (int)r.compact, (int)r.batch_jac, (int)r.batch_hess, (int)r.hess_chunks,
           r.scratch);
    // the names qc_kernel_name gives, once per (question, kernel): several names for one kernel show as several lines
    const char* const ids[3] = {r.jac, r.hess, r.fused};
    for (int w = 0; w < 3; ++w) g_names.insert(std::string(w == 0 ? "jac " : (w == 1 ? "hess " : "fused ")) + ids[w] + " " + qc_kernel_name(&S.h, w));
}

const int kSizes[] = {2, 3, 4, 5, 8, 9, 12, 16, 32, 40};
const int kDrives[] = {0, 1, 2, 4, 5, 6, 7, 8, 9, 14, 15, 33};
const int kLengths[] = {1, 1024, 1025, 1536, 1537, 2048, 2049, 4096, 4097};

// generator kinds at the sizes the switches act on, and the length thresholds at 2N = 16
void sweep_switches() {
    for (int order : {4, 0})
        for (int N : {8, 16})
            for (int m : {1, 6})
                for (int g = 0; g < 3; ++g) run_case(Case{order, N, m, g, S_UNITARY, true, 1000, QC_KERNEL_AUTO, 0});
    for (int m : {2, 6})
        for (int g = 0; g < 2; ++g)
            for (int len : kLengths) run_case(Case{4, 8, m, g, S_UNITARY, true, len, QC_KERNEL_AUTO, 0});
}

void sweep_full() {
    // every size and drive count at order 4 and the exponential integrator, the other orders at fewer: a unitary, free timestep, dense drives
    for (int order : {4, 0})
        for (int N : kSizes)
            for (int m : kDrives)
                if (N == 8 || N == 16 || N == 32 || m == 0 || m == 2 || m == 8 || m == 9 || m == 33)      // (every drive count at the tile sizes)
                    run_case(Case{order, N, m, G_DENSE, S_UNITARY, true, 1000, QC_KERNEL_AUTO, 0});
    for (int order : {2, 6, 12, 20})
        for (int N : {2, 8, 9, 16, 40})
            for (int m : {0, 8, 9}) run_case(Case{order, N, m, G_DENSE, S_UNITARY, true, 1000, QC_KERNEL_AUTO, 0});
    // state kinds, timestep and generator kinds at the sizes of the MFMA kernels (N = 4: padded tiles)
    for (int order : {4, 0})
        for (int N : {4, 8, 16})
            for (int m : {1, 6})
                for (int sk = 0; sk < (order ? 2 : 3); ++sk)
                    for (int ft = 1; ft >= 0; --ft)
                        for (int g = 0; g < 3; ++g)
                            if (N != 4 || m == 6) run_case(Case{order, N, m, g, sk, ft == 1, 1000, QC_KERNEL_AUTO, 0});
    // the length thresholds at 2N = 16 (N = 4: the masked instantiations)
    for (int m : {2, 5, 6})
        for (int g = 0; g < 2; ++g)
            for (int len : kLengths) run_case(Case{4, 8, m, g, S_UNITARY, true, len, QC_KERNEL_AUTO, 0});
    for (int len : kLengths) run_case(Case{4, 4, 6, G_DENSE, S_UNITARY, true, len, QC_KERNEL_AUTO, 0});
    // no drives and a fixed timestep: the constraint is linear, there is no Hessian
    for (int order : {4, 6, 0})
        for (int N : {4, 8, 16, 32}) run_case(Case{order, N, 0, G_DENSE, S_UNITARY, false, 1000, QC_KERNEL_AUTO, 0});
    // the forced classes, refusals included
    for (int order : {4, 6, 0})
        for (int N : {8, 16, 32, 40})
            for (int m : {2, 33})
                for (int k : {QC_KERNEL_MFMA, QC_KERNEL_LDS}) run_case(Case{order, N, m, G_DENSE, S_UNITARY, true, 1000, k, 0});
    // chunks of the direct host path
    for (int N : {2, 8, 16})
        for (int g = 0; g < 2; ++g)
            for (int sk = 0; sk < 2; ++sk) run_case(Case{4, N, 6, g, sk, true, 1000, QC_KERNEL_AUTO, 63});
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "full";
    if (mode == "full") sweep_full();
    else if (mode == "switches") sweep_switches();
    else if (mode == "enumerators") {
        for (int k = 0; k < QC_JAC_KERNELS; ++k) printf("jac %s\n", qc_jac_kernel_id((QcJacKernel)k));
        for (int k = 0; k < QC_HESS_KERNELS; ++k) printf("hess %s\n", qc_hess_kernel_id((QcHessKernel)k));
        for (int k = 0; k < QC_FUSED_KERNELS; ++k) printf("fused %s\n", qc_fused_kernel_id((QcFusedKernel)k));
    } else { fprintf(stderr, "usage: %s full | switches | enumerators\n", argv[0]); return 2; }
    for (const std::string& n : g_names) printf("name %s\n", n.c_str());
    return 0;
}
