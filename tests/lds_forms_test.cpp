// The LDS budget of the LDS / global-workspace kernels (qc_lds_kernels.hip, qc_lds_exp_hess.hip), as a table: one line per case of
// tests/test_lds_chunk_forms.py, printed by the device-free half of qc_create (qc_blueprint_build) and the plan function.  No GPU:
// that file builds this one against libqcolloc_hip.so (the build line of tests/kernel_plan_test.cpp), feeds it its case lists and
// compares every line with its own restatement of the four layouts, the four chunk rules and the 160 KiB switch.
// usage: lds_forms_test CASES.txt -- one case per line,
//   id order(0 = exponential) N state_cols m T zdim off_U off_a off_dt kernel(0 auto, 1 mfma, 2 lds) hermitian hess_align n_deriv {x_off dx_off dim}
// prints: id | jchunk lds_bytes_jac lds_bytes_hess use_ws ws_stride | F + dF, mu_d2F, one call (qc_kernel_name)
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "qc_internal.h"
#include "qc_plan.h"

namespace {

// (m + 1) dense generators, column-major n x n, drift first: exactly antisymmetric, or (hermitian = 0) one entry of the first drive off
std::vector<double> generators(int n, int m, bool hermitian) {
    std::vector<double> G((size_t)(m + 1) * n * n, 0.0);
    auto at = [&](int k, int r, int c) -> double& { return G[(size_t)k * n * n + (size_t)c * n + r]; };
    for (int k = 0; k <= m; ++k)
        for (int c = 0; c < n; ++c)
            for (int r = 0; r < c; ++r) {
                const double v = 0.125 * ((r * 7 + c * 3 + k * 5) % 11 + 1);
                at(k, r, c) = v;
                at(k, c, r) = -v;
            }
    if (!hermitian) at(m > 0 ? 1 : 0, 0, 1) += 0.5;
    return G;
}

int run_case(FILE* f) {
    char id[128];
    int order, N, cols, m, T, zdim, off_U, off_a, off_dt, kernel, herm, align, n_deriv;
    const int got = fscanf(f, "%127s %d %d %d %d %d %d %d %d %d %d %d %d %d", id, &order, &N, &cols, &m, &T, &zdim, &off_U, &off_a, &off_dt, &kernel, &herm, &align,
                           &n_deriv);
    if (got == EOF) return 0;
    if (got != 14 || n_deriv < 0 || n_deriv > QC_MAX_DERIV) { fprintf(stderr, "malformed case line (%d fields)\n", got); return -1; }
    qc_desc d;
    memset(&d, 0, sizeof(d));
    for (int i = 0; i < n_deriv; ++i)
        if (fscanf(f, "%d %d %d", &d.deriv_x_off[i], &d.deriv_dx_off[i], &d.deriv_dim[i]) != 3) { fprintf(stderr, "%s: malformed integrator\n", id); return -1; }
    const std::vector<double> G = generators(2 * N, m, herm != 0);
    d.N = N;
    d.m = m;
    d.T = T;
    d.zdim = zdim;
    d.off_U = off_U;
    d.off_a = off_a;
    d.off_dt = off_dt;
    d.dt_fixed = 0.17;
    d.integrator = order ? QC_PADE : QC_EXPONENTIAL;
    d.pade_order = order ? order : 4;
    d.n_deriv = n_deriv;
    d.G_drift = G.data();
    d.G_drives = G.data() + (size_t)4 * N * N;
    d.kernel = kernel == 0 ? QC_KERNEL_AUTO : (kernel == 1 ? QC_KERNEL_MFMA : QC_KERNEL_LDS);
    d.state_cols = cols;
    d.hess_align = align;
    qc_blueprint B;
    std::string err;
    const int rc = qc_blueprint_build(&d, &B, &err);
    if (rc) { printf("%s | refused %d %s\n", id, rc, err.c_str()); return 1; }
    qc_handle h;
    h.prm = B.prm;
    h.dims = B.dims;
    h.cls = B.cls;
    h.plan = qc_plan(h.prm, h.cls);      // (qc_kernel_name reads the handle's plan)
    printf("%s | %d %zu %zu %d %lld | %s %s %s\n", id, h.prm.jchunk, B.lds_bytes_jac, B.lds_bytes_hess, h.prm.use_ws, h.prm.ws_stride, qc_kernel_name(&h, 0),
           qc_kernel_name(&h, 1), qc_kernel_name(&h, 2));
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES.txt\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int rc;
    while ((rc = run_case(f)) > 0) {}
    fclose(f);
    return rc < 0 ? 1 : 0;
}
