// Which kernels serve a handle, as a table: one line per descriptor of a sweep over integrators, sizes, state kinds, drive counts,
// generator kinds, trajectory lengths and the forced kernel classes, printed by the device-free half of qc_create
// (qc_blueprint_build) and the plan function (qc_plan, qc_plan.cpp).  No GPU: tests/test_kernel_plan.py builds this file against
// libqcolloc_hip.so, runs it and compares the output byte for byte with tests/golden/kernel_selection.txt, which was recorded
// from the predicate chains the library had before it had a plan function.  After the cases: every name qc_kernel_name gave for a kernel.
// `lists`: pairs and triples of descriptors, one line per list with the three answers of qc_plan_list (can the members share one
// launch: F + dF, mu_d2F, the host-buffer Jacobian path) behind the members as qc_create would see them.
// usage: kernel_plan_test full | switches | lists | enumerators
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

int columns_of(const Case& c) { return c.skind == S_UNITARY ? c.N : (c.skind == S_KETS ? std::max(1, c.N / 2) : 1); }

// the descriptor of a case; `G` keeps the generators it points at
qc_desc desc_of(const Case& c, const std::vector<double>& G) {
    const int N = c.N, n = 2 * N, m = c.m;
    const int nc = columns_of(c);
    const int s = n * nc;
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
    return d;
}

void run_case(const Case& c) {
    const int N = c.N, m = c.m;
    const std::vector<double> G = generators(2 * N, m, c.gkind);
    qc_desc d = desc_of(c, G);
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

// ---- lists: members over ONE trajectory (the knot is as wide as the widest member needs; a member may cover a range of intervals) ----
struct Member { Case c; int t_begin, t_end; };      // t_end = 0: every interval

Member whole(int order, int N, int m, int gkind = G_DENSE, int skind = S_UNITARY, bool free_dt = true, int kernel = QC_KERNEL_AUTO) {
    return Member{Case{order, N, m, gkind, skind, free_dt, 40, kernel, 0}, 0, 0};
}
Member shard(Member mb, int t_begin, int t_end) { mb.t_begin = t_begin; mb.t_end = t_end; return mb; }
Member of_length(Member mb, int n_int) { mb.c.n_int = n_int; return mb; }

void run_list(const std::vector<Member>& members, int own_zdim = -1) {
    const int count = (int)members.size();
    int zdim = 0;
    for (const Member& mb : members) zdim = std::max(zdim, 2 * mb.c.N * columns_of(mb.c) + mb.c.m + (mb.c.free_dt ? 1 : 0));
    std::vector<Setup> S((size_t)count);
    std::vector<const QcParams*> prm;
    std::vector<const QcPlan*> plans;
    std::string what;
    for (int i = 0; i < count; ++i) {
        const Case& c = members[(size_t)i].c;
        const std::vector<double> G = generators(2 * c.N, c.m, c.gkind);
        qc_desc d = desc_of(c, G);
        d.zdim = i == own_zdim ? d.zdim + 1 : zdim;      // (`own_zdim`: that member reads knots of another width -- not one trajectory)
        d.t_begin = members[(size_t)i].t_begin;
        d.t_end = members[(size_t)i].t_end;
        const int rc = setup(&d, G, &S[(size_t)i]);
        char text[128];
        snprintf(text, sizeof(text), "%s%s%d N=%d %s %s m=%d %s t=%d+%d z=%d %s", i ? " ; " : "", c.order ? "pade" : "exp", c.order, c.N, kSName[c.skind],
                 c.free_dt ? "free" : "fixed", c.m, kGName[c.gkind], rc ? -1 : (int)S[(size_t)i].h.prm.t_begin, rc ? -1 : S[(size_t)i].h.prm.n_int, d.zdim,
                 kernel_class_name(c.kernel));
        what += text;
        if (rc) { printf("list %d: %s | refused %d\n", count, what.c_str(), rc); return; }
        S[(size_t)i].h.plan = qc_plan(S[(size_t)i].h.prm, S[(size_t)i].h.cls);
        prm.push_back(&S[(size_t)i].h.prm);
        plans.push_back(&S[(size_t)i].h.plan);
    }
    // the members | one launch for F + dF, for mu_d2F, for the host-buffer Jacobian path
    printf("list %d: %s | %d %d %d\n", count, what.c_str(), (int)qc_plan_list(prm.data(), plans.data(), count, QC_LIST_F_JAC),
           (int)qc_plan_list(prm.data(), plans.data(), count, QC_LIST_HESS), (int)qc_plan_list(prm.data(), plans.data(), count, QC_LIST_LANDING));
}

void sweep_lists() {
    // equal members: every drive-count class of the batched launches, the drive counts beyond the registers of mu_d2F, full and padded tiles
    for (int N : {2, 5, 8})
        for (int m : {0, 2, 6, 8, 9, 32})
            for (int count : {2, 3}) run_list(std::vector<Member>((size_t)count, whole(4, N, m)));
    for (int N : {2, 8}) run_list({whole(4, N, 0, G_DENSE, S_UNITARY, false), whole(4, N, 0, G_DENSE, S_UNITARY, false)});      // linear: no Hessian
    run_list({whole(4, 8, 6, G_DENSE, S_KETS), whole(4, 8, 6, G_DENSE, S_KETS), whole(4, 8, 6, G_DENSE, S_KETS)});
    run_list({whole(4, 8, 3, G_PERM), whole(4, 8, 3, G_PERM)});
    run_list({whole(4, 8, 7, G_NONANTI), whole(4, 8, 7, G_NONANTI)});
    // one field apart: drives, levels, state columns, antisymmetry, timestep kind alone does not count
    run_list({whole(4, 8, 6), whole(4, 8, 4)});
    run_list({whole(4, 8, 6), whole(4, 8, 5)});      // (the same drive-count class: still two launches)
    run_list({whole(4, 8, 4), whole(4, 8, 4), whole(4, 8, 6)});
    run_list({whole(4, 8, 6), whole(4, 8, 4), whole(4, 8, 4)});
    run_list({whole(4, 8, 2), whole(4, 5, 2)});
    run_list({whole(4, 4, 2), whole(4, 5, 2), whole(4, 4, 2)});
    run_list({whole(4, 8, 2), whole(4, 8, 2, G_DENSE, S_KETS)});
    run_list({whole(4, 8, 2, G_DENSE, S_KETS), whole(4, 8, 2, G_DENSE, S_DENSITY)});
    run_list({whole(4, 8, 6), whole(4, 8, 6, G_NONANTI)});
    run_list({whole(4, 8, 6, G_NONANTI), whole(4, 8, 6), whole(4, 8, 6)});
    run_list({whole(4, 8, 6), whole(4, 8, 6, G_PERM)});
    run_list({whole(4, 8, 9), whole(4, 8, 9, G_NONANTI)});
    // a member of the LDS class, of the exponential integrator, of another order, of the 2N = 32 kernels
    run_list({whole(4, 8, 6), whole(4, 8, 6, G_DENSE, S_UNITARY, true, QC_KERNEL_LDS)});
    run_list({whole(4, 8, 6, G_DENSE, S_UNITARY, true, QC_KERNEL_LDS), whole(4, 8, 6), whole(4, 8, 6)});
    run_list({whole(4, 8, 6, G_DENSE, S_UNITARY, true, QC_KERNEL_LDS), whole(4, 8, 6, G_DENSE, S_UNITARY, true, QC_KERNEL_LDS)});
    run_list({whole(4, 8, 6), whole(0, 8, 6)});
    run_list({whole(0, 8, 6), whole(0, 8, 6)});
    run_list({whole(0, 2, 2), whole(0, 2, 2), whole(0, 2, 2)});
    run_list({whole(6, 8, 2), whole(6, 8, 2)});
    run_list({whole(4, 8, 2), whole(6, 8, 2)});
    run_list({whole(4, 16, 2), whole(4, 16, 2)});
    run_list({whole(4, 9, 2), whole(4, 9, 2)});
    // one member alone
    run_list({whole(4, 8, 6)});
    run_list({whole(4, 2, 2)});
    // ranges of intervals: equal shards share, another first interval or another length does not; knots of another width
    run_list({shard(whole(4, 8, 6), 3, 9), shard(whole(4, 8, 6), 3, 9)});
    run_list({shard(whole(4, 8, 6), 3, 9), shard(whole(4, 8, 6), 4, 10)});
    run_list({shard(whole(4, 8, 6), 3, 9), shard(whole(4, 8, 6), 3, 10), shard(whole(4, 8, 6), 3, 9)});
    run_list({whole(4, 8, 6), shard(whole(4, 8, 6), 0, 39)});
    run_list({whole(4, 2, 2), of_length(whole(4, 2, 2), 41)});
    run_list({whole(4, 8, 6), whole(4, 8, 6)}, 1);
    // lengths past the persistent grids of the batched launches (1024 and 4096 workgroups)
    for (int len : {1025, 4097}) run_list({of_length(whole(4, 8, 6), len), of_length(whole(4, 8, 6), len)});
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "full";
    if (mode == "full") sweep_full();
    else if (mode == "switches") sweep_switches();
    else if (mode == "lists") sweep_lists();
    else if (mode == "enumerators") {
        for (int k = 0; k < QC_JAC_KERNELS; ++k) printf("jac %s\n", qc_jac_kernel_id((QcJacKernel)k));
        for (int k = 0; k < QC_HESS_KERNELS; ++k) printf("hess %s\n", qc_hess_kernel_id((QcHessKernel)k));
        for (int k = 0; k < QC_FUSED_KERNELS; ++k) printf("fused %s\n", qc_fused_kernel_id((QcFusedKernel)k));
    } else { fprintf(stderr, "usage: %s full | switches | lists | enumerators\n", argv[0]); return 2; }
    for (const std::string& n : g_names) printf("name %s\n", n.c_str());
    return 0;
}
