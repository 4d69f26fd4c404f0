// Trajectory cost terms: the quadratic regularisers on a / da / dda and the minimum-time
// term, summed over all knots, with gradient and upper-triangular Hessian:
//     J(Z) = sum_t  1/2 sum_k R_k (sc_t (v_tk - b_tk))^2  +  D sum_{t < n_mt} dt_t,      sc_t = dt_t (or 1)
// (`QuadraticRegularizer(name, traj, R; baseline, timestep_name)`, reference call sites
// unitary_smooth_pulse_problem.jl:151-153; `MinimumTimeObjective(traj; D)`, unitary_minimum_time_problem.jl:67-69).
// The per-knot weighting by dt is how QuantumCollocationCore 0.3 is recalled to define the regulariser (its source
// is not vendored: SURVEY 8c); QC_REG_PLAIN drops it.
//
// One wavefront per knot: the lanes sweep the knot's zdim entries (coalesced 8-byte loads), write the whole
// gradient row (zeros where nothing is regularised, so the caller never memsets), reduce q_t = sum_k R_k dv^2 with
// DPP-free shuffles and lane 0 finishes the dt entries.  J is reduced in a fixed order (per-knot partials, then one
// workgroup), so repeated evaluations are bit-identical.  This is O(T zdim) bytes: latency-, not bandwidth-bound.
//
// Extension terms (qc_terms_create_ext, header comment of qc_terms_ext): the smoothness term couples neighbouring knots, so
// the wave of knot t also reads x_{t-1}[s_k] and x_{t+1}[s_k] (a forward difference enters J once, at the knot that owns its
// left end); the pairwise term reads the partners inside the knot through a per-entry adjacency list (gradient) and
// sweeps the pair list once (J and Hessian); the linear slack cost adds a constant.  The wave of knot t still writes its
// whole gradient row and nothing else, so no atomics.  A handle without extension terms launches qc_terms_kernel, the
// EXT = false instantiation: the regulariser pass above, with the same arguments.
#include <algorithm>
#include <string>
#include <vector>

#include "qc_side.h"

struct qc_terms : qc_side {
    qc_terms_desc d{};
    int n_reg = 0, cross = 0;
    int64_t hess_per_knot = 0;
    int* dslot = nullptr;          // zdim: index into the regulariser list or -1
    double* dR = nullptr;          // n_reg
    double* dbase = nullptr;       // n_reg x T or NULL
    double* dpart = nullptr;       // T partial sums
    double *dZ = nullptr, *dJ = nullptr, *dgrad = nullptr, *dhess = nullptr;   // staging for the host-pointer entry
    std::vector<int> index;
    // extension terms (has_ext = 0: none; the handle is then what qc_terms_create makes)
    int has_ext = 0, cross_p = 0;
    int64_t hs_base = 0, hp_base = 0, hp_knot = 0, hess_nnz = 0;
    std::vector<int> s_index, p_a, p_b, l_index;
    int* dxi = nullptr;            // [sslot zdim | lslot zdim | adj_ptr zdim+1 | adj_idx 2 n_pair | pair_a | pair_b]
    double* dxd = nullptr;         // [smooth_R | lin_w | adj_Q 2 n_pair | pair_Q]
};

namespace {

struct TermsParams {
    long long T;
    int zdim, off_dt, n_reg, plain, cross;
    long long global_dim, n_mt, hess_per_knot;
    double dt_fixed, D;
    const int* slot;
    const double* R;
    const double* base;
};

struct TermsExtParams {
    int n_smooth, n_pair, cross_p;
    long long hs_base, hp_base, hp_knot;   // value offsets of the smoothness and pairwise blocks, pairwise values per knot
    const int* sslot;                      // zdim: index into smooth_R or -1
    const double* sR;
    const int* lslot;                      // zdim: index into lin_w or -1
    const double* lw;
    const int* adj_ptr;                    // zdim + 1: entry j's partners are adj_idx[adj_ptr[j] .. adj_ptr[j+1])
    const int* adj_idx;
    const double* adj_Q;
    const int* pa;
    const int* pb;
    const double* pQ;
};

template <bool EXT>
__device__ __forceinline__ void terms_knot(const TermsParams& P, const TermsExtParams& X, const double* __restrict__ Z,
                                           double* __restrict__ part, double* __restrict__ grad, double* __restrict__ hess) {
    const int lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (grad && blockIdx.x == 0)
        for (long long i = threadIdx.x; i < P.global_dim; i += 256) grad[P.T * P.zdim + i] = 0.0;
    if (t >= P.T) return;
    const double* z = Z + t * P.zdim;
    const double dt = P.off_dt >= 0 ? z[P.off_dt] : P.dt_fixed;
    const double sc = P.plain ? 1.0 : dt;
    double q = 0.0, qp = 0.0, r = 0.0;     // qp: sum_p Q_p d_p^2; r: smoothness + linear part of J (EXT only)
    for (int j = lane; j < P.zdim; j += 64) {
        const int k = P.slot[j];
        double g = 0.0;
        if (k >= 0) {
            const double w = P.R[k];
            const double dv = z[j] - (P.base ? P.base[t * P.n_reg + k] : 0.0);
            g = w * sc * sc * dv;
            q = fma(w * dv, dv, q);
            if (hess) {
                double* hk = hess + t * P.hess_per_knot;
                hk[k] = w * sc * sc;
                if (P.cross) hk[P.n_reg + k] = 2.0 * dt * w * dv;
            }
        }
        if constexpr (EXT) {
            const double x = z[j];
            const int ks = X.sslot[j];
            if (ks >= 0) {
                const double w = X.sR[ks];
                const bool has_prev = t > 0, has_next = t + 1 < P.T;
                double gs = has_prev ? w * (x - z[j - P.zdim]) : 0.0;
                if (has_next) {
                    const double dn = z[j + P.zdim] - x;
                    gs -= w * dn;
                    r = fma(0.5 * w * dn, dn, r);
                }
                g += gs;
                if (hess) {
                    double* hs = hess + X.hs_base + t * 2 * X.n_smooth;
                    hs[ks] = w * (double)((int)has_prev + (int)has_next);
                    if (has_next) hs[X.n_smooth + ks] = -w;
                }
            }
            double gp = 0.0;
            for (int e = X.adj_ptr[j]; e < X.adj_ptr[j + 1]; ++e) gp = fma(X.adj_Q[e], x - z[X.adj_idx[e]], gp);
            g = fma(sc * sc, gp, g);
            const int kl = X.lslot[j];
            if (kl >= 0) {
                g += X.lw[kl];
                r = fma(X.lw[kl], x, r);
            }
        }
        if (grad && j != P.off_dt) grad[t * P.zdim + j] = g;
    }
    if constexpr (EXT) {
        for (int p = lane; p < X.n_pair; p += 64) {
            const double Q = X.pQ[p], d = z[X.pa[p]] - z[X.pb[p]];
            qp = fma(Q * d, d, qp);
            if (hess) {
                double* hp = hess + X.hp_base + t * X.hp_knot;
                const double v = Q * sc * sc;
                hp[p] = v;
                hp[X.n_pair + p] = v;
                hp[2 * X.n_pair + p] = -v;
                if (X.cross_p) {
                    hp[3 * X.n_pair + p] = 2.0 * dt * Q * d;
                    hp[4 * X.n_pair + p] = -2.0 * dt * Q * d;
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            qp += __shfl_xor(qp, off, 64);
            r += __shfl_xor(r, off, 64);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
    if (lane == 0) {
        const double mt = (P.off_dt >= 0 && t < P.n_mt) ? P.D : 0.0;
        if constexpr (EXT) {
            part[t] = 0.5 * sc * sc * (q + qp) + r + mt * dt;
            if (grad && P.off_dt >= 0) grad[t * P.zdim + P.off_dt] = (P.plain ? 0.0 : dt * (q + qp)) + mt;
            if (hess && X.cross_p) hess[X.hp_base + t * X.hp_knot + 5 * X.n_pair] = qp;
        } else {
            part[t] = 0.5 * sc * sc * q + mt * dt;
            if (grad && P.off_dt >= 0) grad[t * P.zdim + P.off_dt] = (P.plain ? 0.0 : dt * q) + mt;
        }
        if (hess && P.cross) hess[t * P.hess_per_knot + 2 * P.n_reg] = q;
    }
}

// the regulariser pass: the kernel of handles without extension terms (its arguments carry nothing of them)
__global__ __launch_bounds__(256) void qc_terms_kernel(TermsParams P, const double* __restrict__ Z, double* __restrict__ part,
                                                       double* __restrict__ grad, double* __restrict__ hess) {
    terms_knot<false>(P, TermsExtParams{}, Z, part, grad, hess);
}

__global__ __launch_bounds__(256) void qc_terms_ext_kernel(TermsParams P, TermsExtParams X, const double* __restrict__ Z,
                                                           double* __restrict__ part, double* __restrict__ grad, double* __restrict__ hess) {
    terms_knot<true>(P, X, Z, part, grad, hess);
}

// fixed-order sum of the per-knot partials: thread i adds part[i], part[i+256], ...; then a binary tree
__global__ __launch_bounds__(256) void qc_terms_sum_kernel(const double* __restrict__ part, long long T, double* __restrict__ J) {
    __shared__ double red[256];
    double acc = 0.0;
    for (long long i = threadIdx.x; i < T; i += 256) acc += part[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) J[0] = red[0];
}

thread_local std::string g_terr;
int tfail(qc_side* h, int code, const std::string& msg) { return qc_side_fail(h, &g_terr, code, msg); }

}  // namespace

extern "C" const char* qc_terms_last_error(const qc_terms* h) { return h ? h->err.c_str() : g_terr.c_str(); }

static int terms_validate(const qc_terms_desc* d, int* cross) {
    if (!d) return tfail(nullptr, QC_ERR_INVALID, "qc_terms: NULL descriptor");
    if (d->T < 1 || d->zdim < 1 || d->global_dim < 0) return tfail(nullptr, QC_ERR_INVALID, "qc_terms: bad T / zdim / global_dim");
    if (d->off_dt >= d->zdim) return tfail(nullptr, QC_ERR_INVALID, "qc_terms: off_dt outside the knot");
    if (d->n_reg < 0 || d->n_reg > d->zdim) return tfail(nullptr, QC_ERR_INVALID, "qc_terms: bad n_reg");
    if (d->n_reg > 0 && (!d->reg_index || !d->reg_R)) return tfail(nullptr, QC_ERR_INVALID, "qc_terms: NULL regulariser arrays");
    for (int k = 0; k < d->n_reg; ++k) {
        const int j = d->reg_index[k];
        if (j < 0 || j >= d->zdim || j == d->off_dt || (k > 0 && j <= d->reg_index[k - 1]))
            return tfail(nullptr, QC_ERR_INVALID, "qc_terms: reg_index must be strictly increasing, inside the knot and not the timestep");
    }
    if (d->weighting != QC_REG_DT_SCALED && d->weighting != QC_REG_PLAIN) return tfail(nullptr, QC_ERR_INVALID, "qc_terms: unknown weighting (QC_REG_DT_SCALED = 2, QC_REG_PLAIN = 3; the values 0 and 1 of ABI <= 0.3 are retired)");
    if (d->min_time_D != 0.0 && d->off_dt < 0) return tfail(nullptr, QC_ERR_INVALID, "qc_terms: a minimum-time term needs a free timestep");
    if (d->min_time_knots < 0 || d->min_time_knots > d->T) return tfail(nullptr, QC_ERR_INVALID, "qc_terms: min_time_knots out of range");
    *cross = (d->weighting == QC_REG_DT_SCALED && d->off_dt >= 0 && d->n_reg > 0) ? 1 : 0;
    return QC_OK;
}

extern "C" int qc_terms_desc_hess_nnz(const qc_terms_desc* d, int64_t* nnz) {
    int cross = 0;
    int rc = terms_validate(d, &cross);
    if (rc) return rc;
    if (!nnz) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_desc_hess_nnz: NULL output");
    *nnz = d->T * ((int64_t)d->n_reg * (1 + cross) + cross);
    return QC_OK;
}

extern "C" int qc_terms_desc_hess_structure(const qc_terms_desc* d, int64_t* rows, int64_t* cols, int one_based) {
    int cross = 0;
    int rc = terms_validate(d, &cross);
    if (rc) return rc;
    if (!rows || !cols) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_desc_hess_structure: NULL output");
    const int64_t b = one_based ? 1 : 0;
    int64_t e = 0;
    for (int64_t t = 0; t < d->T; ++t) {
        const int64_t c0 = t * d->zdim + b;
        for (int k = 0; k < d->n_reg; ++k, ++e) rows[e] = cols[e] = c0 + d->reg_index[k];
        if (!cross) continue;
        for (int k = 0; k < d->n_reg; ++k, ++e) {
            const int64_t a = c0 + d->reg_index[k], c = c0 + d->off_dt;
            rows[e] = a < c ? a : c;
            cols[e] = a < c ? c : a;
        }
        rows[e] = cols[e] = c0 + d->off_dt;
        ++e;
    }
    return QC_OK;
}

static bool ext_empty(const qc_terms_ext* x) { return !x || (x->n_smooth == 0 && x->n_pair == 0 && x->n_lin == 0); }

static int ext_validate(const qc_terms_desc* d, const qc_terms_ext* x, int* cross, int* cross_p) {
    int rc = terms_validate(d, cross);
    if (rc) return rc;
    *cross_p = 0;
    if (!x) return QC_OK;
    if (x->n_smooth < 0 || x->n_pair < 0 || x->n_lin < 0) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_ext: negative count");
    if ((x->n_smooth && (!x->smooth_index || !x->smooth_R)) || (x->n_pair && (!x->pair_a || !x->pair_b || !x->pair_Q)) ||
        (x->n_lin && (!x->lin_index || !x->lin_w)))
        return tfail(nullptr, QC_ERR_INVALID, "qc_terms_ext: NULL array behind a non-zero count");
    auto inside = [&](int j) { return j >= 0 && j < d->zdim && j != d->off_dt; };
    std::vector<char> seen(d->zdim, 0);
    for (int k = 0; k < x->n_smooth; ++k) {
        const int j = x->smooth_index[k];
        if (!inside(j)) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_ext: smooth_index outside the knot or the timestep");
        if (seen[j]) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_ext: repeated smooth_index");
        seen[j] = 1;
    }
    seen.assign(d->zdim, 0);
    for (int k = 0; k < x->n_lin; ++k) {
        const int j = x->lin_index[k];
        if (!inside(j)) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_ext: lin_index outside the knot or the timestep");
        if (seen[j]) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_ext: repeated lin_index");
        seen[j] = 1;
    }
    for (int p = 0; p < x->n_pair; ++p) {
        if (!inside(x->pair_a[p]) || !inside(x->pair_b[p]))
            return tfail(nullptr, QC_ERR_INVALID, "qc_terms_ext: pair index outside the knot or the timestep");
        if (x->pair_a[p] == x->pair_b[p]) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_ext: pair_a[p] == pair_b[p]");
    }
    *cross_p = (d->weighting == QC_REG_DT_SCALED && d->off_dt >= 0 && x->n_pair > 0) ? 1 : 0;
    return QC_OK;
}

// value counts of the three parts of the Hessian: per-knot prefix, smoothness block, pairwise values per knot
static void ext_counts(const qc_terms_desc* d, const qc_terms_ext* x, int cross, int cross_p, int64_t* prefix, int64_t* smooth, int64_t* hp_knot) {
    *prefix = d->T * ((int64_t)d->n_reg * (1 + cross) + cross);
    *smooth = x ? (int64_t)x->n_smooth * (2 * d->T - 1) : 0;
    *hp_knot = x ? 3 * (int64_t)x->n_pair + cross_p * (2 * (int64_t)x->n_pair + 1) : 0;
}

extern "C" int64_t qc_sizeof_terms_ext(void) { return (int64_t)sizeof(qc_terms_ext); }

extern "C" int qc_terms_desc_ext_hess_nnz(const qc_terms_desc* d, const qc_terms_ext* x, int64_t* nnz) {
    int cross = 0, cross_p = 0;
    int rc = ext_validate(d, x, &cross, &cross_p);
    if (rc) return rc;
    if (!nnz) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_desc_ext_hess_nnz: NULL output");
    int64_t a, b, c;
    ext_counts(d, x, cross, cross_p, &a, &b, &c);
    *nnz = a + b + d->T * c;
    return QC_OK;
}

extern "C" int qc_terms_desc_ext_hess_structure(const qc_terms_desc* d, const qc_terms_ext* x, int64_t* rows, int64_t* cols, int one_based) {
    int cross = 0, cross_p = 0;
    int rc = ext_validate(d, x, &cross, &cross_p);
    if (rc) return rc;
    if (!rows || !cols) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_desc_ext_hess_structure: NULL output");
    if ((rc = qc_terms_desc_hess_structure(d, rows, cols, one_based))) return rc;
    if (!x) return QC_OK;
    int64_t e, sm, hpk;
    ext_counts(d, x, cross, cross_p, &e, &sm, &hpk);
    const int64_t b = one_based ? 1 : 0;
    auto put = [&](int64_t r, int64_t c) {
        rows[e] = (r < c ? r : c) + b;
        cols[e] = (r < c ? c : r) + b;
        ++e;
    };
    for (int64_t t = 0; t < d->T; ++t) {
        const int64_t c0 = t * d->zdim;
        for (int k = 0; k < x->n_smooth; ++k) put(c0 + x->smooth_index[k], c0 + x->smooth_index[k]);
        if (t + 1 < d->T)
            for (int k = 0; k < x->n_smooth; ++k) put(c0 + x->smooth_index[k], c0 + d->zdim + x->smooth_index[k]);
    }
    for (int64_t t = 0; t < d->T; ++t) {
        const int64_t c0 = t * d->zdim;
        for (int p = 0; p < x->n_pair; ++p) put(c0 + x->pair_a[p], c0 + x->pair_a[p]);
        for (int p = 0; p < x->n_pair; ++p) put(c0 + x->pair_b[p], c0 + x->pair_b[p]);
        for (int p = 0; p < x->n_pair; ++p) put(c0 + x->pair_a[p], c0 + x->pair_b[p]);
        if (!cross_p) continue;
        for (int p = 0; p < x->n_pair; ++p) put(c0 + x->pair_a[p], c0 + d->off_dt);
        for (int p = 0; p < x->n_pair; ++p) put(c0 + x->pair_b[p], c0 + d->off_dt);
        put(c0 + d->off_dt, c0 + d->off_dt);
    }
    return QC_OK;
}

extern "C" int qc_terms_create(const qc_terms_desc* d, qc_terms** out) { return qc_terms_create_ext(d, nullptr, out); }

extern "C" int qc_terms_create_ext(const qc_terms_desc* d, const qc_terms_ext* x, qc_terms** out) {
    if (!out) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_create: out is NULL");
    *out = nullptr;
    int cross = 0, cross_p = 0;
    int rc = ext_validate(d, x, &cross, &cross_p);
    if (rc) return rc;
    if (ext_empty(x)) x = nullptr;
    if ((rc = qc_side_check_device(d->device, "qc_terms_create", &g_terr))) return rc;
    qc_side_new<qc_terms> h(new qc_terms());
    h->d = *d;
    h->n_reg = d->n_reg;
    h->device = d->device;
    h->cross = cross;
    h->hess_per_knot = (int64_t)d->n_reg * (1 + cross) + cross;
    {
        int64_t a, sm, hpk;
        ext_counts(d, x, cross, cross_p, &a, &sm, &hpk);
        h->hs_base = a;
        h->hp_base = a + sm;
        h->hp_knot = hpk;
        h->hess_nnz = a + sm + d->T * hpk;
    }
    h->index.assign(d->reg_index, d->reg_index + d->n_reg);
    // extension terms: per-entry slots and the pair adjacency, packed into one int and one double buffer
    std::vector<int> xi;
    std::vector<double> xd;
    if (x) {
        h->has_ext = 1;
        h->cross_p = cross_p;
        h->s_index.assign(x->smooth_index, x->smooth_index + x->n_smooth);
        h->l_index.assign(x->lin_index, x->lin_index + x->n_lin);
        h->p_a.assign(x->pair_a, x->pair_a + x->n_pair);
        h->p_b.assign(x->pair_b, x->pair_b + x->n_pair);
        const int zd = d->zdim, np = x->n_pair;
        xi.assign(3 * (size_t)zd + 1 + 4 * (size_t)np, -1);
        for (int k = 0; k < x->n_smooth; ++k) xi[x->smooth_index[k]] = k;
        for (int k = 0; k < x->n_lin; ++k) xi[zd + x->lin_index[k]] = k;
        int* ptr = xi.data() + 2 * zd;
        std::vector<int> deg(zd, 0);
        for (int p = 0; p < np; ++p) { ++deg[x->pair_a[p]]; ++deg[x->pair_b[p]]; }
        ptr[0] = 0;
        for (int j = 0; j < zd; ++j) ptr[j + 1] = ptr[j] + deg[j];
        xd.assign((size_t)x->n_smooth + x->n_lin + 3 * (size_t)np, 0.0);
        std::copy(x->smooth_R, x->smooth_R + x->n_smooth, xd.begin());
        std::copy(x->lin_w, x->lin_w + x->n_lin, xd.begin() + x->n_smooth);
        int* adj = ptr + zd + 1;
        double* adjQ = xd.data() + x->n_smooth + x->n_lin;
        std::vector<int> fill(ptr, ptr + zd);
        for (int p = 0; p < np; ++p) {    // entry j's partners in pair order
            const int a = x->pair_a[p], b = x->pair_b[p];
            adj[fill[a]] = b;
            adjQ[fill[a]++] = x->pair_Q[p];
            adj[fill[b]] = a;
            adjQ[fill[b]++] = x->pair_Q[p];
        }
        std::copy(x->pair_a, x->pair_a + np, adj + 2 * np);
        std::copy(x->pair_b, x->pair_b + np, adj + 3 * np);
        std::copy(x->pair_Q, x->pair_Q + np, adjQ + 2 * np);
    }
    h->d.reg_index = nullptr;   // caller-owned arrays are not retained
    h->d.reg_R = nullptr;
    h->d.reg_baseline = nullptr;
    std::vector<int> slot(d->zdim, -1);
    for (int k = 0; k < d->n_reg; ++k) slot[d->reg_index[k]] = k;
    const size_t Zlen = (size_t)d->T * d->zdim + (size_t)d->global_dim;
    qc_device_guard guard(d->device);
    QC_SIDE_HIP(nullptr, g_terr, guard.err);
    if (!xi.empty()) QC_SIDE_HIP(nullptr, g_terr, h->alloc(&h->dxi, xi.size(), xi.data()));
    if (!xd.empty()) QC_SIDE_HIP(nullptr, g_terr, h->alloc(&h->dxd, xd.size(), xd.data()));
    QC_SIDE_HIP(nullptr, g_terr, h->alloc(&h->dslot, slot.size(), slot.data()));
    if (d->n_reg > 0) {
        QC_SIDE_HIP(nullptr, g_terr, h->alloc(&h->dR, (size_t)d->n_reg, d->reg_R));
        if (d->reg_baseline) QC_SIDE_HIP(nullptr, g_terr, h->alloc(&h->dbase, (size_t)d->n_reg * d->T, d->reg_baseline));
    }
    QC_SIDE_HIP(nullptr, g_terr, h->alloc(&h->dpart, (size_t)d->T));
    QC_SIDE_HIP(nullptr, g_terr, h->alloc(&h->dZ, Zlen));
    QC_SIDE_HIP(nullptr, g_terr, h->alloc(&h->dJ, 1));
    QC_SIDE_HIP(nullptr, g_terr, h->alloc(&h->dgrad, Zlen));
    if (h->hess_nnz) QC_SIDE_HIP(nullptr, g_terr, h->alloc(&h->dhess, (size_t)h->hess_nnz));
    QC_SIDE_HIP(nullptr, g_terr, h->open_stream());
    *out = h.release();
    return QC_OK;
}

extern "C" void qc_terms_destroy(qc_terms* h) {
    if (!h) return;
    h->release_device();
    delete h;
}

extern "C" int qc_terms_hess_nnz(const qc_terms* h, int64_t* nnz) {
    if (!h || !nnz) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_hess_nnz: NULL argument");
    *nnz = h->hess_nnz;
    return QC_OK;
}

extern "C" int qc_terms_hess_structure(const qc_terms* h, int64_t* rows, int64_t* cols, int one_based) {
    if (!h) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_hess_structure: NULL handle");
    qc_terms_desc d = h->d;
    static const double dummy = 0.0;
    d.reg_index = h->index.data();
    d.reg_R = &dummy;
    if (!h->has_ext) return qc_terms_desc_hess_structure(&d, rows, cols, one_based);
    qc_terms_ext x{};
    x.n_smooth = (int32_t)h->s_index.size();
    x.n_pair = (int32_t)h->p_a.size();
    x.n_lin = (int32_t)h->l_index.size();
    x.smooth_index = h->s_index.data();
    x.pair_a = h->p_a.data();
    x.pair_b = h->p_b.data();
    x.lin_index = h->l_index.data();
    x.smooth_R = x.pair_Q = x.lin_w = &dummy;   // the structure reads no values
    return qc_terms_desc_ext_hess_structure(&d, &x, rows, cols, one_based);
}

extern "C" int qc_terms_eval_dev(qc_terms* h, const double* dZ, double* dJ, double* dgrad, double* dhvals, void* stream) {
    if (!h) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_eval_dev: NULL handle");
    if (!dZ || !dJ) return tfail(h, QC_ERR_INVALID, "qc_terms_eval_dev: NULL buffer");
    qc_device_guard guard(h->device);
    QC_SIDE_HIP(h, g_terr, guard.err);
    TermsParams P;
    P.T = h->d.T;
    P.zdim = h->d.zdim;
    P.off_dt = h->d.off_dt;
    P.n_reg = h->n_reg;
    P.plain = h->d.weighting == QC_REG_PLAIN;
    P.cross = h->cross;
    P.global_dim = h->d.global_dim;
    P.n_mt = h->d.min_time_knots;
    P.hess_per_knot = h->hess_per_knot;
    P.dt_fixed = h->d.dt_fixed;
    P.D = h->d.min_time_D;
    P.slot = h->dslot;
    P.R = h->dR;
    P.base = h->dbase;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)((h->d.T + 3) / 4);
    double* hv = h->hess_nnz ? dhvals : nullptr;
    if (h->has_ext) {
        TermsExtParams X{};
        const int zd = h->d.zdim, np = (int)h->p_a.size(), ns = (int)h->s_index.size(), nl = (int)h->l_index.size();
        X.n_smooth = ns;
        X.n_pair = np;
        X.cross_p = h->cross_p;
        X.hs_base = h->hs_base;
        X.hp_base = h->hp_base;
        X.hp_knot = h->hp_knot;
        X.sslot = h->dxi;
        X.lslot = h->dxi + zd;
        X.adj_ptr = h->dxi + 2 * zd;
        X.adj_idx = X.adj_ptr + zd + 1;
        X.pa = X.adj_idx + 2 * np;
        X.pb = X.adj_idx + 3 * np;
        X.sR = h->dxd;
        X.lw = h->dxd + ns;
        X.adj_Q = h->dxd + ns + nl;
        X.pQ = X.adj_Q + 2 * np;
        hipLaunchKernelGGL(qc_terms_ext_kernel, dim3(grid), dim3(256), 0, s, P, X, dZ, h->dpart, dgrad, hv);
    } else {
        hipLaunchKernelGGL(qc_terms_kernel, dim3(grid), dim3(256), 0, s, P, dZ, h->dpart, dgrad, hv);
    }
    hipLaunchKernelGGL(qc_terms_sum_kernel, dim3(1), dim3(256), 0, s, h->dpart, (long long)h->d.T, dJ);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return tfail(h, QC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return QC_OK;
}

extern "C" int qc_terms_eval(qc_terms* h, const double* Z, double* J, double* grad, double* hvals) {
    if (!h) return tfail(nullptr, QC_ERR_INVALID, "qc_terms_eval: NULL handle");
    if (!Z) return tfail(h, QC_ERR_INVALID, "qc_terms_eval: NULL input");
    const size_t Zlen = (size_t)h->d.T * h->d.zdim + (size_t)h->d.global_dim;
    const size_t nh = (size_t)h->hess_nnz;
    qc_device_guard guard(h->device);
    QC_SIDE_HIP(h, g_terr, guard.err);
    QC_SIDE_HIP(h, g_terr, hipMemcpyAsync(h->dZ, Z, Zlen * 8, hipMemcpyHostToDevice, h->stream));
    int rc = qc_terms_eval_dev(h, h->dZ, h->dJ, grad ? h->dgrad : nullptr, hvals ? h->dhess : nullptr, h->stream);
    if (rc) return rc;
    double j = 0.0;
    QC_SIDE_HIP(h, g_terr, hipMemcpyAsync(&j, h->dJ, 8, hipMemcpyDeviceToHost, h->stream));
    if (grad) QC_SIDE_HIP(h, g_terr, hipMemcpyAsync(grad, h->dgrad, Zlen * 8, hipMemcpyDeviceToHost, h->stream));
    if (hvals && nh) QC_SIDE_HIP(h, g_terr, hipMemcpyAsync(hvals, h->dhess, nh * 8, hipMemcpyDeviceToHost, h->stream));
    QC_SIDE_HIP(h, g_terr, hipStreamSynchronize(h->stream));
    if (J) *J = j;
    return QC_OK;
}
