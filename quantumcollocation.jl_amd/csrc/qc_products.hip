// Matrix-free Jacobian products of the dynamics: y = dF(Z) v and w = dF(Z)' lam (qc_eval_jvp_dev / qc_eval_vjp_dev and their
// host-buffer and list forms' device half).  This file holds the GENERIC path and the entry points' shared front end; the fused
// forward kernel of the order-4 Pade integrator at 2N <= 16 is in qc_mfma_products.hip, and qc_plan decides between the two.
//
// Generic path, every handle kind: the per-interval Jacobian pattern is the same for every interval and comes from the library's
// own generator (qc_local_jac_structure), so whatever F + dF kernel serves the handle -- any integrator, Pade order, size, state
// kind, row layout or block order, MFMA class or LDS class -- a product is two launches:
//   1. the handle's own dF launch into a scratch value array the handle owns (no residual store), in whatever form it writes;
//   2. a product kernel over that scratch, driven by two device tables built at the first call:
//        forward     the pattern sorted by row: one workgroup per interval, each thread owns rows;
//        transposed  the pattern sorted by column, the columns of knot t and of knot t+1 kept apart: one workgroup per knot,
//                    each thread owns entries of the knot; an entry's sum runs over the value block of interval t-1 (its knot-t+1
//                    columns) and then over that of interval t (its knot-t columns).
// Every output entry has one writer and a fixed summation order: no atomics, nothing depends on scheduling, repeated calls give
// the same bits.  The transposed kernel writes EVERY entry of w (knots the handle's intervals do not touch and the global_dim tail
// get 0.0) unless it accumulates (the later members of an integrator list).
//
// The Hessian product w = H(Z, mu) v (qc_eval_hvp_dev and its host-buffer and list forms' device half), H the full symmetric matrix whose
// upper triangle qc_hess_structure describes, follows the transposed Jacobian product: the handle's own mu_d2F launch into a scratch of
// n_int x H_stride doubles, then a product kernel, one workgroup per knot and one thread per knot entry, driven by a table built from
// qc_local_hess_structure: every structural entry (i, j) of the upper triangle is listed under target i with source j and, unless
// i == j, under target j with source i; the lists are sorted by (target, source) -- by coordinates, never by where a value lies in the
// interval's block -- and the targets at knot t of an interval (its right-hand neighbour) are kept apart from those at knot t+1 (its
// left-hand neighbour).  An entry of w sums over the block of interval t-1, then over that of interval t.  The alignment padding of a
// block (explicit zeros recorded as duplicates of the block's first entry) is not in the table at all.
#include <string.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "qc_internal.h"
#include "qc_plan.h"

#define fail qc_fail

namespace {

// Device tables (int32), one allocation: a header of offsets, then the arrays.
//   forward:     frow[nr] local row of output k | fptr[nr + 1] | fent[nnz] value index | fcol[nnz] local column (>= zdim: knot t+1)
//   transposed:  for side 0 (columns of knot t) and side 1 (columns of knot t+1):  tptr[zdim + 1] | tent[...] | trow[...]
struct QcProductTables {
    int nr, nnz;
    int frow, fptr, fent, fcol;        // offsets (ints) from the start of the allocation
    int tptr[2], tent[2], trow[2];
};

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void qc_jvp_generic_kernel(const int32_t* __restrict__ tab, int n_int, long long t_begin, int zdim,
                                                                 long long F_stride, long long F_off, long long J_stride, long long J_off,
                                                                 const double* __restrict__ vals, const double* __restrict__ v,
                                                                 double* __restrict__ y) {
    const QcProductTables& H = *reinterpret_cast<const QcProductTables*>(tab);
    const int32_t* frow = tab + H.frow;
    const int32_t* fptr = tab + H.fptr;
    const int32_t* fent = tab + H.fent;
    const int32_t* fcol = tab + H.fcol;
    for (int b = blockIdx.x; b < n_int; b += gridDim.x) {
        const double* Jb = vals + (size_t)b * J_stride + J_off;
        const double* vb = v + (size_t)(t_begin + b) * zdim;        // local column c >= zdim is entry c - zdim of knot t+1: contiguous
        double* yb = y + (size_t)b * F_stride + F_off;
        for (int k = threadIdx.x; k < H.nr; k += kThreads) {
            double acc = 0.0;
            for (int i = fptr[k]; i < fptr[k + 1]; ++i) acc += Jb[fent[i]] * vb[fcol[i]];
            yb[frow[k]] = acc;
        }
    }
}

// grid: one workgroup per knot, then the workgroups of the global_dim tail
__global__ __launch_bounds__(kThreads) void qc_vjp_generic_kernel(const int32_t* __restrict__ tab, int n_int, long long t_begin, long long T,
                                                                 long long global_dim, int zdim, long long F_stride, long long F_off,
                                                                 long long J_stride, long long J_off, const double* __restrict__ vals,
                                                                 const double* __restrict__ lam, double* __restrict__ w, int accumulate) {
    const long long t = blockIdx.x;
    if (t >= T) {      // variables after the knots: no interval reads them
        const long long i = (t - T) * kThreads + threadIdx.x;
        if (i < global_dim && !accumulate) w[T * zdim + i] = 0.0;
        return;
    }
    const QcProductTables& H = *reinterpret_cast<const QcProductTables*>(tab);
    const long long bl = t - 1 - t_begin, br = t - t_begin;      // the interval to the left (this knot is its t+1) and to the right
    const bool left = bl >= 0 && bl < n_int, right = br >= 0 && br < n_int;
    double* wt = w + t * zdim;
    for (int c = threadIdx.x; c < zdim; c += kThreads) {
        double acc = 0.0;
        if (left) {
            const int32_t *ptr = tab + H.tptr[1], *ent = tab + H.tent[1], *row = tab + H.trow[1];
            const double* Jb = vals + (size_t)bl * J_stride + J_off;
            const double* lb = lam + (size_t)bl * F_stride + F_off;
            for (int i = ptr[c]; i < ptr[c + 1]; ++i) acc += Jb[ent[i]] * lb[row[i]];
        }
        if (right) {
            const int32_t *ptr = tab + H.tptr[0], *ent = tab + H.tent[0], *row = tab + H.trow[0];
            const double* Jb = vals + (size_t)br * J_stride + J_off;
            const double* lb = lam + (size_t)br * F_stride + F_off;
            for (int i = ptr[c]; i < ptr[c + 1]; ++i) acc += Jb[ent[i]] * lb[row[i]];
        }
        wt[c] = accumulate ? wt[c] + acc : acc;
    }
}

// Hessian product tables (int32), one allocation: the header, then for side 0 (targets at knot t of an interval) and side 1 (targets at
// knot t+1):  ptr[zdim + 1] | ent[...] value index in the interval's block | src[...] local source variable (>= zdim: knot t+1)
struct QcHessProductTables {
    int ptr[2], ent[2], src[2];        // offsets (ints) from the start of the allocation
};

// grid: one workgroup per knot, then the workgroups of the global_dim tail
__global__ __launch_bounds__(kThreads) void qc_hvp_generic_kernel(const int32_t* __restrict__ tab, int n_int, long long t_begin, long long T,
                                                                 long long global_dim, int zdim, long long H_stride, long long H_off,
                                                                 const double* __restrict__ vals, const double* __restrict__ v,
                                                                 double* __restrict__ w, int accumulate) {
    const long long t = blockIdx.x;
    if (t >= T) {      // variables after the knots: no Hessian entry touches them
        const long long i = (t - T) * kThreads + threadIdx.x;
        if (i < global_dim && !accumulate) w[T * zdim + i] = 0.0;
        return;
    }
    const QcHessProductTables& H = *reinterpret_cast<const QcHessProductTables*>(tab);
    const long long bl = t - 1 - t_begin, br = t - t_begin;      // the interval to the left (this knot is its t+1) and to the right
    const bool left = bl >= 0 && bl < n_int, right = br >= 0 && br < n_int;
    double* wt = w + t * zdim;
    for (int c = threadIdx.x; c < zdim; c += kThreads) {
        double acc = 0.0;
        if (left) {
            const int32_t *ptr = tab + H.ptr[1], *ent = tab + H.ent[1], *src = tab + H.src[1];
            const double* Hb = vals + (size_t)bl * H_stride + H_off;
            const double* vb = v + (t - 1) * zdim;      // local source j >= zdim is entry j - zdim of knot t: contiguous
            for (int i = ptr[c]; i < ptr[c + 1]; ++i) acc += Hb[ent[i]] * vb[src[i]];
        }
        if (right) {
            const int32_t *ptr = tab + H.ptr[0], *ent = tab + H.ent[0], *src = tab + H.src[0];
            const double* Hb = vals + (size_t)br * H_stride + H_off;
            const double* vb = v + t * zdim;
            for (int i = ptr[c]; i < ptr[c + 1]; ++i) acc += Hb[ent[i]] * vb[src[i]];
        }
        wt[c] = accumulate ? wt[c] + acc : acc;
    }
}

// The tables of a handle, on the host: the pattern sorted by (row, column), and by (column, row) on either side -- never by where a
// value lies in the interval's block, so qc_desc.jac_block_order cannot change a sum's order (entries are unique).
std::vector<int32_t> build_tables(const QcParams& P) {
    std::vector<int32_t> lr, lc;
    qc_local_jac_structure(P, &lr, &lc);
    const int nnz = (int)lr.size(), zd = P.zdim;
    std::vector<int> by_row(nnz);
    std::iota(by_row.begin(), by_row.end(), 0);
    std::sort(by_row.begin(), by_row.end(), [&](int a, int b) { return lr[a] != lr[b] ? lr[a] < lr[b] : lc[a] < lc[b]; });
    std::vector<int32_t> frow, fptr, fent, fcol;
    for (int i = 0; i < nnz; ++i) {
        const int e = by_row[i];
        if (i == 0 || lr[e] != lr[by_row[i - 1]]) { frow.push_back(lr[e]); fptr.push_back(i); }
        fent.push_back(e);
        fcol.push_back(lc[e]);
    }
    fptr.push_back(nnz);
    std::vector<int32_t> tptr[2], tent[2], trow[2];
    for (int side = 0; side < 2; ++side) {
        tptr[side].assign(zd + 1, 0);
        for (int e = 0; e < nnz; ++e)
            if ((lc[e] >= zd) == (side == 1)) ++tptr[side][lc[e] - side * zd + 1];
        for (int c = 0; c < zd; ++c) tptr[side][c + 1] += tptr[side][c];
        tent[side].resize(tptr[side][zd]);
        trow[side].resize(tptr[side][zd]);
        std::vector<int32_t> fill(tptr[side].begin(), tptr[side].end() - 1);
        for (int i = 0; i < nnz; ++i) {      // (in row order)
            const int e = by_row[i];
            if ((lc[e] >= zd) == (side == 1)) {
                const int at = fill[lc[e] - side * zd]++;
                tent[side][at] = e;
                trow[side][at] = lr[e];
            }
        }
    }
    static_assert(sizeof(QcProductTables) % sizeof(int32_t) == 0, "the header is a whole number of ints");
    QcProductTables H;
    H.nr = (int)frow.size();
    H.nnz = nnz;
    std::vector<int32_t> blob(sizeof(QcProductTables) / sizeof(int32_t));
    auto append = [&](const std::vector<int32_t>& a) { const int at = (int)blob.size(); blob.insert(blob.end(), a.begin(), a.end()); return at; };
    H.frow = append(frow); H.fptr = append(fptr); H.fent = append(fent); H.fcol = append(fcol);
    for (int side = 0; side < 2; ++side) { H.tptr[side] = append(tptr[side]); H.tent[side] = append(tent[side]); H.trow[side] = append(trow[side]); }
    memcpy(blob.data(), &H, sizeof(H));
    return blob;
}

// first product call of a handle on the generic path: the tables and the scratch values
int prepare_generic(qc_handle* h) {
    if (h->dPtab) return QC_OK;
    const std::vector<int32_t> blob = build_tables(h->prm);
    const size_t nvals = (size_t)h->prm.n_int * (size_t)h->prm.J_stride;
    if (nvals && !h->dPvals) QC_HIP(h, hipMalloc((void**)&h->dPvals, nvals * sizeof(double)));
    int32_t* tab = nullptr;
    QC_HIP(h, hipMalloc((void**)&tab, blob.size() * sizeof(int32_t)));
    const hipError_t e = hipMemcpy(tab, blob.data(), blob.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(tab); QC_HIP(h, e); }
    h->dPtab = tab;
    return QC_OK;
}

// The Hessian product's table, on the host.  Only the hess_nnz structural entries take part: the h_pad padding entries behind them are
// zero duplicates of the first entry, which would otherwise count a diagonal first entry once per padding word.
std::vector<int32_t> build_hess_tables(const QcParams& P) {
    std::vector<int32_t> lr, lc;
    qc_local_hess_structure(P, &lr, &lc);
    const int zd = P.zdim;
    struct Term { int32_t target, src, ent; };
    std::vector<Term> terms;
    for (int e = 0; e < P.hess_nnz; ++e) {
        terms.push_back({lr[e], lc[e], e});
        if (lr[e] != lc[e]) terms.push_back({lc[e], lr[e], e});
    }
    std::sort(terms.begin(), terms.end(), [](const Term& a, const Term& b) {
        return a.target != b.target ? a.target < b.target : (a.src != b.src ? a.src < b.src : a.ent < b.ent);
    });
    std::vector<int32_t> ptr[2], ent[2], src[2];
    for (int side = 0; side < 2; ++side) {
        ptr[side].assign(zd + 1, 0);
        for (const Term& x : terms)
            if ((x.target >= zd) == (side == 1)) {
                ++ptr[side][x.target - side * zd + 1];
                ent[side].push_back(x.ent);      // (terms are in target order: the lists come out grouped by target)
                src[side].push_back(x.src);
            }
        for (int c = 0; c < zd; ++c) ptr[side][c + 1] += ptr[side][c];
    }
    static_assert(sizeof(QcHessProductTables) % sizeof(int32_t) == 0, "the header is a whole number of ints");
    QcHessProductTables H;
    std::vector<int32_t> blob(sizeof(QcHessProductTables) / sizeof(int32_t));
    auto append = [&](const std::vector<int32_t>& a) { const int at = (int)blob.size(); blob.insert(blob.end(), a.begin(), a.end()); return at; };
    for (int side = 0; side < 2; ++side) { H.ptr[side] = append(ptr[side]); H.ent[side] = append(ent[side]); H.src[side] = append(src[side]); }
    memcpy(blob.data(), &H, sizeof(H));
    return blob;
}

// first Hessian product call of a handle: the table and the scratch values
int prepare_hess_generic(qc_handle* h) {
    if (h->dHPtab) return QC_OK;
    const std::vector<int32_t> blob = build_hess_tables(h->prm);
    const size_t nvals = (size_t)h->prm.n_int * (size_t)h->prm.H_stride;
    if (nvals && !h->dHPvals) QC_HIP(h, hipMalloc((void**)&h->dHPvals, nvals * sizeof(double)));
    int32_t* tab = nullptr;
    QC_HIP(h, hipMalloc((void**)&tab, blob.size() * sizeof(int32_t)));
    const hipError_t e = hipMemcpy(tab, blob.data(), blob.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(tab); QC_HIP(h, e); }
    h->dHPtab = tab;
    return QC_OK;
}

int check_args(qc_handle* h, const char* who, const void* a, const void* b, const void* c) {
    if (!h->shards.empty())
        return fail(&h->err, QC_ERR_UNSUPPORTED, std::string(who) + ": the Jacobian products do not serve multi-device handles (qc_create_multi); "
                                                 "use the shard handles (qc_multi_shard) on their own devices");
    if (!a || !b || !c) return fail(&h->err, QC_ERR_INVALID, std::string(who) + ": NULL buffer");
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 8) return fail(&h->err, QC_ERR_INVALID, std::string(who) + ": a buffer is not 8-byte aligned");
    return QC_OK;
}

}  // namespace

int qc_product_jvp_dev(qc_handle* h, const char* who, const double* dZ, const double* dv, double* dy, hipStream_t st) {
    int rc;
    if ((rc = check_args(h, who, dZ, dv, dy))) return rc;
    const QcParams& P = h->prm;
    if (P.n_int == 0) return QC_OK;
    qc_device_guard guard(h->device);
    QC_HIP(h, guard.err);
    if (h->plan.jvp == QC_PROD_PADE4_16) {
        const hipError_t e = qc_launch_mfma16_jvp(P, dZ, dv, dy, st);
        if (e != hipSuccess) return fail(&h->err, QC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
        return QC_OK;
    }
    if ((rc = prepare_generic(h))) return rc;
    if ((rc = qc_eval_F_jac_dev(h, dZ, nullptr, h->dPvals, (void*)st))) return rc;
    const int grid = std::min(P.n_int, 1 << 20);
    hipLaunchKernelGGL(qc_jvp_generic_kernel, dim3(grid), dim3(kThreads), 0, st, h->dPtab, P.n_int, P.t_begin, P.zdim, P.F_stride, P.F_off, P.J_stride,
                       P.J_off, h->dPvals, dv, dy);
    QC_HIP(h, hipGetLastError());
    return QC_OK;
}

int qc_product_vjp_dev(qc_handle* h, const char* who, const double* dZ, const double* dlam, double* dw, bool accumulate, hipStream_t st) {
    int rc;
    if ((rc = check_args(h, who, dZ, dlam, dw))) return rc;
    const QcParams& P = h->prm;
    const long long T = h->desc.T, gd = h->desc.global_dim;
    qc_device_guard guard(h->device);
    QC_HIP(h, guard.err);
    if ((rc = prepare_generic(h))) return rc;
    if (P.n_int > 0 && (rc = qc_eval_F_jac_dev(h, dZ, nullptr, h->dPvals, (void*)st))) return rc;
    const long long grid = T + (gd + kThreads - 1) / kThreads;
    if (grid > 0x7fffffffLL) return fail(&h->err, QC_ERR_UNSUPPORTED, std::string(who) + ": too many knots for one launch");
    hipLaunchKernelGGL(qc_vjp_generic_kernel, dim3((unsigned)grid), dim3(kThreads), 0, st, h->dPtab, P.n_int, P.t_begin, T, gd, P.zdim, P.F_stride, P.F_off,
                       P.J_stride, P.J_off, h->dPvals, dlam, dw, accumulate ? 1 : 0);
    QC_HIP(h, hipGetLastError());
    return QC_OK;
}

int qc_product_hvp_dev(qc_handle* h, const char* who, const double* dZ, const double* dmu, const double* dv, double* dw, bool accumulate,
                       hipStream_t st) {
    if (!h->shards.empty())
        return fail(&h->err, QC_ERR_UNSUPPORTED, std::string(who) + ": the Hessian product does not serve multi-device handles (qc_create_multi); "
                                                 "use the shard handles (qc_multi_shard) on their own devices");
    if (h->prm.hess_nnz == 0)
        return fail(&h->err, QC_ERR_UNSUPPORTED, std::string(who) + ": this handle has no analytic Hessian (hess_nnz = 0)");
    if (!dZ || !dmu || !dv || !dw) return fail(&h->err, QC_ERR_INVALID, std::string(who) + ": NULL buffer");
    if (((uintptr_t)dZ | (uintptr_t)dmu | (uintptr_t)dv | (uintptr_t)dw) % 8) return fail(&h->err, QC_ERR_INVALID, std::string(who) + ": a buffer is not 8-byte aligned");
    const QcParams& P = h->prm;
    const long long T = h->desc.T, gd = h->desc.global_dim;
    qc_device_guard guard(h->device);
    QC_HIP(h, guard.err);
    int rc;
    if ((rc = prepare_hess_generic(h))) return rc;
    // the handle's slice of a value vector starts at its first interval: the scratch is the slice itself
    if (P.n_int > 0 && (rc = qc_eval_hess_dev(h, dZ, dmu, h->dHPvals, (void*)st))) return rc;
    const long long grid = T + (gd + kThreads - 1) / kThreads;
    if (grid > 0x7fffffffLL) return fail(&h->err, QC_ERR_UNSUPPORTED, std::string(who) + ": too many knots for one launch");
    hipLaunchKernelGGL(qc_hvp_generic_kernel, dim3((unsigned)grid), dim3(kThreads), 0, st, h->dHPtab, P.n_int, P.t_begin, T, gd, P.zdim, P.H_stride, P.H_off,
                       h->dHPvals, dv, dw, accumulate ? 1 : 0);
    QC_HIP(h, hipGetLastError());
    return QC_OK;
}

extern "C" int qc_eval_jvp_dev(qc_handle* h, const double* dZ, const double* dv, double* dy, void* stream) {
    if (!h) return fail(nullptr, QC_ERR_INVALID, "qc_eval_jvp_dev: NULL handle");
    return qc_product_jvp_dev(h, "qc_eval_jvp_dev", dZ, dv, dy, (hipStream_t)stream);
}

extern "C" int qc_eval_vjp_dev(qc_handle* h, const double* dZ, const double* dlam, double* dw, void* stream) {
    if (!h) return fail(nullptr, QC_ERR_INVALID, "qc_eval_vjp_dev: NULL handle");
    return qc_product_vjp_dev(h, "qc_eval_vjp_dev", dZ, dlam, dw, false, (hipStream_t)stream);
}

extern "C" int qc_eval_hvp_dev(qc_handle* h, const double* dZ, const double* dmu, const double* dv, double* dw, void* stream) {
    if (!h) return fail(nullptr, QC_ERR_INVALID, "qc_eval_hvp_dev: NULL handle");
    return qc_product_hvp_dev(h, "qc_eval_hvp_dev", dZ, dmu, dv, dw, false, (hipStream_t)stream);
}

// Integrator lists on one device: the members run in member order on the stream.  y: every member writes its own rows of the
// problem's row vector.  w: the first member overwrites (every entry), the others add -- a fixed order, so the sum is reproducible.
static int list_front(qc_handle* const* hs, int32_t count, const char* who, const char* what = "the Jacobian products do") {
    if (!hs || count < 1) return fail(nullptr, QC_ERR_INVALID, std::string(who) + ": no handles");
    for (int i = 0; i < count; ++i) if (!hs[i]) return fail(nullptr, QC_ERR_INVALID, std::string(who) + ": NULL handle");
    for (int i = 0; i < count; ++i) {
        if (!hs[i]->shards.empty())
            return fail(&hs[0]->err, QC_ERR_UNSUPPORTED, std::string(who) + ": " + what + " not serve multi-device handles (qc_create_multi)");
        if (hs[i]->device != hs[0]->device) return fail(&hs[0]->err, QC_ERR_INVALID, std::string(who) + ": the handles are bound to different devices");
        if (hs[i]->dims.Z_len != hs[0]->dims.Z_len) return fail(&hs[0]->err, QC_ERR_INVALID, std::string(who) + ": the handles are not over one trajectory");
    }
    return QC_OK;
}

extern "C" int qc_eval_jvp_dev_multi(qc_handle* const* hs, int32_t count, const double* dZ, const double* dv, double* dy, void* stream) {
    int rc;
    if ((rc = list_front(hs, count, "qc_eval_jvp_dev_multi"))) return rc;
    for (int i = 0; i < count; ++i)
        if ((rc = qc_product_jvp_dev(hs[i], "qc_eval_jvp_dev_multi", dZ, dv, dy, (hipStream_t)stream))) {
            if (i) hs[0]->err = hs[i]->err;      // (errors of a list are read from its first handle)
            return rc;
        }
    return QC_OK;
}

extern "C" int qc_eval_vjp_dev_multi(qc_handle* const* hs, int32_t count, const double* dZ, const double* dlam, double* dw, void* stream) {
    int rc;
    if ((rc = list_front(hs, count, "qc_eval_vjp_dev_multi"))) return rc;
    for (int i = 0; i < count; ++i)
        if ((rc = qc_product_vjp_dev(hs[i], "qc_eval_vjp_dev_multi", dZ, dlam, dw, i > 0, (hipStream_t)stream))) {
            if (i) hs[0]->err = hs[i]->err;
            return rc;
        }
    return QC_OK;
}

extern "C" int qc_eval_hvp_dev_multi(qc_handle* const* hs, int32_t count, const double* dZ, const double* dmu, const double* dv, double* dw,
                                     void* stream) {
    int rc;
    if ((rc = list_front(hs, count, "qc_eval_hvp_dev_multi", "the Hessian product does"))) return rc;
    for (int i = 0; i < count; ++i)      // refused before any member has written: a list with a member without a Hessian leaves w alone
        if (hs[i]->prm.hess_nnz == 0) return fail(&hs[0]->err, QC_ERR_UNSUPPORTED, "qc_eval_hvp_dev_multi: a member has no analytic Hessian (hess_nnz = 0)");
    for (int i = 0; i < count; ++i)
        if ((rc = qc_product_hvp_dev(hs[i], "qc_eval_hvp_dev_multi", dZ, dmu, dv, dw, i > 0, (hipStream_t)stream))) {
            if (i) hs[0]->err = hs[i]->err;
            return rc;
        }
    return QC_OK;
}
