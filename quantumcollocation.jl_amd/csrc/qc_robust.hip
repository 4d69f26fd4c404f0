// UnitaryRobustnessObjective (reference unitary_robustness_problem.jl:46-49): a whole-trajectory term that reads the unitary
// of every knot, reduces over the knots and gives every knot a gradient block; its exact Hessian couples every knot with
// every other.
//
// Notation: U_t the N x N operator of knot t (iso-vec layout, operator_to_iso_vec); S = (s_0 .. s_{n-1}) the subspace levels;
// V_t = U_t[S, S] (Re U[s_a, s_b] at s_b 2N + s_a, Im at s_b 2N + N + s_a); H the n x n error operator (complex, need not
// be Hermitian); dt_t the knot's timestep (or the fixed one); K the number of knots in the sum.
//
//     A_t = V_t' H V_t        tau = sum_{t<K} dt_t        R = (1/tau) sum_{t<K} dt_t A_t        L = Re tr(R'R) / n
//
//     dL/dV_t  = G_t = (2 dt_t / (n tau)) (H V_t R' + H' V_t R)          (complex gradient -> iso slots [Re G; Im G])
//     dL/ddt_t = (2 / (n tau)) Re tr(R' (A_t - R))                         (free timestep only)
//
// Hessian, with <X, Y> = Re tr(X'Y):  d2L/dxdy = (2/n) [<d_x R, d_y R> + <R, d2_xy R>].  For an entry x of knot t with unit
// (or i * unit) direction D_x and E_x = D_x' H V_t + V_t' H D_x:
//     d_x R = dt_t E_x / tau                    d_{dt_t} R = (A_t - R) / tau
//     d2 R (x, y in knot t)   = dt_t (D_x' H D_y + D_y' H D_x) / tau        (0 across knots)
//     d2 R (x in t, dt_s)     = (delta_ts - dt_t / tau) E_x / tau
//     d2 R (dt_t, dt_s)       = -(A_s - R) / tau^2 - (A_t - R) / tau^2
// so the Hessian is a Gram matrix of the rows r_x = d_x R (2n^2 reals each) -- a SYRK of inner dimension 2n^2 -- plus a
// same-knot block correction and rank-structured dt rows, all added in the SYRK's epilogue:
//     C(x, y same knot) = (dt_t / tau) <R, D_x' H D_y + D_y' H D_x>
//     C(x in t, dt_s)   = (delta_ts - dt_t / tau) e_x,       e_x = <R, E_x> / tau
//     C(dt_t, dt_s)     = -(q_t + q_s) / tau,                q_t = <R, A_t - R> / tau
// The gradient is (2/n) dt_t e_x and (2/n) q_t.
//
// Launches (all on the caller's stream, no host synchronisation):
//   1. qc_robust_partial_kernel: per group of kp knots, H V_t and V_t' H V_t in LDS; every workgroup accumulates dt_t A_t and
//      dt_t over its own knot groups (one LDS slot per thread, always the same thread) and writes one partial row.
//   2. qc_robust_reduce_kernel: one workgroup sums the partial rows in workgroup order: S, tau, R = S / tau, L.
//   3. qc_robust_grad_kernel: per group of kp knots, the gradient written dense over Z_len (zeros included, global entries
//      too); with the Hessian requested also the rows r_x, the scalars e_x / q_t and dt_t / tau.
//   4. qc_robust_syrk_kernel (Hessian only): one wave per 16 x 16 tile of the upper triangle on v_mfma_f64_16x16x4_f64,
//      epilogue adds the corrections, stores the column-major packed triangle (entry (i <= j) at j(j+1)/2 + i).
// Every sum runs in an order fixed by the descriptor alone (no atomics): repeated evaluations are bit-identical.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "qc_side.h"

namespace {

constexpr int kRobThreads = 256;
constexpr int kRobMaxParts = 256;            // workgroups of the partial-sum launch (rows the reducer sums)
constexpr int64_t kRobHessCap = int64_t(1) << 27;

typedef double v4d __attribute__((ext_vector_type(4)));

struct RobParams {
    long long T, K, global_dim, ngroups;
    int zdim, off_state, N, n, off_dt, kp, P, m2p, nparts;
    double dt_fixed;
    const int* sub;       // n levels
    const double* H;      // n x n, column-major, real plane then imaginary plane
    const int* slot;      // zdim: local variable index or -1
    const int* var;       // P x 4: kind (0 state, 1 dt), a, b, part (0 re, 1 im)
};

// V (n x n complex, planar, column-major) of knot t from its iso-vec
__device__ inline void load_v(const RobParams& P, const double* __restrict__ Z, long long t, int e, double* __restrict__ sV) {
    const int nn = P.n * P.n, i = e % P.n, j = e / P.n;
    const double* u = Z + t * P.zdim + P.off_state + (long long)P.sub[j] * 2 * P.N;
    sV[e] = u[P.sub[i]];
    sV[nn + e] = u[P.N + P.sub[i]];
}

__device__ inline double knot_dt(const RobParams& P, const double* __restrict__ Z, long long t) {
    return P.off_dt >= 0 ? Z[t * P.zdim + P.off_dt] : P.dt_fixed;
}

// (X Y)[i][j] and (X' Y)[i][j] of planar complex n x n matrices
__device__ inline void mul_nn(const double* X, const double* Y, int n, int i, int j, double& re, double& im) {
    const int nn = n * n;
    double a = 0.0, b = 0.0;
    for (int m = 0; m < n; ++m) {
        const double xr = X[m * n + i], xi = X[nn + m * n + i], yr = Y[j * n + m], yi = Y[nn + j * n + m];
        a = fma(xr, yr, fma(-xi, yi, a));
        b = fma(xr, yi, fma(xi, yr, b));
    }
    re = a;
    im = b;
}
__device__ inline void mul_cn(const double* X, const double* Y, int n, int i, int j, double& re, double& im) {
    const int nn = n * n;
    double a = 0.0, b = 0.0;
    for (int m = 0; m < n; ++m) {
        const double xr = X[i * n + m], xi = X[nn + i * n + m], yr = Y[j * n + m], yi = Y[nn + j * n + m];
        a = fma(xr, yr, fma(xi, yi, a));
        b = fma(xr, yi, fma(-xi, yr, b));
    }
    re = a;
    im = b;
}

__global__ __launch_bounds__(kRobThreads) void qc_robust_partial_kernel(RobParams P, const double* __restrict__ Z, double* __restrict__ part) {
    extern __shared__ double sm[];
    const int n = P.n, nn = n * n, kp = P.kp, E = 2 * nn + 1;
    double* sH = sm;
    double* sV = sH + 2 * nn;
    double* sW = sV + kp * 2 * nn;
    double* sAcc = sW + kp * 2 * nn;
    const int tid = threadIdx.x;
    for (int e = tid; e < 2 * nn; e += kRobThreads) sH[e] = P.H[e];
    for (int e = tid; e < kp * E; e += kRobThreads) sAcc[e] = 0.0;
    for (long long g = blockIdx.x; g < P.ngroups; g += gridDim.x) {
        const long long t0 = g * kp;
        __syncthreads();
        for (int idx = tid; idx < kp * nn; idx += kRobThreads) {
            const int k = idx / nn;
            if (t0 + k < P.K) load_v(P, Z, t0 + k, idx - k * nn, sV + k * 2 * nn);
        }
        __syncthreads();
        for (int idx = tid; idx < kp * nn; idx += kRobThreads) {
            const int k = idx / nn, e = idx - k * nn;
            if (t0 + k >= P.K) continue;
            double re, im;
            mul_nn(sH, sV + k * 2 * nn, n, e % n, e / n, re, im);
            sW[k * 2 * nn + e] = re;
            sW[k * 2 * nn + nn + e] = im;
        }
        __syncthreads();
        for (int idx = tid; idx < kp * nn; idx += kRobThreads) {
            const int k = idx / nn, e = idx - k * nn;
            const long long t = t0 + k;
            if (t >= P.K) continue;
            double re, im;
            mul_cn(sV + k * 2 * nn, sW + k * 2 * nn, n, e % n, e / n, re, im);
            const double dt = knot_dt(P, Z, t);
            double* acc = sAcc + k * E;
            acc[e] = fma(dt, re, acc[e]);
            acc[nn + e] = fma(dt, im, acc[nn + e]);
            if (e == 0) acc[2 * nn] += dt;
        }
    }
    __syncthreads();
    for (int e = tid; e < E; e += kRobThreads) {
        double s = 0.0;
        for (int k = 0; k < kp; ++k) s += sAcc[k * E + e];
        part[(long long)blockIdx.x * E + e] = s;
    }
}

// glob = [R (2n^2) | tau | L]
__global__ __launch_bounds__(kRobThreads) void qc_robust_reduce_kernel(const double* __restrict__ part, int nparts, int n,
                                                                       double* __restrict__ glob, double* __restrict__ dL) {
    extern __shared__ double sm[];
    const int nn = n * n, E = 2 * nn + 1, tid = threadIdx.x;
    double* sums = sm;
    double* red = sm + E;
    for (int e = tid; e < E; e += kRobThreads) {
        double s0 = 0.0, s1 = 0.0;
        int b = 0;
        for (; b + 1 < nparts; b += 2) {
            s0 += part[(long long)b * E + e];
            s1 += part[(long long)(b + 1) * E + e];
        }
        if (b < nparts) s0 += part[(long long)b * E + e];
        sums[e] = s0 + s1;
    }
    __syncthreads();
    const double tau = sums[2 * nn];
    double q = 0.0;
    for (int e = tid; e < 2 * nn; e += kRobThreads) {
        const double R = sums[e] / tau;
        glob[e] = R;
        q = fma(R, R, q);
    }
    red[tid] = q;
    __syncthreads();
    for (int off = kRobThreads / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        const double L = red[0] / n;
        glob[2 * nn] = tau;
        glob[2 * nn + 1] = L;
        dL[0] = L;
    }
}

__global__ __launch_bounds__(kRobThreads) void qc_robust_grad_kernel(RobParams P, const double* __restrict__ Z, const double* __restrict__ glob,
                                                                     double* __restrict__ grad, double* __restrict__ r, double* __restrict__ cvec,
                                                                     double* __restrict__ dtn) {
    extern __shared__ double sm[];
    const int n = P.n, nn = n * n, kp = P.kp, tid = threadIdx.x, m2 = 2 * nn;
    double* sH = sm;
    double* sR = sH + m2;
    double* sV = sR + m2;            // per knot: V, W = H V, X = H' V, A = V' W, G = W R' + X R
    double* sW = sV + kp * m2;
    double* sX = sW + kp * m2;
    double* sA = sX + kp * m2;
    double* sG = sA + kp * m2;
    double* sq = sG + kp * m2;       // kp
    double* sdt = sq + kp;           // kp
    const long long t0 = (long long)blockIdx.x * kp;
    const double tau = glob[m2];
    const double two_n = 2.0 / n;
    if (grad && blockIdx.x == 0)
        for (long long i = tid; i < P.global_dim; i += kRobThreads) grad[P.T * P.zdim + i] = 0.0;
    for (int e = tid; e < m2; e += kRobThreads) {
        sH[e] = P.H[e];
        sR[e] = glob[e];
    }
    for (int k = tid; k < kp; k += kRobThreads) sdt[k] = t0 + k < P.K ? knot_dt(P, Z, t0 + k) : 0.0;
    for (int idx = tid; idx < kp * nn; idx += kRobThreads) {
        const int k = idx / nn;
        if (t0 + k < P.K) load_v(P, Z, t0 + k, idx - k * nn, sV + k * m2);
    }
    __syncthreads();
    for (int idx = tid; idx < kp * nn; idx += kRobThreads) {
        const int k = idx / nn, e = idx - k * nn, i = e % n, j = e / n;
        if (t0 + k >= P.K) continue;
        const double* V = sV + k * m2;
        double re, im;
        mul_nn(sH, V, n, i, j, re, im);
        sW[k * m2 + e] = re;
        sW[k * m2 + nn + e] = im;
        mul_cn(sH, V, n, i, j, re, im);
        sX[k * m2 + e] = re;
        sX[k * m2 + nn + e] = im;
    }
    __syncthreads();
    for (int idx = tid; idx < kp * nn; idx += kRobThreads) {
        const int k = idx / nn, e = idx - k * nn, i = e % n, j = e / n;
        if (t0 + k >= P.K) continue;
        const double *V = sV + k * m2, *W = sW + k * m2, *X = sX + k * m2;
        double re, im;
        mul_cn(V, W, n, i, j, re, im);
        sA[k * m2 + e] = re;
        sA[k * m2 + nn + e] = im;
        // G'[i][j] = sum_m W[i][m] conj(R[j][m]) + X[i][m] R[m][j]
        double a = 0.0, b = 0.0;
        for (int m = 0; m < n; ++m) {
            const double wr = W[m * n + i], wi = W[nn + m * n + i], rr = sR[m * n + j], ri = sR[nn + m * n + j];
            a = fma(wr, rr, fma(wi, ri, a));
            b = fma(wi, rr, fma(-wr, ri, b));
            const double xr = X[m * n + i], xi = X[nn + m * n + i], sr = sR[j * n + m], si = sR[nn + j * n + m];
            a = fma(xr, sr, fma(-xi, si, a));
            b = fma(xr, si, fma(xi, sr, b));
        }
        sG[k * m2 + e] = a;
        sG[k * m2 + nn + e] = b;
    }
    __syncthreads();
    for (int k = tid; k < kp; k += kRobThreads) {
        double s = 0.0;
        if (t0 + k < P.K) {
            const double* A = sA + k * m2;
            for (int e = 0; e < m2; ++e) s = fma(sR[e], A[e] - sR[e], s);
        }
        sq[k] = s / tau;
    }
    __syncthreads();
    if (grad) {
        for (int idx = tid; idx < kp * P.zdim; idx += kRobThreads) {
            const int k = idx / P.zdim, j = idx - k * P.zdim;
            const long long t = t0 + k;
            if (t >= P.T) break;
            double val = 0.0;
            const int p = P.slot[j];
            if (t < P.K && p >= 0) {
                const int* v = P.var + 4 * p;
                if (v[0]) val = two_n * sq[k];
                else val = two_n * sdt[k] * (sG[k * m2 + v[3] * nn + v[2] * n + v[1]] / tau);
            }
            grad[t * P.zdim + j] = val;
        }
    }
    if (!r) return;
    for (int idx = tid; idx < kp * P.P * P.m2p; idx += kRobThreads) {
        const int kq = idx / P.m2p, kk = idx - kq * P.m2p, k = kq / P.P, p = kq - k * P.P;
        const long long t = t0 + k;
        if (t >= P.K) break;
        double val = 0.0;
        if (kk < m2) {
            const int im = kk >= nn, e = kk - im * nn, i = e % n, j = e / n;
            const int* v = P.var + 4 * p;
            if (v[0]) {
                val = (sA[k * m2 + kk] - sR[kk]) / tau;
            } else {
                const int a = v[1], b = v[2];
                const double *W = sW + k * m2, *X = sX + k * m2;
                // E[i][j] = conj(c) delta_ib W[a][j] + c delta_jb conj(X[a][i]),  c = 1 (re) or i (im)
                const double t1r = i == b ? W[j * n + a] : 0.0, t1i = i == b ? W[nn + j * n + a] : 0.0;
                const double t2r = j == b ? X[i * n + a] : 0.0, t2i = j == b ? -X[nn + i * n + a] : 0.0;
                double er, ei;
                if (v[3]) { er = -(t2i - t1i); ei = t2r - t1r; }
                else { er = t1r + t2r; ei = t1i + t2i; }
                val = (sdt[k] / tau) * (im ? ei : er);
            }
        }
        r[(t * P.P + p) * P.m2p + kk] = val;
    }
    for (int idx = tid; idx < kp * P.P; idx += kRobThreads) {
        const int k = idx / P.P, p = idx - k * P.P;
        const long long t = t0 + k;
        if (t >= P.K) break;
        const int* v = P.var + 4 * p;
        cvec[t * P.P + p] = v[0] ? sq[k] : sG[k * m2 + v[3] * nn + v[2] * n + v[1]] / tau;
        if (p == 0) dtn[t] = sdt[k] / tau;
    }
}

struct SyrkParams {
    long long V, ntiles;
    int n, P, m2p;
    const double* H;
    const int* var;
};

// one wave per 16 x 16 tile (I <= J) of the upper triangle: D[row][col] = sum_k r[16J + row][k] r[16I + col][k], so the lanes of
// one result register hold 16 consecutive rows i of one column j -- 128 contiguous bytes of the packed triangle
__global__ __launch_bounds__(kRobThreads) void qc_robust_syrk_kernel(SyrkParams S, const double* __restrict__ r, const double* __restrict__ cvec,
                                                                     const double* __restrict__ dtn, const double* __restrict__ glob,
                                                                     double* __restrict__ hess) {
    const long long tile = (long long)blockIdx.x * (kRobThreads / 64) + (threadIdx.x >> 6);
    if (tile >= S.ntiles) return;
    long long J = (long long)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
    while ((J + 1) * (J + 2) / 2 <= tile) ++J;
    while (J * (J + 1) / 2 > tile) --J;
    const long long I = tile - J * (J + 1) / 2;
    const int lane = threadIdx.x & 63, l16 = lane & 15, kq = lane >> 4;
    const double* ra = r + (16 * J + l16) * S.m2p + kq;
    const double* rb = r + (16 * I + l16) * S.m2p + kq;
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < S.m2p; k += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[k], rb[k], acc, 0, 0, 0);
    const int n = S.n, nn = n * n, m2 = 2 * nn;
    const double tau = glob[m2], two_n = 2.0 / n;
    const long long i = 16 * I + l16;
    const long long ti = i / S.P;
    const int pi = (int)(i - ti * S.P);
    const int* vi = S.var + 4 * pi;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long long j = 16 * J + kq + 4 * q;
        if (j >= S.V || i > j) continue;
        const long long tj = j / S.P;
        const int pj = (int)(j - tj * S.P);
        const int* vj = S.var + 4 * pj;
        double c = 0.0;
        if (!vi[0] && !vj[0]) {
            if (ti == tj) {
                // (dt/tau) [Re(conj(R[b,d]) ph H[a,a2]) + Re(conj(R[d,b]) conj(ph) H[a2,a])],  ph = conj(c_x) c_y
                const int a = vi[1], b = vi[2], a2 = vj[1], d = vj[2];
                const double phr = vi[3] == vj[3] ? 1.0 : 0.0, phi = vi[3] == vj[3] ? 0.0 : (vj[3] ? 1.0 : -1.0);
                const double h1r = S.H[a2 * n + a], h1i = S.H[nn + a2 * n + a], h2r = S.H[a * n + a2], h2i = S.H[nn + a * n + a2];
                const double r1r = glob[d * n + b], r1i = glob[nn + d * n + b], r2r = glob[b * n + d], r2i = glob[nn + b * n + d];
                const double p1r = phr * h1r - phi * h1i, p1i = phr * h1i + phi * h1r;    // ph H[a,a2]
                const double p2r = phr * h2r + phi * h2i, p2i = phr * h2i - phi * h2r;    // conj(ph) H[a2,a]
                c = dtn[ti] * ((r1r * p1r + r1i * p1i) + (r2r * p2r + r2i * p2i));
            }
        } else if (!vi[0]) {
            c = ((ti == tj ? 1.0 : 0.0) - dtn[ti]) * cvec[i];
        } else if (!vj[0]) {
            c = ((ti == tj ? 1.0 : 0.0) - dtn[tj]) * cvec[j];
        } else {
            c = -(cvec[i] + cvec[j]) / tau;
        }
        __builtin_nontemporal_store(two_n * (acc[q] + c), hess + j * (j + 1) / 2 + i);
    }
}

thread_local std::string g_rerr;
int rfail(qc_side* h, int code, const std::string& msg) { return qc_side_fail(h, &g_rerr, code, msg); }

}  // namespace

struct qc_robust : qc_side {
    qc_robust_desc d{};
    int n = 0, P = 0, kp = 0, m2p = 0, nparts = 0;
    int64_t V = 0, Vp = 0, nh = 0, ngroups = 0, Zlen = 0;
    size_t lds_partial = 0, lds_grad = 0;
    std::vector<int64_t> local;   // P sorted offsets inside a knot
    int *dsub = nullptr, *dslot = nullptr, *dvar = nullptr;
    double *dH = nullptr, *dpart = nullptr, *dglob = nullptr, *dr = nullptr, *dcvec = nullptr, *ddtn = nullptr;
    double *dZ = nullptr, *dL = nullptr, *dgrad = nullptr, *dhess = nullptr;   // staging of the host-pointer entry (dhess: at the first call that asks for it)
};

namespace {

struct RobLayout {
    int n = 0, P = 0;
    int64_t V = 0;
    std::vector<int> sub;
    std::vector<int64_t> local;   // sorted offsets inside a knot
    std::vector<int> var;         // P x 4
    std::vector<int> slot;        // zdim
};

int robust_layout(const qc_robust_desc* d, RobLayout* out) {
    if (!d) return rfail(nullptr, QC_ERR_INVALID, "qc_robust: NULL descriptor");
    if (d->T < 1 || d->zdim < 1 || d->global_dim < 0) return rfail(nullptr, QC_ERR_INVALID, "qc_robust: bad T / zdim / global_dim");
    if (d->N < 1) return rfail(nullptr, QC_ERR_INVALID, "qc_robust: N must be >= 1");
    if (d->off_state < 0 || (int64_t)d->off_state + 2 * (int64_t)d->N * d->N > d->zdim)
        return rfail(nullptr, QC_ERR_INVALID, "qc_robust: the state component (2N^2 entries from off_state) does not fit inside the knot (zdim)");
    if (d->off_dt >= d->zdim || d->off_dt < -1) return rfail(nullptr, QC_ERR_INVALID, "qc_robust: off_dt outside the knot");
    if (d->off_dt >= d->off_state && d->off_dt < d->off_state + 2 * d->N * d->N)
        return rfail(nullptr, QC_ERR_INVALID, "qc_robust: off_dt inside the state component");
    if (d->n_knots < 1 || d->n_knots > d->T) return rfail(nullptr, QC_ERR_INVALID, "qc_robust: n_knots must be in 1 .. T");
    if (d->hessian != QC_ROBUST_HESS_NONE && d->hessian != QC_ROBUST_HESS_EXACT)
        return rfail(nullptr, QC_ERR_INVALID, "qc_robust: hessian must be QC_ROBUST_HESS_NONE (0) or QC_ROBUST_HESS_EXACT (1)");
    if (!d->H_re) return rfail(nullptr, QC_ERR_INVALID, "qc_robust: H_re is NULL");
    out->sub.clear();
    if (d->subspace) {
        if (d->n_sub < 1 || d->n_sub > d->N) return rfail(nullptr, QC_ERR_INVALID, "qc_robust: n_sub must be in 1 .. N");
        std::vector<char> seen(d->N, 0);
        for (int a = 0; a < d->n_sub; ++a) {
            const int s = d->subspace[a];
            if (s < 0 || s >= d->N || seen[s]) return rfail(nullptr, QC_ERR_INVALID, "qc_robust: subspace levels must be distinct and in 0 .. N-1");
            seen[s] = 1;
            out->sub.push_back(s);
        }
    } else {
        if (d->n_sub != 0 && d->n_sub != d->N) return rfail(nullptr, QC_ERR_INVALID, "qc_robust: NULL subspace needs n_sub = 0 or N");
        for (int a = 0; a < d->N; ++a) out->sub.push_back(a);
    }
    if (2 * d->N > 64)
        return rfail(nullptr, QC_ERR_UNSUPPORTED, "qc_robust: 2N = " + std::to_string(2 * d->N) + " exceeds the supported 2N <= 64");
    const int n = (int)out->sub.size();
    out->n = n;
    std::vector<std::pair<int64_t, int>> ent;   // (offset, 4-tuple index)
    std::vector<int> tup;
    for (int b = 0; b < n; ++b)
        for (int part = 0; part < 2; ++part)
            for (int a = 0; a < n; ++a) {
                ent.push_back({d->off_state + (int64_t)out->sub[b] * 2 * d->N + part * d->N + out->sub[a], (int)tup.size() / 4});
                tup.insert(tup.end(), {0, a, b, part});
            }
    if (d->off_dt >= 0) {
        ent.push_back({d->off_dt, (int)tup.size() / 4});
        tup.insert(tup.end(), {1, 0, 0, 0});
    }
    std::sort(ent.begin(), ent.end());
    out->P = (int)ent.size();
    out->local.resize(out->P);
    out->var.resize(4 * (size_t)out->P);
    out->slot.assign(d->zdim, -1);
    for (int p = 0; p < out->P; ++p) {
        out->local[p] = ent[p].first;
        for (int q = 0; q < 4; ++q) out->var[4 * p + q] = tup[4 * ent[p].second + q];
        out->slot[ent[p].first] = p;
    }
    out->V = d->n_knots * (int64_t)out->P;
    if (d->hessian == QC_ROBUST_HESS_EXACT && out->V * (out->V + 1) / 2 > kRobHessCap)
        return rfail(nullptr, QC_ERR_UNSUPPORTED,
                     "qc_robust: the exact Hessian over V = " + std::to_string(out->V) + " variables has " + std::to_string(out->V * (out->V + 1) / 2) +
                         " entries, more than the supported 2^27 (1 GiB of values)");
    return QC_OK;
}

}  // namespace

extern "C" const char* qc_robust_last_error(const qc_robust* h) { return h ? h->err.c_str() : g_rerr.c_str(); }

extern "C" int64_t qc_sizeof_robust_desc(void) { return (int64_t)sizeof(qc_robust_desc); }

extern "C" int qc_robust_desc_n_vars(const qc_robust_desc* d, int64_t* n_vars) {
    RobLayout L;
    int rc = robust_layout(d, &L);
    if (rc) return rc;
    if (!n_vars) return rfail(nullptr, QC_ERR_INVALID, "qc_robust_desc_n_vars: NULL output");
    *n_vars = L.V;
    return QC_OK;
}

extern "C" int qc_robust_desc_vars(const qc_robust_desc* d, int64_t* vars) {
    RobLayout L;
    int rc = robust_layout(d, &L);
    if (rc) return rc;
    if (!vars) return rfail(nullptr, QC_ERR_INVALID, "qc_robust_desc_vars: NULL output");
    for (int64_t t = 0, v = 0; t < d->n_knots; ++t)
        for (int p = 0; p < L.P; ++p) vars[v++] = t * d->zdim + L.local[p];
    return QC_OK;
}

extern "C" int qc_robust_desc_hess_nnz(const qc_robust_desc* d, int64_t* nnz) {
    RobLayout L;
    int rc = robust_layout(d, &L);
    if (rc) return rc;
    if (!nnz) return rfail(nullptr, QC_ERR_INVALID, "qc_robust_desc_hess_nnz: NULL output");
    *nnz = d->hessian == QC_ROBUST_HESS_EXACT ? L.V * (L.V + 1) / 2 : 0;
    return QC_OK;
}

extern "C" int qc_robust_desc_hess_structure(const qc_robust_desc* d, int64_t* rows, int64_t* cols, int one_based) {
    RobLayout L;
    int rc = robust_layout(d, &L);
    if (rc) return rc;
    if (d->hessian != QC_ROBUST_HESS_EXACT) return QC_OK;
    if (!rows || !cols) return rfail(nullptr, QC_ERR_INVALID, "qc_robust_desc_hess_structure: NULL output");
    std::vector<int64_t> g(L.V);
    for (int64_t t = 0, v = 0; t < d->n_knots; ++t)
        for (int p = 0; p < L.P; ++p) g[v++] = t * d->zdim + L.local[p] + (one_based ? 1 : 0);
    int64_t e = 0;
    for (int64_t j = 0; j < L.V; ++j)
        for (int64_t i = 0; i <= j; ++i, ++e) {
            rows[e] = g[i];
            cols[e] = g[j];
        }
    return QC_OK;
}

extern "C" int qc_robust_create(const qc_robust_desc* d, qc_robust** out) {
    if (!out) return rfail(nullptr, QC_ERR_INVALID, "qc_robust_create: out is NULL");
    *out = nullptr;
    RobLayout L;
    int rc = robust_layout(d, &L);
    if (rc) return rc;
    if ((rc = qc_side_check_device(d->device, "qc_robust_create", &g_rerr))) return rc;
    qc_side_new<qc_robust> h(new qc_robust());
    h->d = *d;
    h->d.subspace = nullptr;    // caller-owned arrays are not retained
    h->d.H_re = h->d.H_im = nullptr;
    h->device = d->device;
    const int n = L.n, nn = n * n, m2 = 2 * nn;
    h->n = n;
    h->P = L.P;
    h->V = L.V;
    h->local = L.local;
    h->m2p = (m2 + 3) / 4 * 4;
    h->kp = std::max(1, std::min(64, kRobThreads / nn));
    h->ngroups = (d->n_knots + h->kp - 1) / h->kp;
    h->nparts = (int)std::min<int64_t>(h->ngroups, kRobMaxParts);
    h->Vp = (L.V + 15) / 16 * 16;
    h->nh = d->hessian == QC_ROBUST_HESS_EXACT ? L.V * (L.V + 1) / 2 : 0;
    h->Zlen = d->T * (int64_t)d->zdim + d->global_dim;
    h->lds_partial = ((size_t)m2 + (size_t)h->kp * (2 * m2 + m2 + 1)) * 8;
    h->lds_grad = ((size_t)2 * m2 + (size_t)h->kp * 5 * m2 + 2 * (size_t)h->kp) * 8;
    std::vector<double> Hp(m2);
    for (int e = 0; e < nn; ++e) {
        Hp[e] = d->H_re[e];
        Hp[nn + e] = d->H_im ? d->H_im[e] : 0.0;
    }
    qc_device_guard guard(d->device);
    QC_SIDE_HIP(nullptr, g_rerr, guard.err);
    QC_SIDE_HIP(nullptr, g_rerr, h->alloc(&h->dsub, L.sub.size(), L.sub.data()));
    QC_SIDE_HIP(nullptr, g_rerr, h->alloc(&h->dslot, L.slot.size(), L.slot.data()));
    QC_SIDE_HIP(nullptr, g_rerr, h->alloc(&h->dvar, L.var.size(), L.var.data()));
    QC_SIDE_HIP(nullptr, g_rerr, h->alloc(&h->dH, Hp.size(), Hp.data()));
    QC_SIDE_HIP(nullptr, g_rerr, h->alloc(&h->dpart, (size_t)h->nparts * (m2 + 1)));
    QC_SIDE_HIP(nullptr, g_rerr, h->alloc(&h->dglob, (size_t)(m2 + 2)));
    QC_SIDE_HIP(nullptr, g_rerr, h->alloc(&h->dZ, (size_t)h->Zlen));
    QC_SIDE_HIP(nullptr, g_rerr, h->alloc(&h->dL, 1));
    QC_SIDE_HIP(nullptr, g_rerr, h->alloc(&h->dgrad, (size_t)h->Zlen));
    if (h->nh) {
        // rows past V stay zero: the SYRK reads whole 16-row tiles
        QC_SIDE_HIP(nullptr, g_rerr, h->alloc(&h->dr, (size_t)h->Vp * h->m2p));
        QC_SIDE_HIP(nullptr, g_rerr, hipMemset(h->dr, 0, (size_t)h->Vp * h->m2p * 8));
        QC_SIDE_HIP(nullptr, g_rerr, h->alloc(&h->dcvec, (size_t)h->V));
        QC_SIDE_HIP(nullptr, g_rerr, h->alloc(&h->ddtn, (size_t)d->n_knots));
    }
    if (h->lds_partial > 65536)
        QC_SIDE_HIP(nullptr, g_rerr, hipFuncSetAttribute(reinterpret_cast<const void*>(qc_robust_partial_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_partial));
    if (h->lds_grad > 65536)
        QC_SIDE_HIP(nullptr, g_rerr, hipFuncSetAttribute(reinterpret_cast<const void*>(qc_robust_grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_grad));
    QC_SIDE_HIP(nullptr, g_rerr, h->open_stream());
    *out = h.release();
    return QC_OK;
}

extern "C" void qc_robust_destroy(qc_robust* h) {
    if (!h) return;
    h->release_device();
    delete h;
}

extern "C" int qc_robust_n_vars(const qc_robust* h, int64_t* n_vars) {
    if (!h || !n_vars) return rfail(nullptr, QC_ERR_INVALID, "qc_robust_n_vars: NULL argument");
    *n_vars = h->V;
    return QC_OK;
}

extern "C" int qc_robust_vars(const qc_robust* h, int64_t* vars) {
    if (!h || !vars) return rfail(nullptr, QC_ERR_INVALID, "qc_robust_vars: NULL argument");
    for (int64_t t = 0, v = 0; t < h->d.n_knots; ++t)
        for (int p = 0; p < h->P; ++p) vars[v++] = t * h->d.zdim + h->local[p];
    return QC_OK;
}

extern "C" int qc_robust_hess_nnz(const qc_robust* h, int64_t* nnz) {
    if (!h || !nnz) return rfail(nullptr, QC_ERR_INVALID, "qc_robust_hess_nnz: NULL argument");
    *nnz = h->nh;
    return QC_OK;
}

extern "C" int qc_robust_hess_structure(const qc_robust* h, int64_t* rows, int64_t* cols, int one_based) {
    if (!h) return rfail(nullptr, QC_ERR_INVALID, "qc_robust_hess_structure: NULL handle");
    if (!h->nh) return QC_OK;
    if (!rows || !cols) return rfail(nullptr, QC_ERR_INVALID, "qc_robust_hess_structure: NULL output");
    std::vector<int64_t> g(h->V);
    qc_robust_vars(h, g.data());
    const int64_t b = one_based ? 1 : 0;
    int64_t e = 0;
    for (int64_t j = 0; j < h->V; ++j)
        for (int64_t i = 0; i <= j; ++i, ++e) {
            rows[e] = g[i] + b;
            cols[e] = g[j] + b;
        }
    return QC_OK;
}

extern "C" int qc_robust_eval_dev(qc_robust* h, const double* dZ, double* dL, double* dgrad, double* dhvals, void* stream) {
    if (!h) return rfail(nullptr, QC_ERR_INVALID, "qc_robust_eval_dev: NULL handle");
    if (!dZ) return rfail(h, QC_ERR_INVALID, "qc_robust_eval_dev: NULL input");
    if (dhvals && !h->nh) return rfail(h, QC_ERR_INVALID, "qc_robust_eval_dev: Hessian values requested from a handle created without a Hessian");
    qc_device_guard guard(h->device);
    QC_SIDE_HIP(h, g_rerr, guard.err);
    RobParams P;
    P.T = h->d.T;
    P.K = h->d.n_knots;
    P.global_dim = h->d.global_dim;
    P.ngroups = h->ngroups;
    P.zdim = h->d.zdim;
    P.off_state = h->d.off_state;
    P.N = h->d.N;
    P.n = h->n;
    P.off_dt = h->d.off_dt;
    P.kp = h->kp;
    P.P = h->P;
    P.m2p = h->m2p;
    P.nparts = h->nparts;
    P.dt_fixed = h->d.dt_fixed;
    P.sub = h->dsub;
    P.H = h->dH;
    P.slot = h->dslot;
    P.var = h->dvar;
    hipStream_t s = (hipStream_t)stream;
    const int m2 = 2 * h->n * h->n;
    double* Lout = dL ? dL : h->dglob + m2 + 1;     // (the reducer always writes L into glob as well)
    hipLaunchKernelGGL(qc_robust_partial_kernel, dim3(h->nparts), dim3(kRobThreads), h->lds_partial, s, P, dZ, h->dpart);
    hipLaunchKernelGGL(qc_robust_reduce_kernel, dim3(1), dim3(kRobThreads), (size_t)(m2 + 1 + kRobThreads) * 8, s, (const double*)h->dpart,
                       h->nparts, h->n, h->dglob, Lout);
    if (dgrad || dhvals) {
        const unsigned grid = (unsigned)((h->d.T + h->kp - 1) / h->kp);
        hipLaunchKernelGGL(qc_robust_grad_kernel, dim3(grid), dim3(kRobThreads), h->lds_grad, s, P, dZ, (const double*)h->dglob, dgrad,
                           dhvals ? h->dr : nullptr, h->dcvec, h->ddtn);
    }
    if (dhvals) {
        SyrkParams S;
        S.V = h->V;
        S.ntiles = (h->Vp / 16) * (h->Vp / 16 + 1) / 2;
        S.n = h->n;
        S.P = h->P;
        S.m2p = h->m2p;
        S.H = h->dH;
        S.var = h->dvar;
        const unsigned grid = (unsigned)((S.ntiles + 3) / 4);
        hipLaunchKernelGGL(qc_robust_syrk_kernel, dim3(grid), dim3(kRobThreads), 0, s, S, (const double*)h->dr, (const double*)h->dcvec,
                           (const double*)h->ddtn, (const double*)h->dglob, dhvals);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rfail(h, QC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return QC_OK;
}

extern "C" int qc_robust_eval(qc_robust* h, const double* Z, double* L, double* grad, double* hvals) {
    if (!h) return rfail(nullptr, QC_ERR_INVALID, "qc_robust_eval: NULL handle");
    if (!Z) return rfail(h, QC_ERR_INVALID, "qc_robust_eval: NULL input");
    if (hvals && !h->nh) return rfail(h, QC_ERR_INVALID, "qc_robust_eval: Hessian values requested from a handle created without a Hessian");
    qc_device_guard guard(h->device);
    QC_SIDE_HIP(h, g_rerr, guard.err);
    if (hvals && !h->dhess) QC_SIDE_HIP(h, g_rerr, h->alloc(&h->dhess, (size_t)h->nh));
    QC_SIDE_HIP(h, g_rerr, hipMemcpyAsync(h->dZ, Z, (size_t)h->Zlen * 8, hipMemcpyHostToDevice, h->stream));
    int rc = qc_robust_eval_dev(h, h->dZ, h->dL, grad ? h->dgrad : nullptr, hvals ? h->dhess : nullptr, h->stream);
    if (rc) return rc;
    double l = 0.0;
    QC_SIDE_HIP(h, g_rerr, hipMemcpyAsync(&l, h->dL, 8, hipMemcpyDeviceToHost, h->stream));
    if (grad) QC_SIDE_HIP(h, g_rerr, hipMemcpyAsync(grad, h->dgrad, (size_t)h->Zlen * 8, hipMemcpyDeviceToHost, h->stream));
    if (hvals) QC_SIDE_HIP(h, g_rerr, hipMemcpyAsync(hvals, h->dhess, (size_t)h->nh * 8, hipMemcpyDeviceToHost, h->stream));
    QC_SIDE_HIP(h, g_rerr, hipStreamSynchronize(h->stream));
    if (L) *L = l;
    return QC_OK;
}
