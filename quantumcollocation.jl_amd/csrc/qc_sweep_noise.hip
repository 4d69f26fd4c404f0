// Noise-trajectory sweeps: S samples of one pulse whose perturbation amplitudes change from interval to interval.  In interval
// t = 0 .. T-2, for sample s,
//     G_{s,t} = G_drift + sum_j (theta[s,j] + xi[s,t,j]) P_j + sum_k c[s,k] a_{t,k} G_k,      x_{t+1} = exp(h_t G_{s,t}) x_t,  x_0 = init,
// with `noise` = xi, S x (T-1) x n_pert, sample-major, then interval, then perturbation.  A detuning that drifts during the pulse
// (Ornstein-Uhlenbeck, 1/f), additive noise on a drive line (P_j = G_k), S realisations of a stochastic average: one launch that fills
// the device instead of S single-sample calls with the noise written into S copies of Z.
//
// "mfma16-sweep" handles with n_pert >= 1 and m + n_pert <= 8.  A sweep wavefront already keeps the m drive tiles in registers and
// rebuilds G = base + sum a_u G_u every interval; a perturbation whose amplitude changes per interval is one more such tile whose
// "control" is read per sample.  Both kernels are their qc_sweep.hip / qc_sweep_grad.hip counterparts (read those headers first: work item,
// chunk rule, lane maps, the squaring rule, the Horner table) with M' = m + n_pert tiles, M in {1, 2, 4, 6, 8}: the drives, then P_0 .. P_{p-1}.
//   * lane k < m reads control k from Z and multiplies it by c[s,k]; lane m + j reads noise[s,t,j], factor 1: one load per lane and
//     interval (a per-lane choice between two wave-uniform addresses), requested one interval ahead as the controls are;
//   * base folds theta as in the sweep; Ga = base, the drive fmas in ascending k, THEN the noise fmas in ascending j.  At xi = +0.0 the
//     extra fmas leave every value as it was (fma(0, P, Ga) may turn a -0 into +0, nothing else), so finals / fids / grad / grad_samples
//     equal qc_sweep_eval's and qc_sweep_grad's on the same handle value for value;
//   * everything after Ga is the sweep's: qc_sweep_noise_kernel stores the chunk totals to h->dTot and qc_sweep_finish_kernel follows
//     unchanged; the gradient runs the fidelity's seed, qc_sweep_noise_grad_kernel, and the reductions of qc_sweep_grad.hip unchanged.
// The backward walk reduces sum(ZT_t . G_u) over all m + n_pert tiles.  The perturbation tiles give
//     grad_noise[s,t,j] = dF_s/dxi[s,t,j] = sum(ZT_t . P_j)       (ZT_t = h_t L(h_t G^T; lambda_{t+1} x_t^T), as in qc_sweep_grad.hip),
// the time-resolved sensitivity of every sample (qc_sweep_grad_params sums it over t: sum_t grad_noise[s,t,j] = grad_theta[s,j] at
// xi = 0).  The interval's values leave through two vector stores: lanes 0 .. m-1 (the drives) and lane m + p (the
// timestep) to grad_samples in the gradient's layout, lanes m .. m+p-1 to grad_noise; either buffer may be absent.  No atomics: repeated calls return the same bits, and no output's bits depend
// on which others were requested.  A non-finite xi[s,t,j] stays inside sample s (and the weighted sums over the samples).
// Cost against the sweep at the same M: n_pert more fmas per tile register (4 n_pert) and the same single load per interval; the
// gradient adds n_pert wave reductions per interval.
//
// Out of scope: "mfma32-sweep" and "rollout-per-sample" handles, pullbacks / pushforwards / Hessian products with noise, several devices.
//
// gfx950 cross-compile: see the table in DESIGN.md ("Noise-trajectory sweeps"); no private segment, no spills in any instantiation.
#include <math.h>
#include <stdint.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_mfma;

// the constants of qc_sweep.hip / qc_sweep_grad.hip, restated (those files' are internal to them)
constexpr int kNDeg = 8;
constexpr double kNTh = 0.125;
constexpr int kNTiles = 8;          // tiles a wave keeps in registers: drives and perturbations together
constexpr int kNWaves = 4;          // (sample, chunk) items per workgroup: one wave each, the waves never synchronise
constexpr int kNGSlice = 2 * 272;   // LDS doubles of one wave of the backward walk: two transposition tiles

__constant__ const double kNInvFact[kNDeg + 1] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0};

struct NoiseParams {
    int n, nc, m, p, zdim, off_a, off_dt, n_int, chunk, n_chunks, nd;   // nd = m + (off_dt >= 0): derivatives per interval in grad_samples
    long long items;             // S * n_chunks
    double dt_fixed;
    const double* img;           // A-layout images [matrix][kk][lane]: drift, m drives, p perturbations
};

template <int CTRL>
__device__ inline double ndpp(double x) {
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ inline v4d nimg(const double* __restrict__ img, int mat, int lane) {
    const double* p = img + (size_t)mat * 256 + lane;
    return v4d{p[0], p[64], p[128], p[192]};
}

__device__ __forceinline__ v4d nmma(const v4d& a, const v4d& b, v4d acc) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], b[kk], acc, 0, 0, 0);
    return acc;
}

// (R, dR) <- (A R + C,  dA R + A dR): gstep of qc_sweep_grad.hip
__device__ __forceinline__ void nstep(const v4d& A, const v4d& dA, v4d& R, v4d& dR, const v4d& C) {
    const v4d z = {0.0, 0.0, 0.0, 0.0};
    v4d a0 = z, a1 = z, a2 = C;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(dA[kk], R[kk], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[kk], dR[kk], a1, 0, 0, 0);
        a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[kk], R[kk], a2, 0, 0, 0);
    }
    dR = a0 + a1;
    R = a2;
}

// the sum over the 64 lanes in a fixed order, wave-uniform: wave_sum of qc_sweep_grad.hip
__device__ inline double nwave_sum(double v) {
    v += ndpp<0x128>(v);
    v += ndpp<0x124>(v);
    v += ndpp<0x122>(v);
    v += ndpp<0x121>(v);
    return (bcast_lane(v, 0) + bcast_lane(v, 16)) + (bcast_lane(v, 32) + bcast_lane(v, 48));
}

// the number of squarings of the interval: the rule of qc_sweep_mfma16_kernel, expression for expression
__device__ __forceinline__ int nsquarings(double h, const v4d& Ga) {
    int sq = 0;
    double best = 0.0;
    bool bad = false;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        double cs = fabs(h * Ga[kk]);
        cs += ndpp<0x128>(cs);
        cs += ndpp<0x124>(cs);
        cs += ndpp<0x122>(cs);
        cs += ndpp<0x121>(cs);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double v = bcast_lane(cs, 16 * r);
            if (!(v == v) || v > 1e300) bad = true;
            best = fmax(best, v);
        }
    }
    if (!bad && best > kNTh) {
        int e;
        (void)frexp(best / kNTh, &e);
        sq = e;
        if (ldexp(kNTh, e - 1) >= best) sq = e - 1;
        sq = sq < 0 ? 0 : (sq > 60 ? 60 : sq);
    }
    return __builtin_amdgcn_readfirstlane(sq);
}

// Where lane l finds the coefficient of tile min(l, m + p - 1).  Drive lanes read the shared controls of knot t of Z, perturbation
// lanes the sample's own noise of interval t; lanes past the last tile repeat the last one (p >= 1: there always is one).
struct LaneCoef {
    int off;             // inside the knot (off_a + k), or inside the interval's noise values (j)
    bool drv;
    double cl;           // c[s,k] for a drive lane, 1 for a perturbation lane
};

__device__ __forceinline__ LaneCoef lane_coef(const NoiseParams& P, int lane, long long s, const double* __restrict__ scale) {
    const int m = P.m, mt = m + P.p;
    const int kl = lane < mt ? lane : mt - 1;
    LaneCoef c;
    c.drv = kl < m;
    c.off = c.drv ? P.off_a + kl : kl - m;
    c.cl = (scale && c.drv) ? scale[s * m + kl] : 1.0;
    return c;
}

// one load per lane: knot t of Z (`zt`) or interval t of the sample's noise (`nt`), both wave-uniform addresses
__device__ __forceinline__ double lane_load(const LaneCoef& c, const double* __restrict__ zt, const double* __restrict__ nt) {
    return (c.drv ? zt : nt)[c.off];
}

// Launch 1: the chunk totals.  qc_sweep_mfma16_kernel with m + p tiles and the per-lane coefficient source.
template <int M>
__global__ __launch_bounds__(64 * kNWaves, 2) void qc_sweep_noise_kernel(const NoiseParams P, const double* __restrict__ Z,
                                                                          const double* __restrict__ theta, const double* __restrict__ scale,
                                                                          const double* __restrict__ noise, double* __restrict__ tot) {
    __shared__ double scr_all[kNWaves * 16 * 17];
    const int lane = threadIdx.x & 63;
    const int wq = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* __restrict__ scr = scr_all + wq * (16 * 17);
    const long long item = (long long)blockIdx.x * kNWaves + wq;
    if (item >= P.items) return;
    const long long s = item / P.n_chunks;
    const int c = (int)(item - s * P.n_chunks);
    const int t0 = c * P.chunk, t1 = min(P.n_int, t0 + P.chunk);
    const int g = lane >> 4, j = lane & 15;
    const int m = P.m, mt = m + P.p;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    // ---- once per wave: the sample's base tile, the drive and perturbation tiles --------------------------------------------
    v4d base = nimg(P.img, 0, lane);
    for (int q = 0; q < P.p; ++q) {
        const double th = theta[s * P.p + q];
        const v4d Pq = nimg(P.img, 1 + m + q, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) base[r] = fma(th, Pq[r], base[r]);
    }
    v4d Gj[M];      // the images follow one another: tile u is matrix 1 + u, drives then perturbations
#pragma unroll
    for (int u = 0; u < M; ++u) Gj[u] = u < mt ? nimg(P.img, 1 + u, lane) : zero;
    const LaneCoef lc = lane_coef(P, lane, s, scale);
    const double* __restrict__ ns = noise + s * P.n_int * (long long)P.p;      // the sample's noise

    const double* __restrict__ z = Z + (long long)t0 * P.zdim;
    double av = lane_load(lc, z, ns + (long long)t0 * P.p);
    const double hfix = opaque_scalar(P.dt_fixed);      // keeps the two arms apart: no flat load (qc_mfma_common.h)
    double h = ft ? z[P.off_dt] : hfix;
    v4d W = IdB;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        // the next interval's coefficients and timestep are requested before this interval's products
        const int tn = t + 1 < t1 ? t + 1 : t;
        const double* __restrict__ zn = Z + (long long)tn * P.zdim;
        const double av_n = lane_load(lc, zn, ns + (long long)tn * P.p);
        const double h_n = ft ? zn[P.off_dt] : hfix;
        const double al = av * lc.cl;
        v4d Ga = base;
#pragma unroll
        for (int u = 0; u < M; ++u) {
            const double a = u < mt ? bcast_lane(al, u) : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) Ga[r] = fma(a, Gj[u][r], Ga[r]);
        }
        const int sq = nsquarings(h, Ga);
        const double sc = ldexp(1.0, -sq);
        const v4d Y = (h * sc) * Ga;
        v4d R = kNInvFact[kNDeg] * IdB;
#pragma unroll 1
        for (int k = kNDeg; k >= 1; --k) R = nmma(Y, R, kNInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            const v4d Et = lds_transpose16(scr, R, g, j);
            R = nmma(Et, R, zero);
        }
        const v4d Et = lds_transpose16(scr, R, g, j);     // E^T in D layout = E in A layout
        W = nmma(Et, W, zero);
        av = av_n;
        h = h_n;
    }
    double* __restrict__ o = tot + item * 256;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[j * 16 + 4 * r + g] = W[r];
}

// Launch 3: the backward walk.  qc_sweep_grad_kernel<M, false> with m + p tiles; gs (S x (T-1) x nd) and gn (S x (T-1) x p) may each be
// NULL, not both.
template <int M>
__global__ __launch_bounds__(64 * kNWaves, 2) void qc_sweep_noise_grad_kernel(const NoiseParams P, const double* __restrict__ Z,
                                                                               const double* __restrict__ theta, const double* __restrict__ scale,
                                                                               const double* __restrict__ noise, const double* __restrict__ xs,
                                                                               const double* __restrict__ ls, double* __restrict__ gs,
                                                                               double* __restrict__ gn) {
    __shared__ double scr_all[kNWaves * kNGSlice];
    const int lane = threadIdx.x & 63;
    const int wq = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* __restrict__ scr = scr_all + wq * kNGSlice;
    const long long item = (long long)blockIdx.x * kNWaves + wq;
    if (item >= P.items) return;
    const long long s = item / P.n_chunks;
    const int c = (int)(item - s * P.n_chunks);
    const int t0 = c * P.chunk, t1 = min(P.n_int, t0 + P.chunk);
    const int g = lane >> 4, j = lane & 15;
    const int m = P.m, mt = m + P.p;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    v4d base = nimg(P.img, 0, lane);
    for (int q = 0; q < P.p; ++q) {
        const double th = theta[s * P.p + q];
        const v4d Pq = nimg(P.img, 1 + m + q, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) base[r] = fma(th, Pq[r], base[r]);
    }
    v4d Gj[M];
#pragma unroll
    for (int u = 0; u < M; ++u) Gj[u] = u < mt ? nimg(P.img, 1 + u, lane) : zero;
    const LaneCoef lc = lane_coef(P, lane, s, scale);
    const double* __restrict__ ns = noise + s * P.n_int * (long long)P.p;      // the sample's noise

    v4d x, lam;
    {
        const int ns = P.n * P.nc;
        const double* __restrict__ xe = xs + item * ns;
        const double* __restrict__ le = ls + item * ns;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * r + g;
            const bool in = row < P.n && j < P.nc;
            x[r] = in ? xe[row + P.n * j] : 0.0;
            lam[r] = in ? le[row + P.n * j] : 0.0;
        }
    }

    const double hfix = opaque_scalar(P.dt_fixed);
    const double* __restrict__ z = Z + (long long)(t1 - 1) * P.zdim;
    double av = lane_load(lc, z, ns + (long long)(t1 - 1) * P.p);
    double h = ft ? z[P.off_dt] : hfix;
#pragma unroll 1
    for (int t = t1 - 1; t >= t0; --t) {
        // the previous interval's coefficients and timestep are requested before this interval's products
        const int tn = t > t0 ? t - 1 : t;
        const double* __restrict__ zn = Z + (long long)tn * P.zdim;
        const double av_n = lane_load(lc, zn, ns + (long long)tn * P.p);
        const double h_n = ft ? zn[P.off_dt] : hfix;
        const double al = av * lc.cl;
        v4d Ga = base;
#pragma unroll
        for (int u = 0; u < M; ++u) {
            const double a = u < mt ? bcast_lane(al, u) : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) Ga[r] = fma(a, Gj[u][r], Ga[r]);
        }
        const int sq = nsquarings(h, Ga);
        const double hs = h * ldexp(1.0, -sq);
        // K^T = lambda x^T of knot t+1 (D layout) from the A-layout forms of both
        v4d KT;
        {
            const v4d in[2] = {x, lam};
            v4d tr[2];
            lds_transpose16_multi<2>(scr, in, tr, g, j);
            KT = nmma(tr[1], tr[0], zero);
        }
        // M = 8: the lane compares are made per interval from an opaque copy of the lane index (qc_sweep_grad_kernel: kept loop-invariant
        // they live in scalar registers and the kernel spills)
        int ln = lane;
        if constexpr (M >= 8) asm volatile("" : "+v"(ln));
        double out = 0.0;      // lane u < m + p: tile u (the drives, then the noise values); lane m + p: the timestep (free timesteps)
        if (ft && gs) {
            double ph = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) ph = fma(KT[r], Ga[r], ph);
            const double dh = -nwave_sum(ph);
            out = ln == mt ? dh : out;
        }
        const v4d Y = hs * Ga;
        const v4d dY = hs * KT;
        v4d R = kNInvFact[kNDeg] * IdB;
        v4d dR = zero;
#pragma unroll 1
        for (int k = kNDeg; k >= 1; --k) nstep(Y, dY, R, dR, kNInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            const v4d in[2] = {R, dR};
            v4d tr[2];
            lds_transpose16_multi<2>(scr, in, tr, g, j);      // E^T, dE^T in D layout = E, dE in A layout
            nstep(tr[0], tr[1], R, dR, zero);
        }
        const v4d ZT = nmma(R, dR, zero);                       // E^T dE
#pragma unroll
        for (int u = 0; u < M; ++u) {
            if (u < mt) {
                double pu = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) pu = fma(ZT[r], Gj[u][r], pu);
                const double du = nwave_sum(pu);
                out = ln == u ? du * lc.cl : out;      // a perturbation lane's factor is 1
            }
        }
        const long long it = s * P.n_int + t;
        if (gs && (ln < m || (ft && ln == mt))) gs[it * P.nd + (ln < m ? ln : m)] = out;
        if (gn && ln >= m && ln < mt) gn[it * P.p + (ln - m)] = out;
        x = nmma(R, x, zero);
        lam = nmma(R, lam, zero);
        av = av_n;
        h = h_n;
    }
}

NoiseParams noise_params(const qc_sweep* h, int64_t S, int64_t chunk, int64_t n_chunks) {
    NoiseParams P;
    P.n = h->n; P.nc = h->nc; P.m = h->d.m; P.p = h->d.n_pert; P.zdim = h->d.zdim; P.off_a = h->d.off_a; P.off_dt = h->d.off_dt;
    P.n_int = (int)(h->d.T - 1); P.chunk = (int)chunk; P.n_chunks = (int)n_chunks; P.nd = h->d.m + (h->d.off_dt >= 0 ? 1 : 0);
    P.items = S * n_chunks;
    P.dt_fixed = h->d.dt_fixed;
    P.img = h->dImg;
    return P;
}

// launch 1: grows h->dTot and launches qc_sweep_noise_kernel<M> (S x n_chunks tiles of 256 doubles, the layout of qc_sweep_launch_totals)
int noise_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dnoise, hipStream_t st,
                        int64_t* chunk_out, int64_t* n_chunks_out) {
    std::string& slot = *qc_sweep_err_slot();
    int64_t chunk, n_chunks;
    qc_sweep_chunks(S, h->d.T, &chunk, &n_chunks);
    QC_SIDE_HIP(h, slot, h->grow(h->dTot, (size_t)S * n_chunks * 256));
    const NoiseParams P = noise_params(h, S, chunk, n_chunks);
    const unsigned grid = (unsigned)((P.items + kNWaves - 1) / kNWaves);
#define QC_NOISE_LAUNCH(M_) hipLaunchKernelGGL(qc_sweep_noise_kernel<M_>, dim3(grid), dim3(64 * kNWaves), 0, st, P, dZ, dtheta, dscale, dnoise, h->dTot.p)
    QC_SWEEP_FOR_M(P.m + P.p, QC_NOISE_LAUNCH);
#undef QC_NOISE_LAUNCH
    *chunk_out = chunk;
    *n_chunks_out = n_chunks;
    return QC_OK;
}

// do `count` doubles at `a` share a byte with `cb` doubles at `b`?  (either NULL: no)
bool overlaps(const double* a, size_t count, const double* b, size_t cb) {
    if (!a || !b || !count || !cb) return false;
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + count * 8, b0 = (uintptr_t)b, b1 = b0 + cb * 8;
    return a0 < b1 && b0 < a1;
}

size_t noise_count(const qc_sweep* h, int64_t S) { return (size_t)S * (size_t)(h->d.T - 1) * (size_t)h->d.n_pert; }

// the argument checks of the evaluation's entry points, in the order of the header: those of qc_sweep_eval with the scope and `noise`
int noise_eval_check(qc_sweep* h, const char* who, const double* Z, const double* init, int64_t S, const double* theta, const double* noise,
                     const double* finals, const double* fids) {
    int rc = qc_sweep_check(h, who, &qc_sweep::noise_ok, "qc_sweep noise: ", &qc_sweep::noise_why, Z, init, noise ? nullptr : "noise", S, theta);
    if (rc) return rc;
    const std::string pre = std::string(who) + ": ";
    if (!finals && !fids) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "finals and fids are both NULL");
    if (fids && h->d.fid_kind == QC_SWEEP_FID_NONE) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "fidelities requested from a handle created without one");
    const size_t nn = noise_count(h, S);
    if (overlaps(noise, nn, finals, (size_t)S * h->ns) || overlaps(noise, nn, fids, (size_t)S))
        return qc_sweep_fail(h, QC_ERR_INVALID, pre + "noise overlaps an output");
    return QC_OK;
}

// ... and of the gradient's: those of qc_sweep_grad with both scopes and `noise`
int noise_grad_check(qc_sweep* h, const char* who, const double* Z, const double* init, int64_t S, const double* theta, const double* noise,
                     const double* fids, const double* J, const double* grad, const double* grad_samples, const double* grad_noise) {
    int rc = qc_sweep_check(h, who, &qc_sweep::noise_grad_ok, "qc_sweep noise: ", &qc_sweep::noise_grad_why, Z, init, noise ? nullptr : "noise", S,
                            theta);
    if (rc) return rc;
    const std::string pre = std::string(who) + ": ";
    if (!fids && !J && !grad && !grad_samples && !grad_noise) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "every output is NULL");
    const size_t nn = noise_count(h, S), n_int = (size_t)(h->d.T - 1), nd = (size_t)h->d.m + (h->d.off_dt >= 0 ? 1 : 0);
    if (overlaps(noise, nn, fids, (size_t)S) || overlaps(noise, nn, J, 1) || overlaps(noise, nn, grad, (size_t)h->Zlen) ||
        overlaps(noise, nn, grad_samples, (size_t)S * n_int * nd) || overlaps(noise, nn, grad_noise, nn))
        return qc_sweep_fail(h, QC_ERR_INVALID, pre + "noise overlaps an output");
    return QC_OK;
}

int noise_eval_launch(qc_sweep* h, const char* who, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                      const double* dnoise, double* dfinals, double* dfids, void* stream) {
    int rc = noise_eval_check(h, who, dZ, dinit, S, dtheta, dnoise, dfinals, dfids);
    if (rc) return rc;
    qc_device_guard guard(h->device);
    QC_SIDE_HIP(h, *qc_sweep_err_slot(), guard.err);
    hipStream_t st = (hipStream_t)stream;
    int64_t chunk, n_chunks;
    if ((rc = noise_launch_totals(h, dZ, S, dtheta, dscale, dnoise, st, &chunk, &n_chunks))) return rc;
    return qc_sweep_launch_finish(h, S, n_chunks, dinit, dfinals, dfids, st);
}

int noise_grad_launch(qc_sweep* h, const char* who, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                      const double* dnoise, const double* dweights, double* dfids, double* dJ, double* dgrad, double* dgrad_samples,
                      double* dgrad_noise, void* stream) {
    int rc = noise_grad_check(h, who, dZ, dinit, S, dtheta, dnoise, dfids, dJ, dgrad, dgrad_samples, dgrad_noise);
    if (rc) return rc;
    std::string& slot = *qc_sweep_err_slot();
    qc_device_guard guard(h->device);
    QC_SIDE_HIP(h, slot, guard.err);
    hipStream_t st = (hipStream_t)stream;
    int64_t chunk, n_chunks;
    if ((rc = noise_launch_totals(h, dZ, S, dtheta, dscale, dnoise, st, &chunk, &n_chunks))) return rc;
    const NoiseParams P = noise_params(h, S, chunk, n_chunks);
    const size_t n_state = (size_t)S * n_chunks * h->ns;
    QC_SIDE_HIP(h, slot, h->grow(h->dXs, n_state));
    QC_SIDE_HIP(h, slot, h->grow(h->dLs, n_state));
    if (!dfids) {
        QC_SIDE_HIP(h, slot, h->grow(h->dGfid, (size_t)S));
        dfids = h->dGfid.p;
    }
    const bool want_grad = (dgrad || dgrad_samples) && P.nd > 0;
    double* gsamp = dgrad_samples;
    if (want_grad && !gsamp) {      // the handle's own buffer, as qc_sweep_grad_dev
        QC_SIDE_HIP(h, slot, h->grow(h->dGsamp, (size_t)S * P.n_int * P.nd));
        gsamp = h->dGsamp.p;
    }
    qc_sweep_launch_fid_seed(h, S, n_chunks, dinit, dfids, st);
    if (want_grad || dgrad_noise) {
        const unsigned grid = (unsigned)((P.items + kNWaves - 1) / kNWaves);
        double* gs = want_grad ? gsamp : nullptr;
#define QC_NOISE_GRAD_LAUNCH(M_)                                                                                                         \
    hipLaunchKernelGGL(qc_sweep_noise_grad_kernel<M_>, dim3(grid), dim3(64 * kNWaves), 0, st, P, dZ, dtheta, dscale, dnoise,               \
                       (const double*)h->dXs.p, (const double*)h->dLs.p, gs, dgrad_noise)
        QC_SWEEP_FOR_M(P.m + P.p, QC_NOISE_GRAD_LAUNCH);
#undef QC_NOISE_GRAD_LAUNCH
    }
    qc_sweep_launch_weighted(h, S, gsamp, dweights, dfids, dgrad, dJ, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qc_sweep_fail(h, QC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return QC_OK;
}

}  // namespace

bool qc_sweep_noise_scope(const qc_sweep_desc* d, std::string* why) {
    const int form = qc_sweep_desc_form(d);
    if (form == 2) { *why = "noise trajectories are not served in the mfma32-sweep form"; return false; }
    if (form == 0) { *why = qc_sweep_per_sample_why(d); return false; }
    if (d->n_pert == 0) { *why = "the handle has no perturbations (n_pert = 0): noise enters through the perturbation generators"; return false; }
    if (d->m + d->n_pert > kNTiles) {
        *why = "m + n_pert = " + std::to_string(d->m) + " + " + std::to_string(d->n_pert) + " exceeds the 8 tiles a wavefront keeps in registers";
        return false;
    }
    return true;
}

extern "C" int qc_sweep_desc_noise_supported(const qc_sweep_desc* d, int32_t* supported) {
    int rc = qc_sweep_validate_desc(d);
    if (rc) return rc;
    if (!supported) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep_desc_noise_supported: supported is NULL");
    std::string why;
    const bool ok = qc_sweep_noise_scope(d, &why);
    *supported = ok ? 1 : 0;
    if (!ok) (void)qc_sweep_fail(nullptr, QC_ERR_UNSUPPORTED, "qc_sweep noise: " + why);
    return QC_OK;
}

extern "C" int qc_sweep_noise_eval_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                                       const double* dnoise, double* dfinals, double* dfids, void* stream) {
    return noise_eval_launch(h, "qc_sweep_noise_eval_dev", dZ, dinit, S, dtheta, dscale, dnoise, dfinals, dfids, stream);
}

// The host-buffer entry points: stage, launch on the handle's stream, copy back, synchronise.
extern "C" int qc_sweep_noise_eval(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale,
                                   const double* noise, double* finals, double* fids) {
    const char* who = "qc_sweep_noise_eval";
    int rc = noise_eval_check(h, who, Z, init, S, theta, noise, finals, fids);
    if (rc) return rc;
    const size_t nS = (size_t)S, m = (size_t)h->d.m, p = (size_t)h->d.n_pert, ns = (size_t)h->ns;
    qc_stage stage(h, qc_sweep_err_slot());
    const double* dZ = stage.in(h->sZ, Z, (size_t)h->Zlen);
    const double* dinit = stage.in(h->sInit, init, ns);
    const double* dtheta = stage.in(h->sTheta, theta, nS * p);
    const double* dscale = stage.in(h->sScale, scale, nS * m);
    const double* dnoise = stage.in(h->sNoise, noise, noise_count(h, S));
    double* dfinals = stage.out(h->sFinals, finals, nS * ns);
    double* dfids = stage.out(h->sFids, fids, nS);
    if ((rc = stage.status())) return rc;
    if ((rc = noise_eval_launch(h, who, dZ, dinit, S, dtheta, dscale, dnoise, dfinals, dfids, h->stream))) return rc;
    return stage.finish();
}

extern "C" int qc_sweep_noise_grad_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                                       const double* dnoise, const double* dweights, double* dfids, double* dJ, double* dgrad,
                                       double* dgrad_samples, double* dgrad_noise, void* stream) {
    return noise_grad_launch(h, "qc_sweep_noise_grad_dev", dZ, dinit, S, dtheta, dscale, dnoise, dweights, dfids, dJ, dgrad, dgrad_samples,
                             dgrad_noise, stream);
}

extern "C" int qc_sweep_noise_grad(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale,
                                   const double* noise, const double* weights, double* fids, double* J, double* grad, double* grad_samples,
                                   double* grad_noise) {
    const char* who = "qc_sweep_noise_grad";
    int rc = noise_grad_check(h, who, Z, init, S, theta, noise, fids, J, grad, grad_samples, grad_noise);
    if (rc) return rc;
    const size_t nS = (size_t)S, m = (size_t)h->d.m, p = (size_t)h->d.n_pert, Zlen = (size_t)h->Zlen, nn = noise_count(h, S);
    const size_t n_samp = nS * (size_t)(h->d.T - 1) * (m + (h->d.off_dt >= 0 ? 1 : 0));
    qc_stage stage(h, qc_sweep_err_slot());
    const double* dZ = stage.in(h->sZ, Z, Zlen);
    const double* dinit = stage.in(h->sInit, init, (size_t)h->ns);
    const double* dtheta = stage.in(h->sTheta, theta, nS * p);
    const double* dscale = stage.in(h->sScale, scale, nS * m);
    const double* dnoise = stage.in(h->sNoise, noise, nn);
    const double* dweights = stage.in(h->sW, weights, nS);
    double* dfids = stage.out(h->sFids, fids, nS);
    double* dJ = stage.out(h->sJ, J, 1);
    double* dgrad = stage.out(h->sGrad, grad, Zlen);
    double* dsamp = stage.out(h->sGradS, grad_samples, n_samp);
    double* dgn = stage.out(h->sGnoise, grad_noise, nn);
    if ((rc = stage.status())) return rc;
    if ((rc = noise_grad_launch(h, who, dZ, dinit, S, dtheta, dscale, dnoise, dweights, dfids, dJ, dgrad, dsamp, dgn, h->stream))) return rc;
    return stage.finish();
}
