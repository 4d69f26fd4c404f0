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
// "mfma32-sweep" handles whose descriptor sets QC_SWEEP_WIDE_NOISE are routed to the two kernels of qc_sweep32_noise.hip (the same lane
// map on 2 x 2 tiles; nothing is resident there, so no tile limit); the checks, the staging and the entry points below are shared.
// "mfma64-sweep" handles whose descriptor sets QC_SWEEP_WIDE_64_NOISE are routed to the two kernels of qc_sweep64_noise.hip (4 x 4 tiles in
// LDS, one workgroup per item; up to 16 + 8 generators), the gradient only with QC_SWEEP_WIDE_64_GRAD as well; the same shared parts.
//
// Out of scope: "mfma32-sweep" / "mfma64-sweep" handles without their bit and "rollout-per-sample" handles, pullbacks / pushforwards / Hessian products with noise, several devices.
//
// gfx950 cross-compile: see the table in DESIGN.md ("Noise-trajectory sweeps"); no private segment, no spills in any instantiation.
#include <math.h>
#include <stdint.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_sweep16_common.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep16;         // the forward kernel's and the closed walk's pieces: both kernels here are theirs with m + p tiles

constexpr int kNTiles = 8;          // tiles a wave keeps in registers: drives and perturbations together

// Where lane l finds the coefficient of tile min(l, m + p - 1).  Drive lanes read the shared controls of knot t of Z, perturbation
// lanes the sample's own noise of interval t; lanes past the last tile repeat the last one (p >= 1: there always is one).
struct LaneCoef {
    int off;             // inside the knot (off_a + k), or inside the interval's noise values (j)
    bool drv;
    double cl;           // c[s,k] for a drive lane, 1 for a perturbation lane
};

__device__ __forceinline__ LaneCoef lane_coef(const SweepParams& P, int lane, long long s, const double* __restrict__ scale) {
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
__global__ __launch_bounds__(64 * kWaves, 2) void qc_sweep_noise_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                          const double* __restrict__ theta, const double* __restrict__ scale,
                                                                          const double* __restrict__ noise, double* __restrict__ tot) {
    __shared__ double scr_all[kWaves * kTile];
    const WaveItem w = wave_item(kWaves);
    double* __restrict__ scr = scr_all + w.wq * kTile;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m, mt = m + P.p;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    // ---- once per wave: the sample's base tile, the drive and perturbation tiles --------------------------------------------
    const v4d base = base_tile(P.img, m, P.p, theta, s, lane);
    v4d Gj[M];      // the images follow one another: tile u is matrix 1 + u, drives then perturbations
    resident_tiles(P.img, mt, lane, Gj);
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
        const v4d Ga = generator(base, Gj, mt, al);
        const int sq = squarings(h, Ga);
        const double sc = ldexp(1.0, -sq);
        const v4d Y = (h * sc) * Ga;
        v4d R = kInvFact[kDeg] * IdB;
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) R = mma16(Y, R, kInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            const v4d Et = lds_transpose16(scr, R, g, j);
            R = mma16(Et, R, zero);
        }
        const v4d Et = lds_transpose16(scr, R, g, j);     // E^T in D layout = E in A layout
        W = mma16(Et, W, zero);
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
__global__ __launch_bounds__(64 * kWaves, 2) void qc_sweep_noise_grad_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                               const double* __restrict__ theta, const double* __restrict__ scale,
                                                                               const double* __restrict__ noise, const double* __restrict__ xs,
                                                                               const double* __restrict__ ls, double* __restrict__ gs,
                                                                               double* __restrict__ gn) {
    __shared__ double scr_all[kWaves * kWalkSlice<false>];
    const WaveItem w = wave_item(kWaves);
    double* __restrict__ scr = scr_all + w.wq * kWalkSlice<false>;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m, mt = m + P.p;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    const v4d base = base_tile(P.img, m, P.p, theta, s, lane);
    v4d Gj[M];
    resident_tiles(P.img, mt, lane, Gj);
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
        v4d Ga = base;      // qc_sweep16::generator written out: through the call <6> spills two scalar registers
#pragma unroll
        for (int u = 0; u < M; ++u) {
            const double a = u < mt ? bcast_lane(al, u) : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) Ga[r] = fma(a, Gj[u][r], Ga[r]);
        }
        const int sq = squarings(h, Ga);
        const double hs = h * ldexp(1.0, -sq);
        // K^T = lambda x^T of knot t+1 (D layout) from the A-layout forms of both
        v4d KT;
        {
            const v4d in[2] = {x, lam};
            v4d tr[2];
            lds_transpose16_multi<2>(scr, in, tr, g, j);
            KT = mma16(tr[1], tr[0], zero);
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
            const double dh = -wave_sum(ph);
            out = ln == mt ? dh : out;
        }
        const v4d Y = hs * Ga;
        const v4d dY = hs * KT;
        v4d R = kInvFact[kDeg] * IdB;
        v4d dR = zero;
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) step16(Y, dY, R, dR, kInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            const v4d in[2] = {R, dR};
            v4d tr[2];
            lds_transpose16_multi<2>(scr, in, tr, g, j);      // E^T, dE^T in D layout = E, dE in A layout
            step16(tr[0], tr[1], R, dR, zero);
        }
        const v4d ZT = mma16(R, dR, zero);                       // E^T dE
#pragma unroll
        for (int u = 0; u < M; ++u) {
            if (u < mt) {
                double pu = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) pu = fma(ZT[r], Gj[u][r], pu);
                const double du = wave_sum(pu);
                out = ln == u ? du * lc.cl : out;      // a perturbation lane's factor is 1
            }
        }
        const long long it = s * P.n_int + t;
        if (gs && (ln < m || (ft && ln == mt))) gs[it * P.nd + (ln < m ? ln : m)] = out;
        if (gn && ln >= m && ln < mt) gn[it * P.p + (ln - m)] = out;
        x = mma16(R, x, zero);
        lam = mma16(R, lam, zero);
        av = av_n;
        h = h_n;
    }
}

// launch 1: grows h->dTot and launches qc_sweep_noise_kernel<M> (S x n_chunks tiles of 256 doubles, the layout of qc_sweep_launch_totals)
int noise_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dnoise, hipStream_t st,
                        int64_t* chunk_out, int64_t* n_chunks_out) {
    if (h->wide_noise) return qc_sweep32_noise_launch_totals(h, dZ, S, dtheta, dscale, dnoise, st, chunk_out, n_chunks_out);      // the only mfma32 handles in scope
    if (h->wide64_noise) return qc_sweep64_noise_launch_totals(h, dZ, S, dtheta, dscale, dnoise, st, chunk_out, n_chunks_out);    // the only mfma64 handles in scope
    SweepParams P;
    if (int rc = qc_sweep_plan_totals(h, S, h->dTot, 256, &P, chunk_out, n_chunks_out)) return rc;
#define QC_NOISE_LAUNCH(M_) \
    hipLaunchKernelGGL(qc_sweep_noise_kernel<M_>, dim3(qc_sweep_grid(P, kWaves)), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale, dnoise, h->dTot.p)
    QC_SWEEP_FOR_M(P.m + P.p, QC_NOISE_LAUNCH);
#undef QC_NOISE_LAUNCH
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
    const SweepParams P = qc_sweep_params(h, S, chunk, n_chunks);
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
    if ((want_grad || dgrad_noise) && h->wide_noise) {
        qc_sweep32_noise_launch_walk(h, dZ, S, dtheta, dscale, dnoise, chunk, n_chunks, want_grad ? gsamp : nullptr, dgrad_noise, st);
    } else if ((want_grad || dgrad_noise) && h->wide64_noise) {
        if ((rc = qc_sweep64_noise_launch_walk(h, dZ, S, dtheta, dscale, dnoise, chunk, n_chunks, want_grad ? gsamp : nullptr, dgrad_noise, st))) return rc;
    } else if (want_grad || dgrad_noise) {
        const unsigned grid = qc_sweep_grid(P, kWaves);
        double* gs = want_grad ? gsamp : nullptr;
#define QC_NOISE_GRAD_LAUNCH(M_)                                                                                                         \
    hipLaunchKernelGGL(qc_sweep_noise_grad_kernel<M_>, dim3(grid), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale, dnoise,               \
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
    const qc_sweep_form form = qc_sweep_desc_form(d);
    if (form == QC_SWEEP_FORM_32 && !(d->wide & QC_SWEEP_WIDE_NOISE)) { *why = "noise trajectories are not served in the mfma32-sweep form"; return false; }
    if (form == QC_SWEEP_FORM_PER_SAMPLE) { *why = qc_sweep_per_sample_why(d); return false; }
    if (form == QC_SWEEP_FORM_64 && !(d->wide & QC_SWEEP_WIDE_64_NOISE)) { *why = qc_sweep_form64_unserved(d, "noise trajectories"); return false; }
    if (d->n_pert == 0) { *why = "the handle has no perturbations (n_pert = 0): noise enters through the perturbation generators"; return false; }
    if (form == QC_SWEEP_FORM_16 && d->m + d->n_pert > kNTiles) {      // the wide forms keep no tile resident: m <= 8 (mfma64-sweep: 16) and n_pert <= QC_MAX_PERT, up to 16 (24) generators
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
