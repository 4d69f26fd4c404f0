// Noise-trajectory sweeps for "mfma32-sweep" handles (16 < 2N <= 32) whose `wide` has QC_SWEEP_WIDE_NOISE: the two kernels of
// qc_sweep_noise.hip (read its header first: the model, the lane map, the zero-noise contract, grad_noise) with every matrix 2 x 2 tiles of
// 16 x 16.  In interval t of sample s
//     G_{s,t} = G_drift + sum_j (theta[s,j] + xi[s,t,j]) P_j + sum_k c[s,k] a_{t,k} G_k.
// The wide kernels keep no drive tiles in registers: qc_sweep32::generator reads the images 1 .. m again every interval, and the
// perturbation images follow the drives in the image buffer.  A per-interval perturbation is therefore a longer loop bound, mt = m + p,
// and a per-lane coefficient source; there is no template parameter and no tile limit (m <= 8, p <= QC_MAX_PERT: up to 16 generators).
//   * lane l < m reads control l of knot t of Z and multiplies it by c[s,l]; lane m + j reads noise[(s (T-1) + t) p + j], factor 1; lanes
//     past mt repeat lane mt - 1 (p >= 1: there always is one).  Each lane carries its own pointer and stride (zdim or p) in vector
//     registers and steps it per interval, as `gp` walks in qc_sweep32_grad_kernel<true>: one load per lane and interval, requested one
//     interval ahead;
//   * base_matrix folds theta; generator(img, mt, al, ...) adds the drives in ascending k, THEN the perturbations in ascending j.  At
//     xi = +0.0 the extra fmas leave every value as it was (a -0 may become +0, nothing else);
//   * everything after the generator is qc_sweep_mfma32_kernel's / qc_sweep32_grad_kernel<false>'s: the chunk totals go to h->dTot
//     (S x n_chunks x 1024) and qc_sweep_finish_kernel follows; the gradient runs the seed, the walk below and the reductions unchanged.
// The walk's contraction sum ZT . G_u runs over u < mt; lane u keeps du * cl (a perturbation lane's factor is 1), lane mt the timestep's
// value.  Every lane that has a value carries the address it belongs to: lanes 0 .. m-1 and lane mt walk down grad_samples in the
// gradient's layout, lanes m .. mt-1 walk down grad_noise; one vector store per interval with per-lane addresses serves both buffers
// (a lane whose buffer is absent keeps a null address and stride 0).  No atomics, sums in a fixed order; which buffers are present
// changes which lanes store, never what they hold.
// MFMAs per interval: 288 + 32 sq forward, 848 + 96 sq backward, as without noise; p more image reads (8 loads a lane) and 16 p fmas per
// interval, and p more wave sums in the walk.
// gfx950 cross-compile: see the table in DESIGN.md 5.8.9; no private segment, no spills in either kernel.
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_sweep32_common.h"
#include "qc_sweep32_walk.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep32;

// Where lane l finds the coefficient of generator min(l, mt - 1) in interval t, how far the next interval's lies, and the sample's factor.
struct LaneCoef {
    const double* cp;
    int stride;          // doubles from one interval to the next: zdim for a drive lane, p for a perturbation lane
    double cl;           // c[s,k] for a drive lane, 1 for a perturbation lane
};

__device__ __forceinline__ LaneCoef lane_coef(const SweepParams& P, int lane, long long s, int t, const double* __restrict__ Z,
                                              const double* __restrict__ scale, const double* __restrict__ noise) {
    const int m = P.m, mt = m + P.p;
    const int kl = lane < mt ? lane : mt - 1;
    const bool drv = kl < m;
    LaneCoef c;
    c.cp = drv ? Z + (long long)t * P.zdim + P.off_a + kl : noise + (s * P.n_int + t) * (long long)P.p + (kl - m);
    c.stride = drv ? P.zdim : P.p;
    c.cl = (scale && drv) ? scale[s * m + kl] : 1.0;
    return c;
}

// Launch 1: the chunk totals.  Restates qc_sweep_mfma32_kernel (qc_sweep32.hip; to be changed with it, exp_plain included) with mt generators.
__global__ __launch_bounds__(64 * kWaves, 2) void qc_sweep32_noise_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                            const double* __restrict__ theta, const double* __restrict__ scale,
                                                                            const double* __restrict__ noise, double* __restrict__ tot) {
    __shared__ double scr_all[kWaves * kScr];
    const WaveItem w = wave_item(kWaves);
    double* __restrict__ scr = scr_all + w.wq * kScr;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m, mt = m + P.p;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    // ---- once per wave: the sample's base matrix, the lane's coefficient source ----------------------------------------------------
    v4d base[2][2];
    base_matrix(P.img, m, P.p, theta, s, lane, base);
    const LaneCoef lc = lane_coef(P, lane, s, t0, Z, scale, noise);
    const double* cp = lc.cp;

    const double* __restrict__ z = Z + (long long)t0 * P.zdim;
    double av = *cp;
    const double hfix = opaque_scalar(P.dt_fixed);      // keeps the two arms apart: no flat load (qc_mfma_common.h)
    double h = ft ? z[P.off_dt] : hfix;
    v4d W[2][2] = {{IdB, zero}, {zero, IdB}};
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        // the next interval's coefficients and timestep are requested before this interval's products
        const double* __restrict__ zn = Z + (long long)(t + 1 < t1 ? t + 1 : t) * P.zdim;
        if (t + 1 < t1) cp += lc.stride;
        const double av_n = *cp;
        const double h_n = ft ? zn[P.off_dt] : hfix;
        const double al = av * lc.cl;
        v4d Y[2][2];
        generator(P.img, mt, al, base, lane, Y);
        const int sq = squarings(Y, h);
        const double hs = h * ldexp(1.0, -sq);
#pragma unroll
        for (int q = 0; q < 4; ++q) Y[q >> 1][q & 1] = hs * Y[q >> 1][q & 1];
        v4d R[2][2] = {{kInvFact[kDeg] * IdB, zero}, {zero, kInvFact[kDeg] * IdB}};
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) wmul(Y, R, kInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            transpose4(scr, R, Y, g, j);          // E in A layout; Y is free from here on
            wmul(Y, R, zero);
        }
        transpose4(scr, R, Y, g, j);
        wmul(Y, W, zero);
        av = av_n;
        h = h_n;
    }
    // column-major 32 x 32: entry (16 I + 4 r + g, 16 J + j)
    double* __restrict__ o = tot + item * 1024;
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int J = 0; J < 2; ++J)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[(16 * J + j) * 32 + 16 * I + 4 * r + g] = W[I][J][r];
}

// Launch 3: the backward walk: qc_sweep32_grad_kernel<false> with mt generators, on load_state, outer_kt, dot_tiles and contract_image.  The
// paired chain and ZT restate exp_pair and qc_sweep32_grad_kernel: the calls move this kernel's registers ("Shared and restated in the wide kernels").
// gs (S x (T-1) x nd) and gn (S x (T-1) x p) may each be NULL, not both.
__global__ __launch_bounds__(64 * kWaves) void qc_sweep32_noise_grad_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                             const double* __restrict__ theta, const double* __restrict__ scale,
                                                                             const double* __restrict__ noise, const double* __restrict__ xs,
                                                                             const double* __restrict__ ls, double* __restrict__ gs,
                                                                             double* __restrict__ gn) {
    __shared__ double scr_all[kWaves * kScr];
    const WaveItem w = wave_item(kWaves);
    double* __restrict__ scr = scr_all + w.wq * kScr;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m, mt = m + P.p;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    // ---- once per wave: the sample's base matrix, the state and the adjoint at the chunk's end, the lane's source and destination -------
    v4d base[2][2];
    base_matrix(P.img, m, P.p, theta, s, lane, base);
    const LaneCoef lc = lane_coef(P, lane, s, t1 - 1, Z, scale, noise);
    const double* cp = lc.cp;
    int cstr = lc.stride;
    const double cl = lc.cl;
    // where the lane's value of interval t1 - 1 goes, and how far the previous interval's lies: lanes 0 .. m-1 (the drives) and lane mt
    // (the timestep, free timesteps only) in gs, lanes m .. mt-1 in gn; a lane without a value, or whose buffer is absent: null, stride 0
    double* op = nullptr;
    int ostr = 0;
    {
        const long long it = s * P.n_int + (t1 - 1);
        if (gs && (lane < m || (ft && lane == mt))) {
            op = gs + it * P.nd + (lane < m ? lane : m);
            ostr = P.nd;
        } else if (gn && lane >= m && lane < mt) {
            op = gn + it * P.p + (lane - m);
            ostr = P.p;
        }
    }
    // the loop has no scalar register to spare (qc_sweep32_grad_kernel): what is per lane stays in vector registers
    asm volatile("" : "+v"(cp), "+v"(cstr), "+v"(op), "+v"(ostr));

    v4d x[2], lam[2];
    load_state(xs + item * (P.n * P.nc), P.n, P.nc, g, j, x);
    load_state(ls + item * (P.n * P.nc), P.n, P.nc, g, j, lam);

    const double hfix = opaque_scalar(P.dt_fixed);
    const double* __restrict__ z = Z + (long long)(t1 - 1) * P.zdim;
    double av = *cp;
    double h = ft ? z[P.off_dt] : hfix;
#pragma unroll 1
    for (int t = t1 - 1; t >= t0; --t) {
        // the previous interval's coefficients and timestep are requested before this interval's products
        const double* __restrict__ zn = Z + (long long)(t > t0 ? t - 1 : t) * P.zdim;
        if (t > t0) cp -= cstr;
        const double av_n = *cp;
        const double h_n = ft ? zn[P.off_dt] : hfix;
        const double al = av * cl;
        v4d Y[2][2], dY[2][2];
        generator(P.img, mt, al, base, lane, Y);
        const int sq = squarings(Y, h);      // the rule of the forward kernel: one function
        const double hs = h * ldexp(1.0, -sq);
        outer_kt(scr, x, lam, g, j, dY);      // KT = lambda x^T of knot t+1
        // an opaque copy of the lane index: the lane compares below are made per interval instead of living in scalar registers across
        // the loop (as in qc_sweep32_grad_kernel)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        double out = 0.0;      // lane u < mt: generator u (the drives, then the noise values); lane mt: the timestep (free timesteps)
        if (ft) {
            const double dh = -wave_sum(dot_tiles(dY, Y, 0.0));      // sum_IJ KT[I][J] . Ga[J][I] = sum_IK dY(I, K) . Ga(I, K)
            out = ln == mt ? dh : out;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            Y[q >> 1][q & 1] = hs * Y[q >> 1][q & 1];
            dY[q >> 1][q & 1] = hs * dY[q >> 1][q & 1];
        }
        v4d R[2][2] = {{kInvFact[kDeg] * IdB, zero}, {zero, kInvFact[kDeg] * IdB}};
        v4d dR[2][2] = {{zero, zero}, {zero, zero}};
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) vstep(Y, dY, R, dR, kInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            transpose4(scr, R, Y, g, j);           // E, dE in A layout; Y, dY are free from here on
            transpose4(scr, dR, dY, g, j);
            vstep(Y, dY, R, dR, zero);
        }
        // ZT = E^T dE, into Y
#pragma unroll
        for (int J = 0; J < 2; ++J) {
            v4d z0 = zero, z1 = zero;
#pragma unroll
            for (int K = 0; K < 2; ++K) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    z0 = __builtin_amdgcn_mfma_f64_16x16x4f64(R[K][0][kk], dR[K][J][kk], z0, 0, 0, 0);
                    z1 = __builtin_amdgcn_mfma_f64_16x16x4f64(R[K][1][kk], dR[K][J][kk], z1, 0, 0, 0);
                }
            }
            Y[0][J] = z0;
            Y[1][J] = z1;
        }
#pragma unroll 1
        for (int u = 0; u < mt; ++u) {
            const double du = contract_image(Y, P.img + (size_t)(1 + u) * 1024, lane);
            out = ln == u ? du * cl : out;      // a perturbation lane's factor is 1
        }
        if (op) *op = out;
        op -= ostr;
        vapplyT(R, x);
        vapplyT(R, lam);
        av = av_n;
        h = h_n;
    }
}

}  // namespace

int qc_sweep32_noise_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dnoise,
                                   hipStream_t st, int64_t* chunk_out, int64_t* n_chunks_out) {
    SweepParams P;
    if (int rc = qc_sweep_plan_totals(h, S, h->dTot, 1024, &P, chunk_out, n_chunks_out)) return rc;
    hipLaunchKernelGGL(qc_sweep32_noise_kernel, dim3(qc_sweep_grid(P, kWaves)), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale, dnoise, h->dTot.p);
    return QC_OK;
}

void qc_sweep32_noise_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dnoise,
                                  int64_t chunk, int64_t n_chunks, double* gs, double* gn, hipStream_t st) {
    const SweepParams P = qc_sweep_params(h, S, chunk, n_chunks);
    const unsigned grid = qc_sweep_grid(P, kWaves);
    hipLaunchKernelGGL(qc_sweep32_noise_grad_kernel, dim3(grid), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale, dnoise,
                       (const double*)h->dXs.p, (const double*)h->dLs.p, gs, gn);
}
