// What the kernels of the "mfma16-sweep" form share (2N <= 16: every matrix one 16 x 16 tile in registers; lane maps: qc_mfma_kernels.hip
// header): the forward kernel of qc_sweep.hip, the walks of qc_sweep_grad.hip and qc_sweep_open_grad.hip, the pushforward of
// qc_sweep_jvp.hip, the Hessian product of qc_sweep_hvp.hip and the noise kernels of qc_sweep_noise.hip.  The image-tile load, the
// sample's base tile, the interval's generator, the squaring rule, the single-accumulator product, the paired Horner / squaring step and
// the LDS slices; constants, table, DPP move, wave sum and the rule's tail are those of qc_sweep_common.h.  The counterpart of
// qc_sweep32_common.h.  Device code only.
#pragma once

#include "qc_sweep_common.h"

namespace qc_sweep16 {

using namespace qc_sweep_common;

constexpr int kTile = 16 * 17;      // doubles of LDS of one transposition tile (lds_transpose16: rows padded to 17)
// LDS of one wave of a backward walk: two transposition tiles, and in the parameter flavour behind them the accumulator tile sum_t ZT_t
// (256), the interval's unscaled controls (64) and the scale accumulator (64)
template <bool PAR>
constexpr int kWalkSlice = 2 * kTile + (PAR ? 256 + 128 : 0);

// tile `mat` of the A-layout images [matrix][kk][lane]: drift, m drives, p perturbations
__device__ __forceinline__ v4d image_tile(const double* __restrict__ img, int mat, int lane) {
    const double* p = img + (size_t)mat * 256 + lane;
    return v4d{p[0], p[64], p[128], p[192]};
}

// sample s's base tile G_drift + sum_q theta[s, q] P_q in A layout
__device__ __forceinline__ v4d base_tile(const double* __restrict__ img, int m, int p, const double* __restrict__ theta, long long s, int lane) {
    v4d base = image_tile(img, 0, lane);
    for (int q = 0; q < p; ++q) {
        const double th = theta[s * p + q];
        const v4d Pq = image_tile(img, 1 + m + q, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) base[r] = fma(th, Pq[r], base[r]);
    }
    return base;
}

// ... and beside it its tangent sum_q vtheta[s, q] P_q (vtheta NULL: zeros, through the same arithmetic)
__device__ __forceinline__ void base_tile(const double* __restrict__ img, int m, int p, const double* __restrict__ theta,
                                          const double* __restrict__ vtheta, long long s, int lane, v4d& base, v4d& based) {
    base = image_tile(img, 0, lane);
    based = v4d{0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < p; ++q) {
        const double th = theta[s * p + q];
        const double vth = vtheta ? vtheta[s * p + q] : 0.0;
        const v4d Pq = image_tile(img, 1 + m + q, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            base[r] = fma(th, Pq[r], base[r]);
            based[r] = fma(vth, Pq[r], based[r]);
        }
    }
}

// the tiles a wave keeps in registers: matrices 1 .. mt of the images (the drives; in the noise kernels the perturbations behind them)
template <int M>
__device__ __forceinline__ void resident_tiles(const double* __restrict__ img, int mt, int lane, v4d (&Gj)[M]) {
#pragma unroll
    for (int u = 0; u < M; ++u) Gj[u] = u < mt ? image_tile(img, 1 + u, lane) : v4d{0.0, 0.0, 0.0, 0.0};
}

// the interval's generator Ga = base + sum_u al_u G_u in A layout; lane u of `al` holds the (scaled) amplitude of tile u < mt
template <int M>
__device__ __forceinline__ v4d generator(const v4d& base, const v4d (&Gj)[M], int mt, double al) {
    v4d Ga = base;
#pragma unroll
    for (int u = 0; u < M; ++u) {
        const double a = u < mt ? bcast_lane(al, u) : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) Ga[r] = fma(a, Gj[u][r], Ga[r]);
    }
    return Ga;
}

// ... and beside it its tangent Gad = based + sum_u ald_u G_u
template <int M>
__device__ __forceinline__ void generator(const v4d& base, const v4d& based, const v4d (&Gj)[M], int mt, double al, double ald, v4d& Ga, v4d& Gad) {
    Ga = base;
    Gad = based;
#pragma unroll
    for (int u = 0; u < M; ++u) {
        const double a = u < mt ? bcast_lane(al, u) : 0.0;
        const double ad = u < mt ? bcast_lane(ald, u) : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Ga[r] = fma(a, Gj[u][r], Ga[r]);
            Gad[r] = fma(ad, Gj[u][r], Gad[r]);
        }
    }
}

// The number of squarings of an interval, wave-uniform.  ||h G||_1 = the largest column sum of the A-layout tile Ga (lane (g, i) reg kk
// holds G[i][4kk+g]: rows of 16 lanes share a column).  No tangent ever enters it.
__device__ __forceinline__ int squarings(double h, const v4d& Ga) {
    double best = 0.0;
    bool bad = false;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const double cs = row_sum(fabs(h * Ga[kk]));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double v = bcast_lane(cs, 16 * r);
            if (!(v == v) || v > 1e300) bad = true;
            best = fmax(best, v);
        }
    }
    return squarings_of_norm(best, bad);
}

// D = A B + C with one accumulator: the four MFMAs of a Horner step or a squaring
__device__ __forceinline__ v4d mma16(const v4d& a, const v4d& b, v4d acc) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], b[kk], acc, 0, 0, 0);
    return acc;
}

// (R, dR) <- (A R + C,  dA R + A dR): a Horner step (A = Y, dA = dY, C = I / (k-1)!) or a squaring (A = E, dA = dE, C = 0).  The R chain
// is mma16's, operation for operation.  Three independent accumulator chains, interleaved.
__device__ __forceinline__ void step16(const v4d& A, const v4d& dA, v4d& R, v4d& dR, const v4d& C) {
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

}  // namespace qc_sweep16
