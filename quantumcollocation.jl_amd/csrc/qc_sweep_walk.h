// What the backward walks of the "mfma16-sweep" form agree on: the closed walk of qc_sweep_grad.hip (qc_sweep_grad_kernel, which reverses
// the forward step) and the stored-state walk of qc_sweep_open_grad.hip (qc_sweep_open_grad_kernel, which reads the forward states).  The
// degree-8 series and its 1 / k! table, the ||Y||_1 <= 1/8 squaring rule, the launch parameters, the paired Horner / squaring step, the
// fixed-order wave sum and the LDS slice of a wave.  A walk of the "mfma32-sweep" form that reads stored states takes the same rule, table
// and step order, on 2 x 2 tiles.  Device code only; every translation unit gets its own copy of the table (a __constant__ is private to
// its translation unit).
#pragma once

#include "qc_mfma_common.h"

namespace qc_sweep_walk {

using namespace qc_mfma;

constexpr int kGDeg = 8;            // as the forward kernel (kSDeg, kSTh of qc_sweep.hip)
constexpr double kGTh = 0.125;
constexpr int kGWaves = 4;          // (sample, chunk) items per workgroup: one wave each, the waves never synchronise

// 1 / k!, k = 0 .. 8: the values of kSInvFact (qc_sweep.hip)
__constant__ const double kGInvFact[kGDeg + 1] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0};

struct GradParams {
    int n, nc, m, p, zdim, off_a, off_dt, n_int, chunk, n_chunks, nd;   // nd = m + (off_dt >= 0): derivatives per interval
    long long items;             // S * n_chunks
    double dt_fixed;
    const double* img;           // A-layout images [matrix][kk][lane]: drift, m drives, p perturbations
};

template <int CTRL>
__device__ inline double gdpp(double x) {
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ inline v4d gimg(const double* __restrict__ img, int mat, int lane) {
    const double* p = img + (size_t)mat * 256 + lane;
    return v4d{p[0], p[64], p[128], p[192]};
}

__device__ __forceinline__ v4d gmma(const v4d& a, const v4d& b, v4d acc) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], b[kk], acc, 0, 0, 0);
    return acc;
}

// (R, dR) <- (A R + C,  dA R + A dR): a Horner step (A = Y, dA = dY, C = I / (k-1)!) or a squaring (A = E, dA = dE, C = 0).
// Three independent accumulator chains, interleaved.
__device__ __forceinline__ void gstep(const v4d& A, const v4d& dA, v4d& R, v4d& dR, const v4d& C) {
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

// the sum over the 64 lanes in a fixed order, wave-uniform: row sums by DPP rotations, then (row 0 + row 1) + (row 2 + row 3)
__device__ inline double wave_sum(double v) {
    v += gdpp<0x128>(v);
    v += gdpp<0x124>(v);
    v += gdpp<0x122>(v);
    v += gdpp<0x121>(v);
    return (bcast_lane(v, 0) + bcast_lane(v, 16)) + (bcast_lane(v, 32) + bcast_lane(v, 48));
}

// The number of squarings of an interval, wave-uniform: the rule of the forward kernel.  ||h G||_1 = the largest column sum of the
// A-layout tile Ga (lane (g, i) reg kk holds G[i][4kk+g]: rows of 16 lanes share a column); the smallest sq with ||h G||_1 / 2^sq <= 1/8,
// 0 when the norm is not finite.
__device__ __forceinline__ int squarings(double h, const v4d& Ga) {
    int sq = 0;
    double best = 0.0;
    bool bad = false;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        double cs = fabs(h * Ga[kk]);
        cs += gdpp<0x128>(cs);
        cs += gdpp<0x124>(cs);
        cs += gdpp<0x122>(cs);
        cs += gdpp<0x121>(cs);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double v = bcast_lane(cs, 16 * r);
            if (!(v == v) || v > 1e300) bad = true;
            best = fmax(best, v);
        }
    }
    if (!bad && best > kGTh) {
        int e;
        (void)frexp(best / kGTh, &e);
        sq = e;
        if (ldexp(kGTh, e - 1) >= best) sq = e - 1;
        sq = sq < 0 ? 0 : (sq > 60 ? 60 : sq);
    }
    return __builtin_amdgcn_readfirstlane(sq);
}

// LDS of one wave: two transposition tiles, and in the parameter flavour behind them the accumulator tile sum_t ZT_t (256), the
// interval's unscaled controls (64) and the scale accumulator (64)
template <bool PAR>
constexpr int kGSlice = 2 * 272 + (PAR ? 256 + 128 : 0);

}  // namespace qc_sweep_walk
