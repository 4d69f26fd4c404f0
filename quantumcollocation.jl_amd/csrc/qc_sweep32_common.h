// What the forward kernel (qc_sweep32.hip), the backward walks (qc_sweep32_grad.hip, qc_sweep32_open_grad.hip) and the pushforward
// (qc_sweep32_jvp.hip) of the "mfma32-sweep" form share, in one place so that it cannot drift: the closed walk reverses the forward step,
// and the stored states match the stored-state walk, only if all form the same generator and choose the same number of squarings.  The
// sample's base matrix, the interval's generator, the lane's drive and factor, a state in two tiles, the squaring rule, the four-tile
// transpose, the in-place product X <- A X + c I, the plain exponential (called only where that leaves a kernel's registers and time alone);
// constants, table, DPP move, wave sum, rule's tail and work item are those of qc_sweep_common.h.  The counterpart of qc_sweep16_common.h.
#pragma once

#include "qc_sweep_common.h"

namespace qc_sweep32 {

using namespace qc_sweep_common;

constexpr int kScr = 4 * 272;       // doubles of LDS per wave: four transposition tiles

// sample s's base matrix G_drift + sum_q theta[s, q] P_q in A layout (images: 1024 doubles a matrix -- drift, m drives, p perturbations)
__device__ __forceinline__ void base_matrix(const double* __restrict__ img, int m, int p, const double* __restrict__ theta, long long s, int lane,
                                            v4d (&base)[2][2]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) base[q >> 1][q & 1] = load_image_tile(img + q * 256, lane);
    for (int q = 0; q < p; ++q) {
        const double th = theta[s * p + q];
        const double* __restrict__ Pq = img + (size_t)(1 + m + q) * 1024;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const v4d t = load_image_tile(Pq + u * 256, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) base[u >> 1][u & 1][r] = fma(th, t[r], base[u >> 1][u & 1][r]);
        }
    }
}

// G = base + sum_u al_u G_u in A layout; lane u of `al` holds the (scaled) amplitude of drive u.  The drive images are read from the
// image buffer every interval (8 16-byte loads per drive and lane): eight resident drives would be 256 VGPRs.
__device__ __forceinline__ void generator(const double* __restrict__ img, int m, double al, const v4d (&base)[2][2], int lane, v4d (&G)[2][2]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) G[q >> 1][q & 1] = base[q >> 1][q & 1];
#pragma unroll 1
    for (int u = 0; u < m; ++u) {
        const double a = bcast_lane(al, u);
        const double* __restrict__ Gu = img + (size_t)(1 + u) * 1024;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const v4d t4 = load_image_tile(Gu + q * 256, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) G[q >> 1][q & 1][r] = fma(a, t4[r], G[q >> 1][q & 1][r]);
        }
    }
}

// lane l holds the sample's factor of drive kl = min(l, m-1), folded into the control values: cl = scale[s, kl], 1 without `scale`
struct DriveLane {
    int kl;
    double cl;
};

__device__ __forceinline__ DriveLane drive_lane(const double* scale, int m, long long s, int lane) {
    DriveLane d;
    d.kl = lane < m ? lane : (m > 0 ? m - 1 : 0);
    d.cl = (scale && m > 0) ? scale[s * m + d.kl] : 1.0;
    return d;
}

// an n x nc column-major state at `p` into two D-layout tiles (rows 16 I + 4 r + g, column j), zero outside n x nc
__device__ __forceinline__ void load_state(const double* p, int n, int nc, int g, int j, v4d (&x)[2]) {
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * I + 4 * r + g;
            x[I][r] = (row < n && j < nc) ? p[row + n * j] : 0.0;
        }
}

// The number of squarings, wave-uniform: the smallest sq with ||h G||_1 / 2^sq <= 1/8 (0 for a non-finite norm).  ||h G||_1 is the
// largest column sum: tile (I, K), lane (g, i), reg kk holds G[16 I + i][16 K + 4 kk + g]; the two tile rows and the 16 lanes of a row
// share a column.
__device__ __forceinline__ int squarings(const v4d (&G)[2][2], double h) {
    double best = 0.0;
    bool bad = false;
#pragma unroll
    for (int K = 0; K < 2; ++K) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const double cs = row_sum(fabs(h * G[0][K][kk]) + fabs(h * G[1][K][kk]));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = bcast_lane(cs, 16 * r);
                if (!(v == v) || v > 1e300) bad = true;
                best = fmax(best, v);
            }
        }
    }
    return squarings_of_norm(best, bad);
}

// the four tiles of a D-layout matrix, each transposed: the matrix in A layout (one LDS round trip)
__device__ __forceinline__ void transpose4(double* __restrict__ scr, const v4d (&X)[2][2], v4d (&Xt)[2][2], int g, int j) {
    const v4d in[4] = {X[0][0], X[0][1], X[1][0], X[1][1]};
    v4d out[4];
    lds_transpose16_multi<4>(scr, in, out, g, j);
    Xt[0][0] = out[0]; Xt[0][1] = out[1]; Xt[1][0] = out[2]; Xt[1][1] = out[3];
}

// column J of  X <- A X + c I  in place (A in A layout, X in B / D layout): two independent chains of 8 MFMAs
__device__ __forceinline__ void wcol(const v4d (&A)[2][2], v4d (&X)[2][2], int J, const v4d& c0, const v4d& c1) {
    v4d n0 = c0, n1 = c1;
#pragma unroll
    for (int K = 0; K < 2; ++K) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            n0 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[0][K][kk], X[K][J][kk], n0, 0, 0, 0);
            n1 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[1][K][kk], X[K][J][kk], n1, 0, 0, 0);
        }
    }
    X[0][J] = n0;
    X[1][J] = n1;
}

// X <- A X + c I, c I given as its diagonal tile
__device__ __forceinline__ void wmul(const v4d (&A)[2][2], v4d (&X)[2][2], const v4d& cI) {
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    wcol(A, X, 0, cI, zero);
    wcol(A, X, 1, zero, cI);
}

// where every Horner chain of the form starts: R = I / deg!   (IdB: the identity's diagonal tile, identity_B(g, j))
__device__ __forceinline__ void horner_top(const v4d& IdB, v4d (&R)[2][2]) {
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    R[0][0] = kInvFact[kDeg] * IdB; R[0][1] = zero; R[1][0] = zero; R[1][1] = kInvFact[kDeg] * IdB;
}

// R = exp(hs 2^sq Y) in D layout from the generator Y in A layout (destroyed: it holds the transposed E of the last squaring).
// Y <- hs Y;  Horner: R_deg+1 = I/deg!,  R_k = Y R_k+1 + I/(k-1)!  (the last coefficient is exactly 1: a zero generator gives the
// identity bits);  sq squarings, E as the left factor through one LDS round trip each.
__device__ __forceinline__ void exp_plain(double* scr, v4d (&Y)[2][2], double hs, int sq, const v4d& IdB, int g, int j,
                                          v4d (&R)[2][2]) {
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; ++q) Y[q >> 1][q & 1] = hs * Y[q >> 1][q & 1];
    horner_top(IdB, R);
#pragma unroll 1
    for (int k = kDeg; k >= 1; --k) wmul(Y, R, kInvFact[k - 1] * IdB);
    for (int q = 0; q < sq; ++q) {
        transpose4(scr, R, Y, g, j);          // E in A layout; Y is free from here on
        wmul(Y, R, zero);
    }
}

}  // namespace qc_sweep32
