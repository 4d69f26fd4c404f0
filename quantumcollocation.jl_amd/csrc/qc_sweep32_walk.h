// What the backward walks and the pushforward of the "mfma32-sweep" form share (the closed walks of qc_sweep32_grad.hip and
// qc_sweep32_noise.hip, the stored-state walk of qc_sweep32_open_grad.hip, qc_sweep32_jvp.hip, qc_sweep32_hvp.hip): the paired column step
// of the Horner / squaring chains, the paired chain itself (exp_pair), KT, the elementwise product behind the timestep derivative, the
// contraction with a generator's image and the product with E^T; constants, generator and squaring rule are those of qc_sweep32_common.h.
// A kernel calls a piece only where that leaves its registers and its time where they were ("Shared and restated in the wide kernels").
#pragma once
#include "qc_sweep32_common.h"

namespace qc_sweep32 {

// column J of (R, dR) <- (A R + C, dA R + A dR) in place; C given by its tiles of that column.  Six accumulator chains, interleaved.
__device__ __forceinline__ void vcol(const v4d (&A)[2][2], const v4d (&dA)[2][2], v4d (&R)[2][2], v4d (&dR)[2][2], int J, const v4d& c0,
                                     const v4d& c1) {
    const v4d z = {0.0, 0.0, 0.0, 0.0};
    v4d p0 = z, p1 = z, q0 = z, q1 = z, r0 = c0, r1 = c1;
#pragma unroll
    for (int K = 0; K < 2; ++K) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            p0 = __builtin_amdgcn_mfma_f64_16x16x4f64(dA[0][K][kk], R[K][J][kk], p0, 0, 0, 0);
            p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(dA[1][K][kk], R[K][J][kk], p1, 0, 0, 0);
            q0 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[0][K][kk], dR[K][J][kk], q0, 0, 0, 0);
            q1 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[1][K][kk], dR[K][J][kk], q1, 0, 0, 0);
            r0 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[0][K][kk], R[K][J][kk], r0, 0, 0, 0);
            r1 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[1][K][kk], R[K][J][kk], r1, 0, 0, 0);
        }
    }
    dR[0][J] = p0 + q0;
    dR[1][J] = p1 + q1;
    R[0][J] = r0;
    R[1][J] = r1;
}

__device__ __forceinline__ void vstep(const v4d (&A)[2][2], const v4d (&dA)[2][2], v4d (&R)[2][2], v4d (&dR)[2][2], const v4d& cI) {
    const v4d z = {0.0, 0.0, 0.0, 0.0};
    vcol(A, dA, R, dR, 0, cI, z);
    vcol(A, dA, R, dR, 1, z, cI);
}

// the lane's share of sum_IK A(I, K) . B(I, K), added to `acc` (the closed walks' timestep derivative: -wave_sum of it over dY and Ga)
__device__ __forceinline__ double dot_tiles(const v4d (&A)[2][2], const v4d (&B)[2][2], double acc) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = fma(A[q >> 1][q & 1][r], B[q >> 1][q & 1][r], acc);
    return acc;
}

// y_I = sum_K M[K][I]^T v_K: M^T v for a D-layout M and a two-tile column block v
__device__ __forceinline__ void vapplyT(const v4d (&M)[2][2], v4d (&v)[2]) {
    const v4d z = {0.0, 0.0, 0.0, 0.0};
    v4d y0 = z, y1 = z;
#pragma unroll
    for (int K = 0; K < 2; ++K) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            y0 = __builtin_amdgcn_mfma_f64_16x16x4f64(M[K][0][kk], v[K][kk], y0, 0, 0, 0);
            y1 = __builtin_amdgcn_mfma_f64_16x16x4f64(M[K][1][kk], v[K][kk], y1, 0, 0, 0);
        }
    }
    v[0] = y0;
    v[1] = y1;
}

// The paired chain behind already scaled left factors Y, dY (A layout; destroyed: they hold the transposed E, dE of the last squaring):
// R = I/deg!, dR = 0;  (R, dR) <- (Y R + I/(k-1)!, dY R + Y dR), k = deg .. 1;  sq squarings (E, dE) <- (E E, dE E + E dE), both as left
// factors through two LDS round trips of four tiles.  The R chain is exp_plain's, operation for operation.
__device__ __forceinline__ void exp_pair(double* scr, v4d (&Y)[2][2], v4d (&dY)[2][2], int sq, const v4d& IdB, int g, int j, v4d (&R)[2][2],
                                         v4d (&dR)[2][2]) {
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    horner_top(IdB, R);
    dR[0][0] = zero; dR[0][1] = zero; dR[1][0] = zero; dR[1][1] = zero;
#pragma unroll 1
    for (int k = kDeg; k >= 1; --k) vstep(Y, dY, R, dR, kInvFact[k - 1] * IdB);
    for (int q = 0; q < sq; ++q) {
        transpose4(scr, R, Y, g, j);           // E, dE in A layout; Y, dY are free from here on
        transpose4(scr, dR, dY, g, j);
        vstep(Y, dY, R, dR, zero);
    }
}

// KT = lambda x^T (D layout) from the transposed tiles of both (one LDS round trip of four tiles, 16 MFMAs), written as the A-layout
// operand dY(I, K) = KT[K][I]: the block index swapped
__device__ __forceinline__ void outer_kt(double* scr, const v4d (&x)[2], const v4d (&lam)[2], int g, int j, v4d (&dY)[2][2]) {
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    const v4d in[4] = {x[0], x[1], lam[0], lam[1]};
    v4d tr[4];
    lds_transpose16_multi<4>(scr, in, tr, g, j);
    v4d k00 = zero, k01 = zero, k10 = zero, k11 = zero;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        k00 = __builtin_amdgcn_mfma_f64_16x16x4f64(tr[2][kk], tr[0][kk], k00, 0, 0, 0);
        k01 = __builtin_amdgcn_mfma_f64_16x16x4f64(tr[2][kk], tr[1][kk], k01, 0, 0, 0);
        k10 = __builtin_amdgcn_mfma_f64_16x16x4f64(tr[3][kk], tr[0][kk], k10, 0, 0, 0);
        k11 = __builtin_amdgcn_mfma_f64_16x16x4f64(tr[3][kk], tr[1][kk], k11, 0, 0, 0);
    }
    dY[0][0] = k00; dY[1][0] = k01; dY[0][1] = k10; dY[1][1] = k11;
}

// sum_IJ ZT[I][J] . G_u[J][I] over the wave, G_u by its A-layout image (1024 doubles): tile (J, I) = q against ZT[I][J]
__device__ __forceinline__ double contract_image(const v4d (&ZT)[2][2], const double* Gu, int lane) {
    double pu = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const v4d t4 = load_image_tile(Gu + q * 256, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) pu = fma(ZT[q & 1][q >> 1][r], t4[r], pu);
    }
    return wave_sum(pu);
}

}  // namespace qc_sweep32
