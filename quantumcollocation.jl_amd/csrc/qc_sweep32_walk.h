// What the two backward walks of the "mfma32-sweep" form share: the closed walk of qc_sweep32_grad.hip (qc_sweep32_grad_kernel, which reverses
// the forward step) and the stored-state walk of qc_sweep32_open_grad.hip (qc_sweep32_open_grad_kernel, which reads the forward states).
// The paired column step of the Horner / squaring chains on 2 x 2 tiles and the product with E^T; constants, generator and squaring rule
// are those of qc_sweep32_common.h, the wave sum that of qc_sweep_common.h.
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

}  // namespace qc_sweep32
