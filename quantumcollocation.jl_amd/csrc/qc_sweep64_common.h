// What the kernels of the "mfma64-sweep" form share (qc_sweep64.hip, the forward sweep, and qc_sweep64_grad.hip, its backward walk, which
// must form the same generator and choose the same number of squarings as the forward step): the workgroup's shape and its LDS matrices, the element a thread owns, the
// sample's base matrix, the interval's generator, the squaring rule over the workgroup and the tile product out of LDS.  Constants,
// table, wave sum, rule's tail and chunk range are those of qc_sweep_common.h.  The counterpart of qc_sweep32_common.h.
//
// A matrix is 64 x 64, column-major with a column stride of 66 doubles in LDS (qc_mfma64_kernels.hip: row fragments read consecutive
// rows, column fragments are conflict-free) and with stride 64 in the zero-padded global images.  1024 threads: thread `tid` owns the
// elements idx = tid + 1024 e, e = 0 .. 3 -- row idx & 63 (its lane), column idx >> 6 (its wave + 16 e) -- so a global request of a wave
// is one whole column (512 contiguous bytes) and a column sum is a wave sum.
#pragma once

#include "qc_sweep_common.h"

namespace qc_sweep64 {

using namespace qc_sweep_common;

constexpr int kThreads = 1024;            // 16 waves, one output tile each
constexpr int kLd = 66;                   // column stride of the LDS matrices
constexpr int kMat = 64 * kLd;            // one LDS matrix
constexpr int kImg = 4096;                // one global image
constexpr size_t kLdsBytes = (size_t)4 * kMat * sizeof(double);      // Y, two Horner / squaring buffers, W: 135 168 B

typedef const __attribute__((address_space(1))) double* gptr;       // the images are device memory (qc_mfma_common.h: load_image_tile)

__device__ __forceinline__ int lds_at(int tid, int e) { return ((tid >> 6) + 16 * e) * kLd + (tid & 63); }
__device__ __forceinline__ bool on_diagonal(int tid, int e) { return (tid >> 6) + 16 * e == (tid & 63); }

// the thread's four elements of sample s's base matrix G_drift + sum_q theta[s, q] P_q, by fma in perturbation order
// (images: 4096 doubles a matrix -- drift, m drives, p perturbations)
__device__ __forceinline__ void base_elems(const double* img, int m, int p, const double* __restrict__ theta, long long s, int tid,
                                           double (&base)[4]) {
    const gptr G0 = (gptr)(unsigned long long)img + tid;
#pragma unroll
    for (int e = 0; e < 4; ++e) base[e] = G0[1024 * e];
    for (int q = 0; q < p; ++q) {
        const double th = theta[s * p + q];
        const gptr Pq = G0 + (size_t)(1 + m + q) * kImg;
#pragma unroll
        for (int e = 0; e < 4; ++e) base[e] = fma(th, Pq[1024 * e], base[e]);
    }
}

// the thread's four elements of G = base + sum_u al_u G_u; lane u of `al` holds the (scaled) amplitude of drive u.  The drive images are
// read from global memory every interval (32 KiB a drive, the same for every workgroup of the device: L2-resident).
__device__ __forceinline__ void generator(const double* img, int m, double al, const double (&base)[4], int tid, double (&G)[4]) {
    const gptr G0 = (gptr)(unsigned long long)img + tid;
#pragma unroll
    for (int e = 0; e < 4; ++e) G[e] = base[e];
#pragma unroll 1
    for (int u = 0; u < m; ++u) {
        const double a = bcast_lane(al, u);
        const gptr Gu = G0 + (size_t)(1 + u) * kImg;
#pragma unroll
        for (int e = 0; e < 4; ++e) G[e] = fma(a, Gu[1024 * e], G[e]);
    }
}

// The number of squarings, workgroup-uniform: the smallest sq with ||h G||_1 / 2^sq <= 1/8 (0 for a non-finite norm).  ||h G||_1 is
// the largest column sum; wave w holds the columns w + 16 e, one row a lane, so a column sum is a wave sum (fixed order).  Each wave
// leaves the largest of its four in red[w] (infinity for a sum that is not finite) and every thread takes the largest of the sixteen.
// Holds one workgroup barrier: behind it every wave has left the previous interval's products.
__device__ __forceinline__ int squarings(double* __restrict__ red, const double (&G)[4], double h, int lane, int w) {
    double best = 0.0;
    bool bad = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double v = wave_sum(fabs(h * G[e]));
        if (!(v == v) || v > 1e300) bad = true;
        best = fmax(best, v);
    }
    if (lane == 0) red[w] = bad ? __builtin_inf() : best;
    __syncthreads();
    double all = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) all = fmax(all, red[i]);
    return squarings_of_norm(all, all > 1e300);
}

// Tile (I, J) of D = A B + c I, all three column-major in LDS, D distinct from A and B: one chain of 16 MFMAs over ascending k.
// a = row fragment I of A (lane (g, i), step q: A[16 I + i][4 q + g]), b = column fragment J of B (lane (g, j), step q:
// B[4 q + g][16 J + j]); the tile leaves in the D layout (lane (g, j) reg r = D[16 I + 4 r + g][16 J + j]).
__device__ __forceinline__ void tile_mul(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ D, int I, int J, int g,
                                         int j, double c) {
    const double* __restrict__ pa = A + g * kLd + 16 * I + j;
    const double* __restrict__ pb = B + (16 * J + j) * kLd + g;
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    v4d acc = I == J ? c * identity_B(g, j) : zero;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[q * 4 * kLd], pb[4 * q], acc, 0, 0, 0);
    double* __restrict__ pd = D + (16 * J + j) * kLd + 16 * I + g;
#pragma unroll
    for (int r = 0; r < 4; ++r) pd[4 * r] = acc[r];
}

// ---- the pieces of the backward walk (qc_sweep64_grad.hip): fragments of either operand, as it stands or transposed ----------------------
// The thin matrices (a state, an adjoint: 64 x <= 32) keep the column stride kLd, so one pair of address forms serves every operand:
//   row_frag(M, T): lane (g, i), step q reads M[16 T + i][4 q + g]  (stride kRowStep)  -- the A operand of M X, the B operand of X M^T
//   col_frag(M, T): lane (g, j), step q reads M[4 q + g][16 T + j]  (stride kColStep)  -- the B operand of X M, the A operand of M^T X
// (both conflict-free by the stride of 66: tile_mul's two reads).
constexpr int kThin = 32 * kLd;           // one thin LDS matrix: 64 rows x 32 columns
constexpr int kRowStep = 4 * kLd, kColStep = 4;

__device__ __forceinline__ const double* row_frag(const double* M, int T, int g, int j) { return M + g * kLd + 16 * T + j; }
__device__ __forceinline__ const double* col_frag(const double* M, int T, int g, int j) { return M + (16 * T + j) * kLd + g; }

// acc += sum over NQ steps of a-fragment x b-fragment, ascending k (NQ = 16: a whole 64-long contraction, tile_mul's chain)
template <int SA, int SB, int NQ>
__device__ __forceinline__ v4d chain(const double* __restrict__ pa, const double* __restrict__ pb, v4d acc) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[q * SA], pb[q * SB], acc, 0, 0, 0);
    return acc;
}

// a tile held in registers (D layout) into tile (I, J) of the LDS matrix D
__device__ __forceinline__ void store_tile(double* __restrict__ D, int I, int J, int g, int j, const v4d& acc) {
    double* __restrict__ pd = D + (16 * J + j) * kLd + 16 * I + g;
#pragma unroll
    for (int r = 0; r < 4; ++r) pd[4 * r] = acc[r];
}

}  // namespace qc_sweep64
