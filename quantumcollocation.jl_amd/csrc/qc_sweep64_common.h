// What the kernels of the "mfma64-sweep" form share (qc_sweep64.hip, the forward sweep with and without noise; qc_sweep64_grad.hip and
// qc_sweep64_noise.hip, the backward walks, which must form the same generator and choose the same number of squarings as the forward
// step; qc_sweep64_open_grad.hip, the stored-state walk and its store kernel; qc_sweep64_jvp.hip, the pushforward): the workgroup's shape and its LDS matrices, the element a thread owns, the sample's base
// matrix, the lane's coefficient source, the interval's generator, the squaring rule over the workgroup, the tile product out of LDS, the
// pieces of the walk (its LDS map, the state load, the timestep derivative, the exponential pair with its barriers, the 16-wave sum).
// The launch is qc_sweep64_launch.h's.  Constants, table, wave sum, rule's tail and chunk range are those of qc_sweep_common.h.  The
// counterpart of qc_sweep32_common.h and qc_sweep32_walk.h.
//
// A matrix is 64 x 64, column-major with a column stride of 66 doubles in LDS (qc_mfma64_kernels.hip: row fragments read consecutive
// rows, column fragments are conflict-free) and with stride 64 in the zero-padded global images.  1024 threads: thread `tid` owns the
// elements idx = tid + 1024 e, e = 0 .. 3 -- row idx & 63 (its lane), column idx >> 6 (its wave + 16 e) -- so a global request of a wave
// is one whole column (512 contiguous bytes) and a column sum is a wave sum.
//
// Not shared, and why: qc_sweep64_jvp.hip's generator_pair runs two fma chains over one pass of the images, which `generator` with any
// coefficient source cannot state without reading the images twice (it stays in that file, as chain_pair does: one user each).
#pragma once

#include "qc_sweep_common.h"
#include "qc_sweep_internal.h"      // SweepParams, the kernels' launch-parameter POD (lane_coef)

namespace qc_sweep64 {

using namespace qc_sweep_common;

constexpr int kThreads = 1024;            // 16 waves, one output tile each
constexpr int kLd = 66;                   // column stride of the LDS matrices
constexpr int kMat = 64 * kLd;            // one LDS matrix
constexpr int kImg = 4096;                // one global image
constexpr size_t kLdsBytes = (size_t)4 * kMat * sizeof(double);      // Y, two Horner / squaring buffers, W: 135 168 B
constexpr int kThin = 32 * kLd;           // one thin LDS matrix (a state, an adjoint): 64 rows x 32 columns
constexpr size_t kWalkLdsBytes = (size_t)(3 * kMat + 3 * kThin) * sizeof(double);      // the walks' Y, R, dR, x, lambda, u: 152 064 B

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

// the lane's control value in the knot at `z`
__device__ __forceinline__ double drive_value(const double* z, int off_a, int m, int kl) { return m > 0 ? z[off_a + kl] : 0.0; }

// The noise sweeps' source, over the mt = m + p generators (drives, then perturbations; p >= 1: there always is one): where lane l finds
// the coefficient of generator min(l, mt - 1) in interval t, how far the next interval's lies, and the sample's factor.
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

// the thread's four elements of G = base + sum_u coef(u) G_u over the images 1 .. n, ascending u.  The images are read from global memory
// every interval (32 KiB each, the same for every workgroup of the device: L2-resident).
template <class Coef>
__device__ __forceinline__ void generator_of(const double* img, int n, Coef coef, const double (&base)[4], int tid, double (&G)[4]) {
    const gptr G0 = (gptr)(unsigned long long)img + tid;
#pragma unroll
    for (int e = 0; e < 4; ++e) G[e] = base[e];
#pragma unroll 1
    for (int u = 0; u < n; ++u) {
        const double a = coef(u);
        const gptr Gu = G0 + (size_t)(1 + u) * kImg;
#pragma unroll
        for (int e = 0; e < 4; ++e) G[e] = fma(a, Gu[1024 * e], G[e]);
    }
}

// the same with lane u of `al` holding the (scaled) coefficient of generator u
__device__ __forceinline__ void generator(const double* img, int n, double al, const double (&base)[4], int tid, double (&G)[4]) {
    generator_of(img, n, [al](int u) { return bcast_lane(al, u); }, base, tid, G);
}

// The number of squarings, workgroup-uniform: the smallest sq with ||h G||_1 / 2^sq <= 1/8 (0 for a non-finite norm).  ||h G||_1 is
// the largest column sum; wave w holds the columns w + 16 e, one row a lane, so a column sum is a wave sum (fixed order).  Each wave
// leaves the largest of its four in red[w] (infinity for a sum that is not finite) and every thread takes the largest of the sixteen.
// Holds one workgroup barrier, S: behind it every wave has left the previous interval's products, so a kernel may overwrite what those
// products read right behind the call.  red[] needs two kinds of barrier: S stands between its writes and their reads, and at least one
// further workgroup barrier must stand between a call of squarings() and the next (between those reads and the next call's writes).
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

// ---- the closed backward walk: what qc_sweep64_grad_kernel<PAR> and qc_sweep64_noise_grad_kernel share -------------------------------------
// LDS map of the dynamic part (doubles; column stride 66 everywhere), kWalkLdsBytes:
//     Y | R | dR | x | lambda | u         64 x 64 | 64 x 64 | 64 x 64 | 64 x 32 | 64 x 32 | 64 x 32
// Wave w owns tile (I, J) = (w & 3, w >> 2) of every 64 x 64 product and tile (I, J & 1) of x (w < 8) or of lambda (w >= 8).
struct WalkLds {
    double *Y, *R, *dR, *X, *L, *U;
};

__device__ __forceinline__ WalkLds walk_lds(double* sm) {
    return {sm, sm + kMat, sm + 2 * kMat, sm + 3 * kMat, sm + 3 * kMat + kThin, sm + 3 * kMat + 2 * kThin};
}

// an n x nc column-major state at `p` into the thin LDS matrix M, zero outside n x nc (two elements a thread)
__device__ __forceinline__ void load_state(const double* __restrict__ p, int n, int nc, int tid, double* M) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int idx = tid + 1024 * e, row = idx & 63, col = idx >> 6;
        M[col * kLd + row] = (row < n && col < nc) ? p[row + n * col] : 0.0;
    }
}

// The timestep derivative before its sign, wave-uniform: sum_ab KT[a][b] G[b][a] over the wave's elements G[b = lane][a = w + 16 e],
// KT[a][b] = sum_c lambda[a][c] x[b][c].  Reads x and lambda: called behind S, which stands between their writes (behind Ba) and here.
__device__ __forceinline__ double kt_dot(const double* X, const double* L, int nc, const double (&G)[4], int lane, int w) {
    double kt[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nc; ++c) {
        const double xv = X[c * kLd + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e) kt[e] = fma(L[c * kLd + w + 16 * e], xv, kt[e]);
    }
    double ph = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) ph = fma(kt[e], G[e], ph);
    return wave_sum(ph);
}

// The exponential pair of one interval, in place: on return R holds E = exp(hs 2^sq G) and dR its Frechet derivative in the direction
// hs 2^sq x lambda^T (nct = 1 or 2 column tiles of x, lambda).  Call it behind squarings(): Y, R = I/8!, dR = 0 are written behind S.
//     Horner, k = 8 .. 1:   R_k = Y R_k+1 + I/(k-1)!,   dR_k = dY R_k+1 + Y dR_k+1,   dY R = x u^T with u = hs R^T lambda (dY is never formed)
//     sq squarings:         E' = E E,   dE' = E dE + dE E
// A wave's tile of a product is 4 registers a lane, so R and dR are updated IN PLACE: every wave holds its tiles of the new R, dR in registers
// across a barrier, writes them over the old ones, and a second barrier publishes them.  Barriers, in order, and what each stands between:
//     H0  publishes Y, R, dR.
//     per Horner step:   u = hs R^T lambda (waves 0 .. 4 nct - 1; reads R, lambda; writes u)
//     U   publishes u;   R' = Y R + I/(k-1)!,  dR' = Y dR + x u^T into registers (reads Y, R, dR, x, u)
//     P   every read of R, dR, u of this step is done;   R <- R', dR <- dR'
//     W   publishes R, dR (the next step's u reads R; u is overwritten only behind W)
//     per squaring:   E' = E E, dE' = E dE + dE E into registers;  P;  write;  W      (the same two barriers)
// The R chain is tile_mul's, MFMA for MFMA.  At least 25 barriers: red[]'s rule (squarings()) holds for every caller.
__device__ __forceinline__ void exp_pair(const WalkLds& m, const double (&G)[4], double hs, int sq, int nct, int tid, int I, int J, int g, int j) {
    const int Jc = J & 1;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        m.Y[lds_at(tid, e)] = hs * G[e];
        m.R[lds_at(tid, e)] = on_diagonal(tid, e) ? kInvFact[kDeg] : 0.0;
        m.dR[lds_at(tid, e)] = 0.0;
    }
    __syncthreads();      // H0
#pragma unroll 1
    for (int k = kDeg; k >= 1; --k) {
        if (J < 2 && Jc < nct) {
            const v4d u = chain<kColStep, kColStep, 16>(col_frag(m.R, I, g, j), col_frag(m.L, Jc, g, j), zero);
            store_tile(m.U, I, Jc, g, j, hs * u);
        }
        __syncthreads();      // U
        const v4d c0 = I == J ? kInvFact[k - 1] * IdB : zero;
        const v4d nR = chain<kRowStep, kColStep, 16>(row_frag(m.Y, I, g, j), col_frag(m.R, J, g, j), c0);
        v4d nD = chain<kRowStep, kColStep, 16>(row_frag(m.Y, I, g, j), col_frag(m.dR, J, g, j), zero);
        nD = chain<kRowStep, kRowStep, 4>(row_frag(m.X, I, g, j), row_frag(m.U, J, g, j), nD);
        if (nct > 1) nD = chain<kRowStep, kRowStep, 4>(row_frag(m.X, I, g, j) + 16 * kLd, row_frag(m.U, J, g, j) + 16 * kLd, nD);
        __syncthreads();      // P
        store_tile(m.R, I, J, g, j, nR);
        store_tile(m.dR, I, J, g, j, nD);
        __syncthreads();      // W
    }
#pragma unroll 1
    for (int q = 0; q < sq; ++q) {
        const v4d nE = chain<kRowStep, kColStep, 16>(row_frag(m.R, I, g, j), col_frag(m.R, J, g, j), zero);
        v4d nD = chain<kRowStep, kColStep, 16>(row_frag(m.R, I, g, j), col_frag(m.dR, J, g, j), zero);
        nD = chain<kRowStep, kColStep, 16>(row_frag(m.dR, I, g, j), col_frag(m.R, J, g, j), nD);
        __syncthreads();      // P
        store_tile(m.R, I, J, g, j, nE);
        store_tile(m.dR, I, J, g, j, nD);
        __syncthreads();      // W
    }
}

// lane l's value summed over the 16 waves' rows of part[] (LD values a row), ascending wave order; read behind Ba, which stands between
// the waves' writes and this; the next writes are a whole interval of barriers later
template <int LD>
__device__ __forceinline__ double part_sum(const double* part, int lane) {
    double acc = part[lane];
#pragma unroll
    for (int i = 1; i < 16; ++i) acc += part[i * LD + lane];
    return acc;
}

}  // namespace qc_sweep64
