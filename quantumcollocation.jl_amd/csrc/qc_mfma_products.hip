// Fused matrix-free forward Jacobian product of the order-4 Pade integrator at 2N <= 16 with up to 8 state columns and up to 8 drives
// (unitaries on 1 - 3 qubits, kets, the zero-padded sizes) on v_mfma_f64_16x16x4_f64: y = dF(Z) v without a single Jacobian value in
// memory -- nothing is written to HBM but the result.  Operand layouts and helpers: qc_mfma_common.h and the header of
// qc_mfma_kernels.hip (A layout: lane (g, i) reg kk = X[i][4kk+g]; B = C/D layout: lane (g, j) reg r = X[4r+g][j]; two 16 x 8 matrices
// share a tile, swap8 exchanges the halves).
//
// Per interval: h = dt_t, G = G(a_t), S = U_t+1 + U_t, D = U_t+1 - U_t, c1 = 1/2, c2 = 1/12 (the Pade coefficients),
//   B, F = I -+ h c1 G + h^2 c2 G^2,   residual = B U_t+1 - F U_t.
// ONE WAVE PER INTERVAL (V0, V1 the state parts of v, Sv = V1 + V0, Dv = V1 - V0, Gv = sum_j v_aj G_j, vh the timestep entry):
//   y_U = B V1 - F V0 - h c1 Gv S + h^2 c2 (Gv (G D) + G (Gv D)) + vh (-c1 G S + 2 h c2 G^2 D)
//       = Dv - h c1 (G Sv + Gv S) - vh c1 G S + G [h^2 c2 (G Dv + Gv D) + 2 h c2 vh G D] + h^2 c2 Gv (G D)
//   P1 = G [S | D], P2 = G [Sv | Dv], P3 = Gv [S | D], P4 = G [h^2 c2 (P2 + P3) + 2 h c2 vh P1]_right, P5 = Gv [P1]_right: 20 MFMAs.
//   Derivative-integrator rows: v_x,t+1 - v_x,t - h v_dx,t - dx_t vh.
// Every output entry has one writer; no atomics.
// Launch form: one 64-lane workgroup per interval, a persistent grid beyond kMaxGrid workgroups.
// The transposed product has no fused kernel (profiles/products_summary.txt): dF' lam takes the generic path, qc_products.hip.
#include "qc_mfma_common.h"

namespace {

using namespace qc_mfma;

constexpr int kMaxGrid = 1024;      // workgroups (= waves) of a launch; longer trajectories loop
constexpr int kMaxDrives = 8;

__device__ inline v4d load_GA(const double* __restrict__ Gx, int mat, int lane) { return load_image_tile(Gx + mat * 256, lane); }

// Zero-padded state tile [X | 0] or [X | X]: lane (g, j) reg r = X[4r+g][j & 7] for rows < nr and columns < nc, else 0
template <bool BOTH>
__device__ inline v4d load_tile(const double* __restrict__ x, int nr, int nc, int g, int j) {
    const int jj = j & 7;
    const bool col_ok = jj < nc && (BOTH || j < 8);
    v4d v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = (col_ok && 4 * r + g < nr) ? x[jj * nr + 4 * r + g] : 0.0;
    return v;
}

// G(a) and G2 = sum_k a2_k G_k (no drift), both in the A layout
__device__ inline void assemble2(const double* __restrict__ Gx, int m, int lane, double av, double av2, v4d& Ga, v4d& G2) {
    Ga = load_GA(Gx, 0, lane);
    G2 = v4d{0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < m; ++k) {
        const v4d img = load_GA(Gx, k + 1, lane);
        Ga += bcast_lane(av, k) * img;
        G2 += bcast_lane(av2, k) * img;
    }
}

__global__ __launch_bounds__(64) void qc_mfma16_jvp_kernel(const QcParams P, const double* __restrict__ Z, const double* __restrict__ V,
                                                           double* __restrict__ Y) {
    const int lane = threadIdx.x, g = lane >> 4, j = lane & 15;
    const bool left = j < 8;
    const int nr = P.n, nc = P.nc, m = P.m, zdim = P.zdim;
    const bool ft = P.off_dt >= 0;
    const double c1 = P.c[1], c2 = P.c[2];
    for (int b = blockIdx.x; b < P.n_int; b += gridDim.x) {
        const long long t = P.t_begin + b;
        const double* __restrict__ z0 = Z + t * (long long)zdim;
        const double* __restrict__ z1 = z0 + zdim;
        const double* __restrict__ v0 = V + t * (long long)zdim;
        const double* __restrict__ v1 = v0 + zdim;
        double* __restrict__ yb = Y + (size_t)b * P.F_stride + P.F_off;
        const double h = ft ? load_uniform(z0 + P.off_dt) : opaque_scalar(P.dt_fixed);
        const double vh = ft ? load_uniform(v0 + P.off_dt) : 0.0;
        const double av = load_amp_lanes(z0, P.off_a, m, lane), avv = load_amp_lanes(v0, P.off_a, m, lane);
        v4d Ga, Gv;
        assemble2(P.Gx, m, lane, av, avv, Ga, Gv);
        const v4d u0 = load_tile<true>(z0 + P.off_U, nr, nc, g, j), u1 = load_tile<true>(z1 + P.off_U, nr, nc, g, j);
        const v4d x0 = load_tile<true>(v0 + P.off_U, nr, nc, g, j), x1 = load_tile<true>(v1 + P.off_U, nr, nc, g, j);
        v4d T1, T2;      // [S | D], [Sv | Dv]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            T1[r] = left ? u1[r] + u0[r] : u1[r] - u0[r];
            T2[r] = left ? x1[r] + x0[r] : x1[r] - x0[r];
        }
        const v4d A3[3] = {Ga, Ga, Gv}, B3[3] = {T1, T2, T1};
        v4d P123[3];
        mm16_multi<3>(A3, B3, P123);
        const v4d &P1 = P123[0], &P2 = P123[1], &P3 = P123[2];      // [G S | G D], [G Sv | G Dv], [Gv S | Gv D]
        const double hc1 = h * c1, hc2 = h * h * c2, dhc2 = 2.0 * h * c2 * vh;
        v4d Wt;
#pragma unroll
        for (int r = 0; r < 4; ++r) Wt[r] = hc2 * (P2[r] + P3[r]) + dhc2 * P1[r];
        const v4d A2[2] = {Ga, Gv}, B2[2] = {swap8(Wt), swap8(P1)};
        v4d P45[2];
        mm16_multi<2>(A2, B2, P45);
        const v4d Dv = swap8(T2);
        const double vc1 = vh * c1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double y = Dv[r] - hc1 * (P2[r] + P3[r]) - vc1 * P1[r] + P45[0][r] + hc2 * P45[1][r];
            if (left && j < nc && 4 * r + g < nr) yb[j * nr + 4 * r + g] = y;
        }
        for (int d = 0; d < P.n_deriv; ++d) {
            const int dim = P.ddim_i[d], r0 = P.drow[d], xo = P.x_off[d], dxo = P.dx_off[d];
            for (int i = lane; i < dim; i += 64) yb[r0 + i] = v1[xo + i] - v0[xo + i] - h * v0[dxo + i] - z0[dxo + i] * vh;
        }
    }
}

}  // namespace

// Gx holds the 16 x 16 A-layout images (an MFMA handle at 2N <= 16); QC_NO_PRODUCT_MFMA=1 at create time clears cls.product_mfma.
bool qc_mfma16_products_supported(const QcParams& P, const QcClass& cls) {
    return cls.kernel == QC_KERNEL_MFMA && cls.product_mfma && P.integrator == QC_PADE && P.p == 2 && P.n <= 16 && P.nc <= 8 && P.m <= kMaxDrives;
}

hipError_t qc_launch_mfma16_jvp(const QcParams& P, const double* dZ, const double* dv, double* dy, hipStream_t st) {
    const int grid = P.n_int < kMaxGrid ? P.n_int : kMaxGrid;
    hipLaunchKernelGGL(qc_mfma16_jvp_kernel, dim3(grid), dim3(64), 0, st, P, dZ, dv, dy);
    return hipGetLastError();
}
