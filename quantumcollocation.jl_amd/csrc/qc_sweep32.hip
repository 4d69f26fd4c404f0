// Rollout sweeps for 16 < 2N <= 32 with up to 8 drives ("mfma32-sweep"): the forward kernel of qc_sweep.hip with every matrix 2 x 2
// tiles of 16 x 16 on v_mfma_f64_16x16x4_f64.  Taken only by descriptors with wide = QC_SWEEP_WIDE; the mathematics (Y = dt G_s(a_t) / 2^sq
// with ||Y||_1 <= 1/8 and a wave-uniform sq, the degree-8 Horner chain with the correctly rounded 1/k! table, sq squarings, W <- E_t W),
// the work item (one wavefront per (sample, chunk of consecutive intervals), four per workgroup, never synchronised: wave_item and
// chunk_range of qc_sweep_common.h, as in every kernel of both forms) and the chunk rule are those of qc_sweep_mfma16_kernel.  The interval
// body below restates drive_lane, exp_plain (qc_sweep32_common.h; qc_sweep32_open_store_kernel calls them) and the total's store, as
// qc_sweep32_noise_kernel does: the calls move this kernel's VGPRs or its time ("Shared and restated in the wide kernels").  Sizes 18 .. 30 are zero-padded to 32: the exponential of the padded generator is the exponential of
// the true one plus an identity block.
//
// Tiles.  X[I][J] is the tile of rows 16 I .. and columns 16 J ..; lane maps per tile as everywhere (qc_mfma_kernels.hip header):
// A layout lane (g, i) reg kk = A[i][4kk+g], B / D layout lane (g, j) reg r = X[4r+g][j].  A product is D[I][J] = sum_K A[I][K] B[K][J]:
// 8 tile products, 32 MFMAs.  Column J of a product depends on column J of the right factor only, so R <- Y R and R <- E R are done
// in place one tile column at a time (two accumulator tiles, two independent MFMA chains).  "A D-layout tile read as the A operand is
// its transpose" holds per tile: E as the LEFT factor needs the four tiles transposed (one LDS round trip of four tiles); the block
// index does not move.  MFMAs per interval: 8 x 32 + 32 sq + 32.
//
// Registers.  A matrix is 32 VGPRs per lane, so the drive tiles (up to 256 VGPRs) are not kept: the sample's base matrix
// G_drift + sum theta P_j stays in registers, and the m drive images are read again every interval from the image buffer
// ([matrix][tile I][tile K][pair][lane][2], 16-byte loads; the same 8 KiB per drive for every wave of the device, L2-resident):
// 8 loads per drive and lane against 288+ MFMAs.  The number of drives is a loop bound, not a template parameter: one instantiation.
// The chunk total leaves as a full 32 x 32 column-major matrix (S x n_chunks x 1024 doubles of handle scratch);
// qc_sweep_finish_kernel (qc_sweep.hip) chains the totals with ld = 32.
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_side.h"
#include "qc_sweep32_common.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep32;

__global__ __launch_bounds__(64 * kWaves, 2) void qc_sweep_mfma32_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                           const double* __restrict__ theta, const double* __restrict__ scale,
                                                                           double* __restrict__ tot) {
    __shared__ double scr_all[kWaves * kScr];
    const WaveItem w = wave_item(kWaves);
    double* __restrict__ scr = scr_all + w.wq * kScr;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    // ---- once per wave: the sample's base matrix ----------------------------------------------------------------------------------
    v4d base[2][2];
    base_matrix(P.img, m, P.p, theta, s, lane, base);
    // lane l holds the sample's factor of drive min(l, m-1); folded into the control values
    const int kl = lane < m ? lane : (m > 0 ? m - 1 : 0);
    const double cl = (scale && m > 0) ? scale[s * m + kl] : 1.0;

    const double* __restrict__ z = Z + (long long)t0 * P.zdim;
    double av = m > 0 ? z[P.off_a + kl] : 0.0;
    const double hfix = opaque_scalar(P.dt_fixed);      // keeps the two arms apart: no flat load (qc_mfma_common.h)
    double h = ft ? z[P.off_dt] : hfix;
    v4d W[2][2] = {{IdB, zero}, {zero, IdB}};
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        // the next interval's controls and timestep are requested before this interval's products
        const double* __restrict__ zn = Z + (long long)(t + 1 < t1 ? t + 1 : t) * P.zdim;
        const double av_n = m > 0 ? zn[P.off_a + kl] : 0.0;
        const double h_n = ft ? zn[P.off_dt] : hfix;
        const double al = av * cl;
        v4d Y[2][2];
        generator(P.img, m, al, base, lane, Y);
        const int sq = squarings(Y, h);
        const double hs = h * ldexp(1.0, -sq);
#pragma unroll
        for (int q = 0; q < 4; ++q) Y[q >> 1][q & 1] = hs * Y[q >> 1][q & 1];
        // Horner: R_deg+1 = I/deg!,  R_k = Y R_k+1 + I/(k-1)!   (the last coefficient is exactly 1: a zero generator gives the identity bits)
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

}  // namespace

// A-layout image of one n x n column-major matrix, zero outside n x n: [tile I][tile K][pair][lane][2], pair, e -> kk = 2 pair + e
void qc_sweep32_image(const double* G, int n, double* img) {
    for (int I = 0; I < 2; ++I)
        for (int K = 0; K < 2; ++K)
            for (int kk = 0; kk < 4; ++kk)
                for (int lane = 0; lane < 64; ++lane) {
                    const int g = lane >> 4, i = lane & 15, row = 16 * I + i, col = 16 * K + 4 * kk + g;
                    img[(size_t)(2 * I + K) * 256 + (size_t)(kk >> 1) * 128 + (size_t)lane * 2 + (kk & 1)] =
                        (row < n && col < n) ? G[(size_t)col * n + row] : 0.0;
                }
}

int qc_sweep32_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, hipStream_t st, int64_t* chunk_out,
                             int64_t* n_chunks_out) {
    SweepParams P;
    if (int rc = qc_sweep_plan_totals(h, S, h->dTot, 1024, &P, chunk_out, n_chunks_out)) return rc;
    hipLaunchKernelGGL(qc_sweep_mfma32_kernel, dim3(qc_sweep_grid(P, kWaves)), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale, h->dTot.p);
    return QC_OK;
}
