// Sweep pushforwards for "mfma32-sweep" handles (16 < 2N <= 32) made with QC_SWEEP_WIDE_TANGENT in `wide`: qc_sweep_jvp_kernel
// (qc_sweep_jvp.hip; read its header first) with every matrix 2 x 2 tiles of 16 x 16, as qc_sweep32.hip is qc_sweep.hip on such tiles.
// The mathematics is that file's, line for line:
//     d(hG)_t = vh_t G_s(a_t) + h_t ( sum_j vtheta[s,j] P_j + sum_k ( vc[s,k] a_{t,k} + c[s,k] va_{t,k} ) G_k )
//     Wdot <- E_t Wdot + L(h_t G; d(hG)_t) W,  W <- E_t W        over the intervals of the chunk
// Nothing is reversed: Lindblad generators are served like any others, no flag and no state buffer (two qubits with T1 / T2: 2N = 32).
//
// Work item and chunk rule are qc_sweep_mfma32_kernel's (wave_item / chunk_range of qc_sweep_common.h): one wavefront per (sample, chunk),
// the waves of a workgroup (two, see "Registers") never synchronised.  The paired chain is exp_pair of qc_sweep32_walk.h; c[s,k] waits in
// LDS, so drive_lane is restated.  base_matrix, squarings, transpose4 and the 1/k! table come from qc_sweep32_common.h, the paired column
// step from qc_sweep32_walk.h (vcol: its R chain is wcol's, operation for operation).  Per interval:
//   once per wave   Bdot = sum_j vtheta[s,j] P_j (A layout), the lane's vc[s,k] beside c[s,k]
//   coefficients    al = a c,  aldot = va c + a vc
//   generators      Ga = base + sum al_u G_u,  Gadot = Bdot + sum aldot_u G_u      one pass over the drive images (generator_pair: the
//                   Ga chain is `generator`'s, the same fma on the same operands in the same order)
//   squarings       sq from ||h Ga||_1 by `squarings`; the tangent never influences it
//   scaled tiles    Ydot = (vh 2^-sq) Ga + (h 2^-sq) Gadot,  Y = (h 2^-sq) Ga
//   Horner          Rdot <- Ydot R + Y Rdot (from the old R), R <- Y R + I/(k-1)!, one tile column at a time      8 x 96 MFMAs
//   per squaring    Rdot <- E Rdot + Edot E, R <- E E      E, Edot as left factors: eight tiles transposed in two LDS round trips   96
//   totals          Wdot <- E Wdot + Edot W, W <- E W                                                                               96
// 864 + 96 sq MFMAs per interval against the forward 288 + 32 sq: 3.0 forward sweeps by the count.  The R / W chain is the forward
// kernel's operation for operation, so W carries its bits.  The wave stores W and Wdot as two column-major 32 x 32 matrices:
// S x n_chunks x 2048 doubles of h->dTotJ; qc_sweep_jvp_finish_kernel (qc_sweep_jvp.hip) chains them with ld = 32.
//
// Registers.  Eight matrices (base, Bdot, Y, Ydot, R, Rdot, W, Wdot) are 256 VGPRs a lane and the six accumulator tiles of a column
// step 48 more: one wave per SIMD with the unified VGPR + AGPR file, as qc_sweep32_grad.hip.  With all eight in registers and four waves
// a workgroup the kernel spilled 6 scalar and 4 vector registers; Bdot (read once per interval), the lane's c[s,k] and vc[s,k] and its
// address in the output therefore wait in the wave's LDS slice behind the transposition tiles, and two waves make a workgroup (2 x 18 KiB:
// static LDS under 64 KiB).  gfx950 cross-compile: 256 VGPRs + 102 AGPRs, 106 SGPRs, 36864 B LDS (two waves); no private segment, no
// spills ("Wide sweep pushforwards").
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_sweep32_common.h"
#include "qc_sweep32_walk.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep32;

// G = base + sum_u al_u G_u and Gd = based + sum_u ald_u G_u in A layout from one pass over the drive images.  The G chain is
// qc_sweep32::generator's: the same fma on the same operands in the same order, so G carries its bits.
__device__ __forceinline__ void generator_pair(const double* __restrict__ img, int m, double al, double ald, const v4d (&base)[2][2],
                                               const double* __restrict__ bdl, int lane, v4d (&G)[2][2], v4d (&Gd)[2][2]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        G[q >> 1][q & 1] = base[q >> 1][q & 1];
#pragma unroll
        for (int r = 0; r < 4; ++r) Gd[q >> 1][q & 1][r] = bdl[64 * (4 * q + r) + lane];
    }
#pragma unroll 1
    for (int u = 0; u < m; ++u) {
        const double a = bcast_lane(al, u);
        const double ad = bcast_lane(ald, u);
        const double* __restrict__ Gu = img + (size_t)(1 + u) * 1024;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const v4d t4 = load_image_tile(Gu + q * 256, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                G[q >> 1][q & 1][r] = fma(a, t4[r], G[q >> 1][q & 1][r]);
                Gd[q >> 1][q & 1][r] = fma(ad, t4[r], Gd[q >> 1][q & 1][r]);
            }
        }
    }
}

constexpr int kJW = 2;                       // waves a workgroup: one wave per SIMD either way (512 registers a wave)
constexpr int kJSl = kScr + 19 * 64;         // doubles of LDS a wave: the transposition tiles; behind them Bdot and three values a lane

__global__ __launch_bounds__(64 * kJW) void qc_sweep32_jvp_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                      const double* __restrict__ theta, const double* __restrict__ scale,
                                                                      const double* __restrict__ vZ, const double* __restrict__ vtheta,
                                                                      const double* __restrict__ vscale, double* __restrict__ tot) {
    __shared__ double scr_all[kJW * kJSl];
    const WaveItem w = wave_item(kJW);
    double* __restrict__ scr = scr_all + w.wq * kJSl;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m;
    const bool ft = P.off_dt >= 0;
    const bool hasv = vZ != nullptr;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    // ---- once per wave: the sample's base matrix and its tangent -------------------------------------------------------------------
    v4d base[2][2];
    base_matrix(P.img, m, P.p, theta, s, lane, base);
    // Bdot lives in the wave's LDS slice behind the transposition tiles (tile q of lane l, register r at bdl[64 (4 q + r) + l]: every lane
    // reads back what it wrote itself, no barrier): it is read once per interval, and eight resident matrices would be all 256 VGPRs
    double* __restrict__ bdl = scr + kScr;
    {
        v4d based[2][2] = {{zero, zero}, {zero, zero}};
        if (vtheta) {
            for (int q = 0; q < P.p; ++q) {
                const double vth = vtheta[s * P.p + q];
                const double* __restrict__ Pq = P.img + (size_t)(1 + m + q) * 1024;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const v4d t = load_image_tile(Pq + u * 256, lane);
#pragma unroll
                    for (int r = 0; r < 4; ++r) based[u >> 1][u & 1][r] = fma(vth, t[r], based[u >> 1][u & 1][r]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) bdl[64 * (4 * q + r) + lane] = based[q >> 1][q & 1][r];
    }
    // lane l holds the sample's factor of drive min(l, m-1) and its tangent
    const int kl = lane < m ? lane : (m > 0 ? m - 1 : 0);
    // c[s,k], vc[s,k] and the lane's address in the output wait in LDS as well, each lane's own slot: read once per interval / at the
    // chunk's end, they would otherwise hold registers across the loop, which has none to spare
    double* __restrict__ pk = bdl + 16 * 64 + lane;
    pk[0] = (scale && m > 0) ? scale[s * m + kl] : 1.0;
    pk[64] = (vscale && m > 0) ? vscale[s * m + kl] : 0.0;
    pk[128] = __longlong_as_double((long long)(tot + item * 2048 + j * 32 + g));

    const double* __restrict__ z = Z + (long long)t0 * P.zdim;
    double av = m > 0 ? z[P.off_a + kl] : 0.0;
    const double hfix = opaque_scalar(P.dt_fixed);
    double h = ft ? z[P.off_dt] : hfix;
    double vav = 0.0, vh = 0.0;
    if (hasv) {
        const double* __restrict__ vz = vZ + (long long)t0 * P.zdim;
        if (m > 0) vav = vz[P.off_a + kl];
        if (ft) vh = vz[P.off_dt];
    }
    v4d W[2][2] = {{IdB, zero}, {zero, IdB}};
    v4d Wd[2][2] = {{zero, zero}, {zero, zero}};
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        // the next interval's controls, timestep and their tangents are requested before this interval's products
        const long long tn = t + 1 < t1 ? t + 1 : t;
        const double* __restrict__ zn = Z + tn * P.zdim;
        const double av_n = m > 0 ? zn[P.off_a + kl] : 0.0;
        double h_n = h;                     // a fixed timestep stays where it is: no scalar pair held for it across the loop
        if (ft) h_n = zn[P.off_dt];
        double vav_n = 0.0, vh_n = 0.0;
        if (hasv) {
            const double* __restrict__ vzn = vZ + tn * P.zdim;
            if (m > 0) vav_n = vzn[P.off_a + kl];
            if (ft) vh_n = vzn[P.off_dt];
        }
        const double cl = pk[0], vcl = pk[64];
        const double al = av * cl;
        const double ald = fma(vav, cl, av * vcl);
        v4d Y[2][2], Yd[2][2];
        generator_pair(P.img, m, al, ald, base, bdl, lane, Y, Yd);
        const int sq = squarings(Y, h);      // the rule of the forward kernel: one function; the tangent has no say
        const double hs = h * ldexp(1.0, -sq), vhs = vh * ldexp(1.0, -sq);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Yd[q >> 1][q & 1][r] = fma(vhs, Y[q >> 1][q & 1][r], hs * Yd[q >> 1][q & 1][r]);
            Y[q >> 1][q & 1] = hs * Y[q >> 1][q & 1];
        }
        // Horner on the pair: Rdot_k = Ydot R_k+1 + Y Rdot_k+1,  R_k = Y R_k+1 + I/(k-1)!
        v4d R[2][2], Rd[2][2];
        exp_pair(scr, Y, Yd, sq, IdB, g, j, R, Rd);
        transpose4(scr, R, Y, g, j);
        transpose4(scr, Rd, Yd, g, j);
        vstep(Y, Yd, W, Wd, zero);
        av = av_n;
        h = h_n;
        vav = vav_n;
        vh = vh_n;
    }
    // two column-major 32 x 32 matrices: entry (16 I + 4 r + g, 16 J + j) of W, then of Wdot
    typedef __attribute__((address_space(1))) double gdouble;      // a global address: the stores stay global stores
    gdouble* __restrict__ o = (gdouble*)__double_as_longlong(pk[128]);
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int J = 0; J < 2; ++J)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o[(16 * J) * 32 + 16 * I + 4 * r] = W[I][J][r];
                o[1024 + (16 * J) * 32 + 16 * I + 4 * r] = Wd[I][J][r];
            }
}

}  // namespace

int qc_sweep32_jvp_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dvZ,
                                 const double* dvtheta, const double* dvscale, hipStream_t st, int64_t* chunk_out, int64_t* n_chunks_out) {
    SweepParams P;
    if (int rc = qc_sweep_plan_totals(h, S, h->dTotJ, 2048, &P, chunk_out, n_chunks_out)) return rc;
    hipLaunchKernelGGL(qc_sweep32_jvp_kernel, dim3(qc_sweep_grid(P, kJW)), dim3(64 * kJW), 0, st, P, dZ, dtheta, dscale, dvZ, dvtheta, dvscale, h->dTotJ.p);
    return QC_OK;
}
