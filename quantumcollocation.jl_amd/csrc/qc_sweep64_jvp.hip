// Sweep pushforwards for "mfma64-sweep" handles (32 < 2N <= 64) made with QC_SWEEP_WIDE_64_TANGENT in `wide`: qc_sweep_jvp_kernel
// (qc_sweep_jvp.hip; read its header first for the mathematics, which is not restated) with every matrix 4 x 4 tiles of 16 x 16 in LDS, as
// qc_sweep64.hip is qc_sweep.hip on such tiles.  Nothing is reversed: Lindblad generators are served like any others (N = 25, 2N = 50).
//
// Work item, chunk rule (kSweepFill64), thread-to-element map, base-matrix and generator code are qc_sweep_mfma64_kernel's
// (qc_sweep64_common.h): one WORKGROUP of 1024 threads per (sample, chunk), wave w owns tile (I, J) = (w & 3, w >> 2) of every product.
// Per interval:
//   once per item   Bdot = sum_j vtheta[s,j] P_j, four doubles a thread beside the base matrix; the lane's vc[s,k] beside c[s,k]
//   coefficients    al = a c,  aldot = va c + a vc
//   generators      Ga = base + sum al_u G_u,  Gadot = Bdot + sum aldot_u G_u      one pass over the drive images (generator_pair: the Ga
//                   chain is `generator`'s, the same fma on the same operands in the same order)
//   squarings       sq from ||h Ga||_1 by squarings(); the tangent never influences it
//   scaled          Y = (h 2^-sq) Ga,  Ydot = (vh 2^-sq) Ga + (h 2^-sq) Gadot
//   Horner          R' = Y R + I/(k-1)!,  Rdot' = Ydot R + Y Rdot                                    8 x 3 products
//   per squaring    E' = E E,  Edot' = E Edot + Edot E                                               3 products
//   totals          W' = E W,  Wdot' = E Wdot + Edot W                                               3 products
// (27 + 3 sq) x 256 MFMAs per interval and workgroup against the forward kernel's (9 + sq) x 256: 3.0 forward sweeps by the count.  Every
// R, E and W product is one chain of 16 MFMAs over ascending k on row fragment I of the left factor and column fragment J of the right one
// from the accumulator c I (chain_pair): tile_mul's chain, MFMA for MFMA, on operands formed by the forward kernel's expressions -- W
// carries its bits.  The tangent's two products share the pass: four fragment reads feed three MFMAs, where tile_mul reads two for one.
//
// LDS.  Six matrices (Y, Ydot, R, Rdot, W, Wdot) are 202 752 B; the kernel lives in the forward kernel's four slots, 135 168 B dynamic +
// 128 B static of the CU's 160 KiB, one workgroup per CU:
//     A | Ad | R | Rd            A, Ad hold Y, Ydot during Horner and W, Wdot from the last Horner step to the end of the interval
//   (b) of qc_sweep64_grad.hip: R, Rdot (later E, Edot) are updated IN PLACE -- a wave holds its new tiles in registers across a barrier
//       (every read of the old ones is done), writes them over the old ones, and a second barrier publishes them;
//   W and Wdot spend Horner and the squarings PARKED in registers: a wave's tile of each is 4 doubles a lane.  The last Horner step has read
//       Y, Ydot for the last time in front of its barrier P; behind it each wave stores its parked tiles into A, Ad next to its new R, Rdot
//       tiles, and that step's barrier Wb publishes all four.  The squarings read R, Rd only.  The totals read E, Edot as row fragments and
//       W, Wdot as column fragments, and their results stay in registers: the next interval's parked tiles.
// Barriers of one interval, in order, and what each stands between:
//     S   inside squarings(): behind it every wave has left the previous interval's three totals products -- the last reads of A, Ad, R, Rd,
//         the only products with no barrier of their own behind them.  Y, Ydot, R = I/8!, Rdot = 0 are written behind S.  S also stands
//         between red[]'s writes and reads; the 17 or more barriers that follow stand between those reads and the next interval's writes.
//     H0  publishes Y, Ydot, R, Rdot.
//     per Horner step k = 8 .. 1:   the three products into registers (read A, Ad, R, Rd)
//     P   every read of R, Rd of this step is done (at k = 1: of A, Ad as well);   R <- R', Rd <- Rdot'   (k = 1: A <- W, Ad <- Wdot)
//     Wb  publishes R, Rd (k = 1: and A, Ad)
//     per squaring:   the three products into registers (read R, Rd);  P;  R <- E', Rd <- Edot';  Wb      (the same two barriers)
//     totals:   W' = E W, Wdot' = E Wdot + Edot W into registers (read R, Rd, A, Ad); the overwriting writes are behind the next S.
// After the chunk's last interval each wave stores its tiles of W, then Wdot, from registers: two column-major 64 x 64 matrices (stride
// 64), S x n_chunks x 8192 doubles of h->dTotJ; qc_sweep64_jvp_finish_kernel (qc_sweep_jvp.hip) chains them with ld = 64.  No LDS is read
// or written behind the last totals, so no barrier follows them.  No atomics, every sum in a fixed order: repeated calls give the same bits.
// A NULL direction is read as zeros through the same arithmetic.
//
// gfx950 cross-compile: DESIGN.md 5.8.14 (1024 threads, no private segment, no spills).
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_side.h"
#include "qc_sweep64_common.h"
#include "qc_sweep64_launch.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep64;

// the thread's four elements of Bdot = sum_q vtheta[s, q] P_q, by fma in perturbation order (vtheta NULL: zeros)
__device__ __forceinline__ void based_elems(const double* img, int m, int p, const double* __restrict__ vtheta, long long s, int tid,
                                            double (&based)[4]) {
    const gptr G0 = (gptr)(unsigned long long)img + tid;
#pragma unroll
    for (int e = 0; e < 4; ++e) based[e] = 0.0;
    for (int q = 0; q < p; ++q) {
        const double vth = vtheta ? vtheta[s * p + q] : 0.0;
        const gptr Pq = G0 + (size_t)(1 + m + q) * kImg;
#pragma unroll
        for (int e = 0; e < 4; ++e) based[e] = fma(vth, Pq[1024 * e], based[e]);
    }
}

// G = base + sum_u al_u G_u and Gd = based + sum_u ald_u G_u from one pass over the drive images.  The G chain is qc_sweep64::generator's:
// the same fma on the same operands in the same order, so G carries its bits.
__device__ __forceinline__ void generator_pair(const double* img, int m, double al, double ald, const double (&base)[4], const double (&based)[4],
                                               int tid, double (&G)[4], double (&Gd)[4]) {
    const gptr G0 = (gptr)(unsigned long long)img + tid;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        G[e] = base[e];
        Gd[e] = based[e];
    }
#pragma unroll 1
    for (int u = 0; u < m; ++u) {
        const double a = bcast_lane(al, u);
        const double ad = bcast_lane(ald, u);
        const gptr Gu = G0 + (size_t)(1 + u) * kImg;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double gu = Gu[1024 * e];
            G[e] = fma(a, gu, G[e]);
            Gd[e] = fma(ad, gu, Gd[e]);
        }
    }
}

// One tile of a product and of its tangent from one pass over k: P = A B + c0, Pd = Ad B + A Bd.  pa, pad: row fragments I of A, Ad; pb, pbd:
// column fragments J of B, Bd.  The P chain is tile_mul's (ascending k, the same operands); each fragment is read once for the three MFMAs
// of its step.
__device__ __forceinline__ void chain_pair(const double* __restrict__ pa, const double* __restrict__ pad, const double* __restrict__ pb,
                                           const double* __restrict__ pbd, v4d& P, v4d& Pd) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const double a = pa[q * kRowStep], ad = pad[q * kRowStep], b = pb[q * kColStep], bd = pbd[q * kColStep];
        P = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, P, 0, 0, 0);
        Pd = __builtin_amdgcn_mfma_f64_16x16x4f64(ad, b, Pd, 0, 0, 0);
        Pd = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bd, Pd, 0, 0, 0);
    }
}

__global__ __launch_bounds__(kThreads, 1) void qc_sweep64_jvp_kernel(const SweepParams P, const double* __restrict__ Z, const double* __restrict__ theta,
                                                                       const double* __restrict__ scale, const double* __restrict__ vZ,
                                                                       const double* __restrict__ vtheta, const double* __restrict__ vscale,
                                                                       double* __restrict__ tot) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double red[16];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, j = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), I = w & 3, J = w >> 2;
    const long long item = blockIdx.x;
    const ChunkRange ch = chunk_range(item, P.n_chunks, P.chunk, P.n_int);
    const int t0 = ch.t0, t1 = ch.t1, m = P.m;
    const long long s = ch.s;
    const bool ft = P.off_dt >= 0;
    const bool hasv = vZ != nullptr;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    double* const Ab = sm;                  // Y, then W
    double* const Adb = sm + kMat;          // Ydot, then Wdot
    double* const Rb = sm + 2 * kMat;
    double* const Rdb = sm + 3 * kMat;

    // ---- once per item: the sample's base matrix and its tangent, W = I, Wdot = 0 (parked) -------------------------------------------
    double base[4], based[4];
    base_elems(P.img, m, P.p, theta, s, tid, base);
    based_elems(P.img, m, P.p, vtheta, s, tid, based);
    // lane l holds the sample's factor of drive min(l, m-1) and its tangent
    const DriveLane dl = drive_lane(scale, m, s, lane);
    const int kl = dl.kl;
    const double cl = dl.cl;
    const double vcl = (vscale && m > 0) ? vscale[s * m + kl] : 0.0;

    const double* __restrict__ z = Z + (long long)t0 * P.zdim;
    double av = drive_value(z, P.off_a, m, kl);
    const double hfix = opaque_scalar(P.dt_fixed);
    double h = ft ? z[P.off_dt] : hfix;
    double vav = 0.0, vh = 0.0;
    if (hasv) {
        const double* __restrict__ vz = vZ + (long long)t0 * P.zdim;
        if (m > 0) vav = vz[P.off_a + kl];
        if (ft) vh = vz[P.off_dt];
    }
    v4d W = I == J ? IdB : zero, Wd = zero;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        // the next interval's controls, timestep and their tangents are requested before this interval's products
        const long long tn = t + 1 < t1 ? t + 1 : t;
        const double* __restrict__ zn = Z + tn * P.zdim;
        const double av_n = drive_value(zn, P.off_a, m, kl);
        const double h_n = ft ? zn[P.off_dt] : hfix;
        double vav_n = 0.0, vh_n = 0.0;
        if (hasv) {
            const double* __restrict__ vzn = vZ + tn * P.zdim;
            if (m > 0) vav_n = vzn[P.off_a + kl];
            if (ft) vh_n = vzn[P.off_dt];
        }
        const double al = av * cl;
        const double ald = fma(vav, cl, av * vcl);
        double G[4], Gd[4];
        generator_pair(P.img, m, al, ald, base, based, tid, G, Gd);
        const int sq = squarings(red, G, h, lane, w);      // barrier S; the forward kernel's rule: the tangent has no say in sq
        const double sc = ldexp(1.0, -sq);
        const double hs = h * sc, vhs = vh * sc;
        // Horner on the pair: R_deg+1 = I/deg!, Rdot_deg+1 = 0;  R_k = Y R_k+1 + I/(k-1)!,  Rdot_k = Ydot R_k+1 + Y Rdot_k+1
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Ab[lds_at(tid, e)] = hs * G[e];
            Adb[lds_at(tid, e)] = fma(vhs, G[e], hs * Gd[e]);
            Rb[lds_at(tid, e)] = on_diagonal(tid, e) ? kInvFact[kDeg] : 0.0;
            Rdb[lds_at(tid, e)] = 0.0;
        }
        __syncthreads();      // H0
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) {
            v4d nR = I == J ? kInvFact[k - 1] * IdB : zero, nD = zero;
            chain_pair(row_frag(Ab, I, g, j), row_frag(Adb, I, g, j), col_frag(Rb, J, g, j), col_frag(Rdb, J, g, j), nR, nD);
            __syncthreads();      // P
            store_tile(Rb, I, J, g, j, nR);
            store_tile(Rdb, I, J, g, j, nD);
            if (k == 1) {         // Y, Ydot have been read for the last time: the parked tiles take their slots
                store_tile(Ab, I, J, g, j, W);
                store_tile(Adb, I, J, g, j, Wd);
            }
            __syncthreads();      // Wb
        }
#pragma unroll 1
        for (int q = 0; q < sq; ++q) {
            v4d nE = zero, nD = zero;
            chain_pair(row_frag(Rb, I, g, j), row_frag(Rdb, I, g, j), col_frag(Rb, J, g, j), col_frag(Rdb, J, g, j), nE, nD);
            __syncthreads();      // P
            store_tile(Rb, I, J, g, j, nE);
            store_tile(Rdb, I, J, g, j, nD);
            __syncthreads();      // Wb
        }
        // totals: Wdot <- E Wdot + Edot W, W <- E W; the new tiles stay in registers for the next interval
        {
            v4d nW = zero, nD = zero;
            chain_pair(row_frag(Rb, I, g, j), row_frag(Rdb, I, g, j), col_frag(Ab, J, g, j), col_frag(Adb, J, g, j), nW, nD);
            W = nW;
            Wd = nD;
        }
        av = av_n;
        h = h_n;
        vav = vav_n;
        vh = vh_n;
    }
    // W, then Wdot: column-major 64 x 64, lane (g, j) reg r holds element (16 I + 4 r + g, 16 J + j)
    double* __restrict__ o = tot + item * (2 * kImg) + (16 * J + j) * 64 + 16 * I + g;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        o[4 * r] = W[r];
        o[kImg + 4 * r] = Wd[r];
    }
}

}  // namespace

int qc_sweep64_jvp_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dvZ,
                                 const double* dvtheta, const double* dvscale, hipStream_t st, int64_t* chunk_out, int64_t* n_chunks_out) {
    SweepParams P;
    if (int rc = qc_sweep_plan_totals(h, S, h->dTotJ, 2 * kImg, &P, chunk_out, n_chunks_out)) return rc;
    QC_SWEEP64_LAUNCH(h, qc_sweep64_jvp_kernel, kLdsBytes, P, st, dZ, dtheta, dscale, dvZ, dvtheta, dvscale, h->dTotJ.p);
    return QC_OK;
}
