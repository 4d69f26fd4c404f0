// Sweep Hessian products for "mfma32-sweep" handles (16 < 2N <= 32) made with QC_SWEEP_WIDE_HESSIAN in `wide`: the backward walk of
// qc_sweep_hvp.hip (read its header first: the recurrences, the differentiated antisymmetry identities, the series degree) with every
// matrix 2 x 2 tiles of 16 x 16, as qc_sweep32_grad.hip is qc_sweep_grad.hip on such tiles.  The chunk-end states come from
// load_state and the timestep's product from dot_tiles; KT, ZT, the chains and the contraction carry their tangents beside them: written out.
//
// Launches of one call on such a handle (qc_sweep_hvp_launch of qc_sweep_hvp.hip routes here):
//   1. qc_sweep32_jvp_kernel (qc_sweep32_jvp.hip, unchanged, through qc_sweep32_jvp_launch_totals): W_c and Wdot_c as two column-major
//      32 x 32 matrices, 2048 doubles per (sample, chunk) in h->dTotJ.  The handle does not need QC_SWEEP_WIDE_TANGENT for it.
//   2. qc_sweep32_hvp_seed_kernel (qc_sweep_hvp.hip: the seed of that file at ld = 32): x, xdot, lambda, lambdadot at every chunk end,
//      with tgrad_init the step to c = 0.
//   3. qc_sweep32_hvp_kernel, one wavefront per (sample, chunk), four per workgroup, never synchronised, the chunk walked backwards by
//      the rule of qc_sweep_chunks.  X[I][J] is the tile of rows 16 I .. and columns 16 J ..; the four states are 32 x <= 16: two tiles
//      each.  Tile conventions as qc_sweep32_grad.hip (a D-layout tile read as the A operand is its transpose).  Per interval:
//        Ga, Gadot          one pass over the images: drift, perturbations (theta, vtheta), drives (a c, va c + a vc).  Nothing is
//                           resident, the sample's base matrix and its tangent included: see "Registers".  The Ga chain is
//                           base_matrix's followed by generator's, fma for fma, so sq is the forward kernels'
//        sq                 from ||h Ga||_1 by qc_sweep32::squarings; no tangent enters it
//        KT = lambda x^T,  KTdot = lambdadot x^T + lambda xdot^T       eight tiles transposed in two LDS round trips of four   48 MFMAs
//        gdot_h = -sum (KTdot . Ga + KT . Gadot)
//        Y = (h / 2^sq) Ga,  Ydot = (vh / 2^sq) Ga + (h / 2^sq) Gadot,  dY = (h / 2^sq) K,  dYdot = (vh / 2^sq) K + (h / 2^sq) Kdot
//        Horner, k = 10 .. 1, on the quadruple, one tile column at a time, in place (column J of the four results needs column J of the
//        four operands only), nine products a step on eight accumulator tiles, eight independent chains:                   10 x 288
//            R <- Y R + I/(k-1)!,  Rdot <- Ydot R + Y Rdot,  dR <- dY R + Y dR,  dRdot <- dYdot R + dY Rdot + Ydot dR + Y dRdot
//        per squaring the same nine products with the transposed quadruple (sixteen tiles, four LDS round trips) as left factors  288
//        ZT = E^T dE,  ZTdot = Edot^T dE + E^T dEdot                                                                               96
//        gdot_k = vc_k sum ZT . G_k + c_k sum ZTdot . G_k        the drive images read again, 2 m wave sums
//        xdot <- Edot^T x + E^T xdot, x <- E^T x, and lambda, lambdadot alike                                                      96
//      and one vector store per interval (lane k: drive k, lane m: the timestep).
//      MFMAs per interval: 48 + 10 x 288 + 288 sq + 96 + 96 = 3120 + 288 sq, against the wide gradient walk's 848 + 96 sq; the tangent
//      totals of launch 1 add 864 + 96 sq.
//   4. qc_sweep_vjp_reduce_kernel (qc_sweep_vjp.hip, unchanged, through qc_sweep_launch_plain_sum).
// No atomics, sums in a fixed order: repeated calls return the same bits, and no output's bits depend on which others were asked for.  A
// NULL direction is read as zeros through the same arithmetic.  A non-finite vtheta[s], vscale[s], cot[s] or vcot[s] stays inside
// sample s: a wave touches one sample, and the number of squarings never depends on a direction.
//
// Series degree: 10, with this file's own 1/k! table (qc_sweep_hvp.hip, "Series degree"); kDeg = 8 of qc_sweep_common.h is everyone else's.
//
// Registers.  At 8 VGPRs a tile the Horner loop holds the four left factors (128), the quadruple (128), the eight column accumulators
// (64) and the four states (64): 384 of the 512 registers a lane of one wave per SIMD (VGPRs + AGPRs).  The sample's base matrix and its
// tangent (64 more) are NOT kept: both are formed again every interval from the images -- 1 + p + m reads of 8 KiB that hit L2, against
// some 3000 MFMAs.  Written with scalar index arithmetic the walk spilled 18 scalar registers; with the per-lane addresses in vector
// registers, 12 vector ones.  What it is now: the lane's addresses (its control and the timestep in Z and in vZ, its place in the output)
// and their strides walk down in vector registers; lane q holds theta[s, q] and vtheta[s, q]; those two, c[s, k] and vc[s, k] wait in
// the wave's LDS slice behind the transposition tiles (each lane its own slot, no barrier); the interval's controls and timesteps are
// read where they are used, not one interval ahead; the lane index and m are taken through opaque copies per interval, as in the
// other walks of the family.  gfx950 cross-compile: 256 VGPRs + 250 AGPRs, 100 SGPRs, 43008 B LDS (four waves); no private segment, no
// spills.
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_sweep32_common.h"
#include "qc_sweep32_walk.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep32;

constexpr int kHDeg = 10;           // qc_sweep_hvp.hip, "Series degree": this form's own degree and table as well

// 1 / k!, k = 0 .. 10
__constant__ const double kHInvFact[kHDeg + 1] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0,
                                                  1.0 / 40320.0, 1.0 / 362880.0, 1.0 / 3628800.0};

// G = G_drift + sum_q theta_q P_q + sum_u al_u G_u and Gd = sum_q vtheta_q P_q + sum_u ald_u G_u in A layout, from one pass over the
// images.  The G chain is base_matrix's followed by generator's (qc_sweep32_common.h): the same fma on the same operands in the same order.
// Lane q of thl / vthl holds theta[s, q] / vtheta[s, q], lane u of al / ald the scaled amplitude of drive u and its tangent.
__device__ __forceinline__ void generator_pair_images(const double* __restrict__ img, int m, int p, double thl, double vthl, double al, double ald,
                                                      int lane, v4d (&G)[2][2], v4d (&Gd)[2][2]) {
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        G[q >> 1][q & 1] = load_image_tile(img + q * 256, lane);
        Gd[q >> 1][q & 1] = zero;
    }
#pragma unroll 1
    for (int q = 0; q < p; ++q) {
        const double a = bcast_lane(thl, q);
        const double ad = bcast_lane(vthl, q);
        const double* __restrict__ Pq = img + (size_t)(1 + m + q) * 1024;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const v4d t4 = load_image_tile(Pq + u * 256, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                G[u >> 1][u & 1][r] = fma(a, t4[r], G[u >> 1][u & 1][r]);
                Gd[u >> 1][u & 1][r] = fma(ad, t4[r], Gd[u >> 1][u & 1][r]);
            }
        }
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

// Column J of the quadruple (R, Rd, dR, dRd) <- the nine products with the left factors (A, Ad, dA, dAd), in place:
//     R <- A R + C,  Rd <- Ad R + A Rd,  dR <- dA R + A dR,  dRd <- dAd R + dA Rd + Ad dR + A dRd
// a Horner step (A = Y ..., C = I / (k-1)!) or a squaring (A = E ..., C = 0); C given by its tiles of that column.  Eight accumulator
// tiles, eight chains, interleaved; 144 MFMAs.
__device__ __forceinline__ void hcol(const v4d (&A)[2][2], const v4d (&Ad)[2][2], const v4d (&dA)[2][2], const v4d (&dAd)[2][2], v4d (&R)[2][2],
                                     v4d (&Rd)[2][2], v4d (&dR)[2][2], v4d (&dRd)[2][2], int J, const v4d& c0, const v4d& c1) {
    const v4d z = {0.0, 0.0, 0.0, 0.0};
    v4d r0 = c0, r1 = c1, rd0 = z, rd1 = z, dr0 = z, dr1 = z, q0 = z, q1 = z;
#pragma unroll
    for (int K = 0; K < 2; ++K) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            q0 = __builtin_amdgcn_mfma_f64_16x16x4f64(dAd[0][K][kk], R[K][J][kk], q0, 0, 0, 0);
            q1 = __builtin_amdgcn_mfma_f64_16x16x4f64(dAd[1][K][kk], R[K][J][kk], q1, 0, 0, 0);
            rd0 = __builtin_amdgcn_mfma_f64_16x16x4f64(Ad[0][K][kk], R[K][J][kk], rd0, 0, 0, 0);
            rd1 = __builtin_amdgcn_mfma_f64_16x16x4f64(Ad[1][K][kk], R[K][J][kk], rd1, 0, 0, 0);
            dr0 = __builtin_amdgcn_mfma_f64_16x16x4f64(dA[0][K][kk], R[K][J][kk], dr0, 0, 0, 0);
            dr1 = __builtin_amdgcn_mfma_f64_16x16x4f64(dA[1][K][kk], R[K][J][kk], dr1, 0, 0, 0);
            r0 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[0][K][kk], R[K][J][kk], r0, 0, 0, 0);
            r1 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[1][K][kk], R[K][J][kk], r1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int K = 0; K < 2; ++K) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            q0 = __builtin_amdgcn_mfma_f64_16x16x4f64(dA[0][K][kk], Rd[K][J][kk], q0, 0, 0, 0);
            q1 = __builtin_amdgcn_mfma_f64_16x16x4f64(dA[1][K][kk], Rd[K][J][kk], q1, 0, 0, 0);
            rd0 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[0][K][kk], Rd[K][J][kk], rd0, 0, 0, 0);
            rd1 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[1][K][kk], Rd[K][J][kk], rd1, 0, 0, 0);
            dr0 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[0][K][kk], dR[K][J][kk], dr0, 0, 0, 0);
            dr1 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[1][K][kk], dR[K][J][kk], dr1, 0, 0, 0);
            q0 = __builtin_amdgcn_mfma_f64_16x16x4f64(Ad[0][K][kk], dR[K][J][kk], q0, 0, 0, 0);
            q1 = __builtin_amdgcn_mfma_f64_16x16x4f64(Ad[1][K][kk], dR[K][J][kk], q1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int K = 0; K < 2; ++K) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            q0 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[0][K][kk], dRd[K][J][kk], q0, 0, 0, 0);
            q1 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[1][K][kk], dRd[K][J][kk], q1, 0, 0, 0);
        }
    }
    R[0][J] = r0;
    R[1][J] = r1;
    Rd[0][J] = rd0;
    Rd[1][J] = rd1;
    dR[0][J] = dr0;
    dR[1][J] = dr1;
    dRd[0][J] = q0;
    dRd[1][J] = q1;
}

__device__ __forceinline__ void hstep(const v4d (&A)[2][2], const v4d (&Ad)[2][2], const v4d (&dA)[2][2], const v4d (&dAd)[2][2], v4d (&R)[2][2],
                                      v4d (&Rd)[2][2], v4d (&dR)[2][2], v4d (&dRd)[2][2], const v4d& cI) {
    const v4d z = {0.0, 0.0, 0.0, 0.0};
    hcol(A, Ad, dA, dAd, R, Rd, dR, dRd, 0, cI, z);
    hcol(A, Ad, dA, dAd, R, Rd, dR, dRd, 1, z, cI);
}

// (v, vd) <- (M^T v, Md^T v + M^T vd) for D-layout M, Md and two-tile column blocks: y_I = sum_K M[K][I]^T v_K (vapplyT) and its tangent
__device__ __forceinline__ void happlyT(const v4d (&M)[2][2], const v4d (&Md)[2][2], v4d (&v)[2], v4d (&vd)[2]) {
    const v4d z = {0.0, 0.0, 0.0, 0.0};
    v4d y0 = z, y1 = z, d0 = z, d1 = z;
#pragma unroll
    for (int K = 0; K < 2; ++K) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            d0 = __builtin_amdgcn_mfma_f64_16x16x4f64(Md[K][0][kk], v[K][kk], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f64_16x16x4f64(Md[K][1][kk], v[K][kk], d1, 0, 0, 0);
            y0 = __builtin_amdgcn_mfma_f64_16x16x4f64(M[K][0][kk], v[K][kk], y0, 0, 0, 0);
            y1 = __builtin_amdgcn_mfma_f64_16x16x4f64(M[K][1][kk], v[K][kk], y1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int K = 0; K < 2; ++K) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            d0 = __builtin_amdgcn_mfma_f64_16x16x4f64(M[K][0][kk], vd[K][kk], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f64_16x16x4f64(M[K][1][kk], vd[K][kk], d1, 0, 0, 0);
        }
    }
    v[0] = y0;
    v[1] = y1;
    vd[0] = d0;
    vd[1] = d1;
}

constexpr int kHSl = kScr + 4 * 64;      // doubles of LDS a wave: the transposition tiles; behind them four values a lane

// One wavefront per (sample, chunk), walking the chunk backwards: the wide gradient walk with every product differentiated beside itself.
// xs / ls: x and lambda at the chunk ends, xts / lts: their tangents; tgs: S x (T-1) x nd.
__global__ __launch_bounds__(64 * kWaves) void qc_sweep32_hvp_kernel(const SweepParams P, const double* __restrict__ Z, const double* __restrict__ theta,
                                                                      const double* __restrict__ scale, const double* __restrict__ vZ,
                                                                      const double* __restrict__ vtheta, const double* __restrict__ vscale,
                                                                      const double* __restrict__ xs, const double* __restrict__ ls,
                                                                      const double* __restrict__ xts, const double* __restrict__ lts,
                                                                      double* __restrict__ tgs) {
    __shared__ double scr_all[kWaves * kHSl];
    const WaveItem w = wave_item(kWaves);
    double* __restrict__ scr = scr_all + w.wq * kHSl;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    // ---- once per wave: the lane's factors, the four states at the chunk's end, the lane's address in the output ---------------------
    // lane l holds the sample's factor of drive min(l, m-1) and its tangent
    const int kl = lane < m ? lane : (m > 0 ? m - 1 : 0);
    // and theta[s, min(l, p-1)] and its tangent: the generator reads them lane by lane.  The four values wait in the wave's LDS slice
    // behind the transposition tiles, each lane's own slot (no barrier): read once per interval, they would otherwise hold eight
    // registers across the Horner loop, which has none to spare (as pk in qc_sweep32_jvp_kernel)
    double* __restrict__ pk = scr + kScr + lane;
    {
        const int kq = lane < P.p ? lane : (P.p > 0 ? P.p - 1 : 0);
        pk[0] = (scale && m > 0) ? scale[s * m + kl] : 1.0;
        pk[64] = (vscale && m > 0) ? vscale[s * m + kl] : 0.0;
        pk[128] = P.p > 0 ? theta[s * P.p + kq] : 0.0;
        pk[192] = (vtheta && P.p > 0) ? vtheta[s * P.p + kq] : 0.0;
    }

    v4d x[2], xd[2], lam[2], lamd[2];
    {
        const int ns = P.n * P.nc;
        load_state(xs + item * ns, P.n, P.nc, g, j, x);
        load_state(ls + item * ns, P.n, P.nc, g, j, lam);
        load_state(xts + item * ns, P.n, P.nc, g, j, xd);
        load_state(lts + item * ns, P.n, P.nc, g, j, lamd);
    }
    // What the loop reads and writes per lane walks down in vector registers (as cp and op in qc_sweep32_noise_grad_kernel): the lane's
    // control and the timestep in Z, the same two in vZ (null without one), the lane's address in tgs, and their strides.  The loop keeps
    // no scalar for any of them.  Without drives ap rests on the knot's first entry, without a free timestep hp does: read, never used.
    typedef __attribute__((address_space(1))) double gdouble;      // global addresses: the loads and the store stay global ones
    const double* __restrict__ z = Z + (long long)(t1 - 1) * P.zdim;
    const double* ap = z + (m > 0 ? P.off_a + kl : 0);
    const double* hp = z + (ft ? P.off_dt : 0);
    const double* vap = nullptr;
    const double* vhp = nullptr;
    if (vZ) {
        vap = vZ + (ap - Z);
        vhp = vZ + (hp - Z);
    }
    double* gp = tgs + (s * P.n_int + (t1 - 1)) * P.nd + lane;
    int zstr = P.zdim, gstr = P.nd, ftv = P.off_dt;
    asm volatile("" : "+v"(ap), "+v"(hp), "+v"(vap), "+v"(vhp), "+v"(gp), "+v"(zstr), "+v"(gstr), "+v"(ftv));

    const double hfix = P.dt_fixed;
#pragma unroll 1
    for (int t = t1 - 1; t >= t0; --t) {
        // The interval's controls, timestep and their tangents are read where they are used, not one interval ahead as in the shorter
        // walks: an interval is some 3000 MFMAs, the reads are a handful, and values requested ahead would hold eight registers across
        // the Horner loop.
        const double av = *(const gdouble*)ap;
        double h = hfix;
        if (ftv >= 0) h = *(const gdouble*)hp;
        double vav = 0.0, vh = 0.0;
        if (vap) {
            vav = *(const gdouble*)vap;
            if (ftv >= 0) vh = *(const gdouble*)vhp;
            vap -= zstr;
            vhp -= zstr;
        }
        ap -= zstr;
        hp -= zstr;
        const double cl = pk[0], vcl = pk[64];
        const double al = av * cl;
        const double ald = fma(vav, cl, av * vcl);
        // opaque copies of m and of the lane index: the compares below are made per interval instead of living in scalar registers
        // across the loop (as in qc_sweep_hvp_kernel)
        int mu = m;
        asm volatile("" : "+s"(mu));
        int ln = lane;
        asm volatile("" : "+v"(ln));
        v4d Y[2][2], Yd[2][2], dY[2][2], dYd[2][2];
        {
            // the image buffer's address is taken anew where it is used: no derived address is kept across the interval
            const double* __restrict__ img = P.img;
            asm volatile("" : "+s"(img));
            generator_pair_images(img, mu, P.p, pk[128], pk[192], al, ald, ln, Y, Yd);
        }
        const int sq = squarings(Y, h);      // the rule of the forward kernel: one function; no tangent has a say
        const double sc = ldexp(1.0, -sq);
        const double hs = h * sc, vhs = vh * sc;
        // KT = lambda x^T of knot t+1 (D layout) and its tangent, from the transposed tiles of the four states; dY in A layout is KT with the
        // block index swapped: dY(I, K) = KT[K][I]
        {
            v4d tx[4], tl[4];
            {
                const v4d in[4] = {x[0], x[1], xd[0], xd[1]};
                lds_transpose16_multi<4>(scr, in, tx, g, j);
            }
            {
                const v4d in[4] = {lam[0], lam[1], lamd[0], lamd[1]};
                lds_transpose16_multi<4>(scr, in, tl, g, j);
            }
#pragma unroll
            for (int I = 0; I < 2; ++I)
#pragma unroll
                for (int J = 0; J < 2; ++J) {
                    v4d k = zero, kd = zero;
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        k = __builtin_amdgcn_mfma_f64_16x16x4f64(tl[I][kk], tx[J][kk], k, 0, 0, 0);
                        kd = __builtin_amdgcn_mfma_f64_16x16x4f64(tl[2 + I][kk], tx[J][kk], kd, 0, 0, 0);
                    }
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) kd = __builtin_amdgcn_mfma_f64_16x16x4f64(tl[I][kk], tx[2 + J][kk], kd, 0, 0, 0);
                    dY[J][I] = k;
                    dYd[J][I] = kd;
                }
        }
        double out = 0.0;
        if (ftv >= 0) {
            // sum_IJ (KTd[I][J] . Ga[J][I] + KT[I][J] . Gad[J][I]) = sum_IK (dYd(I, K) . Ga(I, K) + dY(I, K) . Gad(I, K))
            const double dhd = -wave_sum(dot_tiles(dY, Yd, dot_tiles(dYd, Y, 0.0)));
            out = ln == mu ? dhd : out;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Yd[q >> 1][q & 1][r] = fma(vhs, Y[q >> 1][q & 1][r], hs * Yd[q >> 1][q & 1][r]);
                dYd[q >> 1][q & 1][r] = fma(vhs, dY[q >> 1][q & 1][r], hs * dYd[q >> 1][q & 1][r]);
            }
            Y[q >> 1][q & 1] = hs * Y[q >> 1][q & 1];
            dY[q >> 1][q & 1] = hs * dY[q >> 1][q & 1];
        }
        v4d R[2][2] = {{kHInvFact[kHDeg] * IdB, zero}, {zero, kHInvFact[kHDeg] * IdB}};
        v4d Rd[2][2] = {{zero, zero}, {zero, zero}};
        v4d dR[2][2] = {{zero, zero}, {zero, zero}};
        v4d dRd[2][2] = {{zero, zero}, {zero, zero}};
#pragma unroll 1
        for (int k = kHDeg; k >= 1; --k) hstep(Y, Yd, dY, dYd, R, Rd, dR, dRd, kHInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            transpose4(scr, R, Y, g, j);           // E, Edot, dE, dEdot in A layout; the four left factors are free from here on
            transpose4(scr, Rd, Yd, g, j);
            transpose4(scr, dR, dY, g, j);
            transpose4(scr, dRd, dYd, g, j);
            hstep(Y, Yd, dY, dYd, R, Rd, dR, dRd, zero);
        }
        // ZT = E^T dE into Y, ZTdot = Edot^T dE + E^T dEdot into Yd
#pragma unroll
        for (int J = 0; J < 2; ++J) {
            v4d z0 = zero, z1 = zero, w0 = zero, w1 = zero;
#pragma unroll
            for (int K = 0; K < 2; ++K) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    w0 = __builtin_amdgcn_mfma_f64_16x16x4f64(Rd[K][0][kk], dR[K][J][kk], w0, 0, 0, 0);
                    w1 = __builtin_amdgcn_mfma_f64_16x16x4f64(Rd[K][1][kk], dR[K][J][kk], w1, 0, 0, 0);
                    z0 = __builtin_amdgcn_mfma_f64_16x16x4f64(R[K][0][kk], dR[K][J][kk], z0, 0, 0, 0);
                    z1 = __builtin_amdgcn_mfma_f64_16x16x4f64(R[K][1][kk], dR[K][J][kk], z1, 0, 0, 0);
                }
            }
#pragma unroll
            for (int K = 0; K < 2; ++K) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    w0 = __builtin_amdgcn_mfma_f64_16x16x4f64(R[K][0][kk], dRd[K][J][kk], w0, 0, 0, 0);
                    w1 = __builtin_amdgcn_mfma_f64_16x16x4f64(R[K][1][kk], dRd[K][J][kk], w1, 0, 0, 0);
                }
            }
            Y[0][J] = z0;
            Y[1][J] = z1;
            Yd[0][J] = w0;
            Yd[1][J] = w1;
        }
        {
            const double* __restrict__ imgc = P.img;
            asm volatile("" : "+s"(imgc));
#pragma unroll 1
            for (int u = 0; u < mu; ++u) {
                const double* __restrict__ Gu = imgc + (size_t)(1 + u) * 1024;
                double pu = 0.0, pud = 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const v4d t4 = load_image_tile(Gu + q * 256, ln);       // tile (J, I) = q against ZT[I][J]
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        pu = fma(Y[q & 1][q >> 1][r], t4[r], pu);
                        pud = fma(Yd[q & 1][q >> 1][r], t4[r], pud);
                    }
                }
                const double du = wave_sum(pu);
                const double dud = wave_sum(pud);
                out = ln == u ? fma(dud, pk[0], du * pk[64]) : out;
            }
        }
        if (ln < gstr) *(gdouble*)gp = out;
        gp -= gstr;
        happlyT(R, Rd, x, xd);
        happlyT(R, Rd, lam, lamd);
    }
}

}  // namespace

void qc_sweep32_hvp_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dvZ,
                                const double* dvtheta, const double* dvscale, int64_t chunk, int64_t n_chunks, double* tgs, hipStream_t st) {
    const SweepParams P = qc_sweep_params(h, S, chunk, n_chunks);
    const unsigned grid = qc_sweep_grid(P, kWaves);
    hipLaunchKernelGGL(qc_sweep32_hvp_kernel, dim3(grid), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale, dvZ, dvtheta, dvscale,
                       (const double*)h->dXs.p, (const double*)h->dLs.p, (const double*)h->dXsT.p, (const double*)h->dLsT.p, tgs);
}
