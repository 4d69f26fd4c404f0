// Open-system sweep gradients for "mfma32-sweep" handles (16 < 2N <= 32): the stored-state walk of qc_sweep_open_grad.hip with every matrix
// 2 x 2 tiles of 16 x 16.  The mathematics is that file's, line for line (read its header first): K = lambda_{t+1} x_t^T with x_t READ from the
// stored forward states, one paired chain per interval in the transposed frame (direction K^T = x_t lambda_{t+1}^T on the A-layout images of
// the forward kernel, dY = KT / 2^sq not scaled by h), ||hG||_1 <= 2^sq / 8 by qc_sweep32::squarings -- the one function the forward kernel,
// the store kernel and the walk call, so the stored states and the walk choose the same sq.  Nothing asks anything of the generators.
// Taken by handles whose descriptor has reserved1[0] = QC_SWEEP_STORED_STATES and wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_STORED (with
// QC_SWEEP_WIDE_PARAMS for the parameter flavour), for qc_sweep_grad*, qc_sweep_grad_params* and qc_sweep_vjp*, antisymmetric generators
// included; at most 16 state columns: the state and the adjoint are two tiles each.
//
// Launches (after the totals and the seed of the closed wide walk, which leave x and lambda at every chunk end in h->dXs / h->dLs):
//   A. qc_sweep32_open_store_kernel, one wavefront per (sample, chunk): from the chunk-start state (init, or the previous chunk's end) the
//      interval body of qc_sweep_mfma32_kernel with x <- E x in place of W <- E W; x_t of every knot t = t0 .. t1-1 goes to
//      h->dXall[s][t][2N x cols].  The chunk's last exponential is skipped.  MFMAs per interval: 8 x 32 + 32 sq + 16 = 272 + 32 sq.
//   B. qc_sweep32_open_grad_kernel<PAR>, one wavefront per (sample, chunk), backwards.  X[I][J] is the tile of rows 16 I .. and columns 16 J ..
//      (qc_sweep32_grad.hip: for a D-layout M the A operand (I, K) of M^T is the tile M[K][I] as it stands).  Per interval, lambda the two
//      D-layout tiles of knot t+1:
//        x_J^T                        read from dXall straight into the B-operand pattern (an index pattern, no LDS), two tiles
//        lambda_A                     one LDS round trip (two tiles)
//        KT[I][J] = lambda_I x_J^T    16 MFMAs; dY(I, K) = KT[K][I] / 2^sq acts as K^T / 2^sq
//        Y = h G / 2^sq, eight paired Horner steps (qc_sweep32_walk.h: vstep)                           8 x 96 MFMAs
//        sq paired squarings (E, dE) <- (E E, E dE + dE E)                                               96 MFMAs, two LDS round trips of four tiles
//        ZT = h dE;  dphi/da_k = c_k sum_IJ ZT[I][J] . G_k[J][I]      the drive images read again from the image buffer, as the closed walk
//                                                                     does; the same pass rebuilds G (Y held the transposed E since)
//        dphi/dh = sum_IJ dE[I][J] . G[J][I]                          wave sums in a fixed order
//        lambda <- E^T lambda                                         16 MFMAs
//      MFMAs per interval: 16 + 768 + 96 sq + 16 = 800 + 96 sq (closed wide walk: 848 + 96 sq): no E^T dE and no x <- E^T x.
//      PAR as qc_sweep32_grad_kernel<true>: Acc = sum_t ZT_t in LDS behind the transposition tiles, two waves a workgroup, the chunk's
//      shares to part[item][p + m], reduced by qc_sweep_par_reduce_kernel; gs may be NULL.  The per-interval values of both flavours are the
//      same operations on the same operands: the same bits.
// No atomics; every sum in a fixed order; no output's bits depend on which others were asked for.  Resources: DESIGN.md 5.8.7.
// The store kernel is built on drive_lane, load_state and exp_plain (qc_sweep32_common.h).  The walk restates drive_lane, load_state,
// exp_pair and, in <true>, the chunk end of qc_sweep32_grad_kernel<true>: the calls move the registers of <false>, and no bench times
// <true> ("Shared and restated in the wide kernels").  The work item is wave_item / chunk_range of qc_sweep_common.h.
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_sweep32_common.h"
#include "qc_sweep32_walk.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep32;

// v <- A v for an A-layout matrix and a two-tile column block (B / D layout)
__device__ __forceinline__ void xapply(const v4d (&A)[2][2], v4d (&v)[2]) {
    const v4d z = {0.0, 0.0, 0.0, 0.0};
    v4d y0 = z, y1 = z;
#pragma unroll
    for (int K = 0; K < 2; ++K) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            y0 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[0][K][kk], v[K][kk], y0, 0, 0, 0);
            y1 = __builtin_amdgcn_mfma_f64_16x16x4f64(A[1][K][kk], v[K][kk], y1, 0, 0, 0);
        }
    }
    v[0] = y0;
    v[1] = y1;
}

// x_t of every knot of the chunk, t = t0 .. t1-1, from the chunk-start state
__global__ __launch_bounds__(64 * kWaves, 2) void qc_sweep32_open_store_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                                 const double* __restrict__ theta, const double* __restrict__ scale,
                                                                                 const double* __restrict__ init, const double* __restrict__ xs,
                                                                                 double* __restrict__ xall) {
    __shared__ double scr_all[kWaves * kScr];
    const WaveItem w = wave_item(kWaves);
    double* __restrict__ scr = scr_all + w.wq * kScr;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, c = ch.c, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const int ns = P.n * P.nc;

    v4d base[2][2];
    base_matrix(P.img, m, P.p, theta, s, lane, base);
    const DriveLane dl = drive_lane(scale, m, s, lane);
    const int kl = dl.kl;
    const double cl = dl.cl;

    v4d x[2];
    {
        const double* __restrict__ x0 = c == 0 ? init : xs + (item - 1) * ns;      // the previous chunk's end: same sample, c >= 1
        load_state(x0, P.n, P.nc, g, j, x);
    }
    // the lane's control of the interval (lane l: drive min(l, m-1)) and, `dto` entries further, the timestep: one pointer walking up
    const double* ap = Z + (long long)t0 * P.zdim + P.off_a + kl;
    const int dto = P.off_dt - P.off_a - kl;
    double av = m > 0 ? ap[0] : 0.0;
    const double hfix = opaque_scalar(P.dt_fixed);
    double h = ft ? ap[dto] : hfix;
    // the lane's entries of a stored knot: tile I, reg r = x[16 I + 4 r + g][j] at xo[16 I + 4 r], xo the lane's own pointer to x[g][j], walking
    // up with t; bit 4 I + r of okm says whether the entry exists (a set bit implies g < n and j < cols: the pointer stays inside the knot).
    // The mask waits in a vector register: kept as eight lane masks it would fill the scalar registers across the loop.
    int okm = 0;
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
        for (int r = 0; r < 4; ++r) okm |= (16 * I + 4 * r + g < P.n && j < P.nc) ? (1 << (4 * I + r)) : 0;
    double* xo = xall + (s * P.n_int + t0) * ns + (okm ? g + P.n * j : 0);
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        {
            int ok = okm;
            asm volatile("" : "+v"(ok));
#pragma unroll
            for (int I = 0; I < 2; ++I)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if ((ok >> (4 * I + r)) & 1) xo[16 * I + 4 * r] = x[I][r];
            xo += ns;
        }
        if (t + 1 == t1) break;      // x_{t1} is the next chunk's start
        ap += P.zdim;
        const double av_n = m > 0 ? ap[0] : 0.0;
        const double h_n = ft ? ap[dto] : hfix;
        const double al = av * cl;
        v4d Y[2][2];
        generator(P.img, m, al, base, lane, Y);
        const int sq = squarings(Y, h);
        v4d R[2][2];
        exp_plain(scr, Y, h * ldexp(1.0, -sq), sq, IdB, g, j, R);
        transpose4(scr, R, Y, g, j);
        xapply(Y, x);
        av = av_n;
        h = h_n;
    }
}

// x_J^T, J = 0, 1, in the B-operand layout, straight from the stored state: tile J, lane (g, j), reg r = x[16 J + j][4 r + g] at
// xp[16 J + 4 n r], xp the lane's own pointer to x[j][g]; bit 4 J + r of `ok` says whether the entry exists (16 J + j < n and 4 r + g < cols),
// everything else of the tiles is zero
__device__ __forceinline__ void load_xT(const double* __restrict__ xp, int n4, int ok, v4d (&xT)[2]) {
#pragma unroll
    for (int J = 0; J < 2; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) xT[J][r] = ((ok >> (4 * J + r)) & 1) ? xp[16 * J + n4 * r] : 0.0;
}

template <bool PAR>
constexpr int kOW = PAR ? 2 : kWaves;                      // waves a workgroup, as the closed wide walk
template <bool PAR>
constexpr int kOSl = PAR ? kScr + 16 * 64 : kScr;          // doubles of LDS a wave: the transposition tiles, PAR: and Acc behind them

// One wavefront per (sample, chunk), walking the chunk backwards on the stored states.  The flavours, `part` and `gs` as
// qc_sweep32_grad_kernel (qc_sweep32_grad.hip).
template <bool PAR>
__global__ __launch_bounds__(64 * kOW<PAR>) void qc_sweep32_open_grad_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                            const double* __restrict__ theta, const double* __restrict__ scale,
                                                                            const double* __restrict__ xall, const double* __restrict__ ls,
                                                                            double* __restrict__ gs, double* __restrict__ part) {
    __shared__ double scr_all[kOW<PAR> * kOSl<PAR>];
    const WaveItem w = wave_item(kOW<PAR>);
    double* __restrict__ scr = scr_all + w.wq * kOSl<PAR>;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    const int ns = P.n * P.nc;

    // ---- once per wave: the sample's base matrix, the adjoint at the chunk's end, the lane's view of the stored states ----------------
    v4d base[2][2];
    base_matrix(P.img, m, P.p, theta, s, lane, base);
    const int kl = lane < m ? lane : (m > 0 ? m - 1 : 0);      // restates drive_lane: the shared form moves the flavour <true>, which no bench times
    const double cl = (scale && m > 0) ? scale[s * m + kl] : 1.0;

    v4d lam[2];
    {
        const double* __restrict__ le = ls + item * ns;
#pragma unroll
        for (int I = 0; I < 2; ++I)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * I + 4 * r + g;
                lam[I][r] = (row < P.n && j < P.nc) ? le[row + P.n * j] : 0.0;
            }
    }
    // knot t of sample s is at xall + (s (T-1) + t) ns; a set bit of okx implies j < n and g < cols, so the lane's pointer stays inside the knot
    int okx = 0;
#pragma unroll
    for (int J = 0; J < 2; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) okx |= (16 * J + j < P.n && 4 * r + g < P.nc) ? (1 << (4 * J + r)) : 0;
    const double* xp = xall + (s * P.n_int + (t1 - 1)) * ns + (okx ? j + P.n * g : 0);
    const int n4 = 4 * P.n;
    v4d xT[2];
    load_xT(xp, n4, okx, xT);

    const double hfix = opaque_scalar(P.dt_fixed);
    // the lane's control of the interval (lane l: drive min(l, m-1)) and, `dto` entries further, the timestep: one pointer walking down
    const double* ap = Z + (long long)(t1 - 1) * P.zdim + P.off_a + kl;
    const int dto = P.off_dt - P.off_a - kl;
    double av = m > 0 ? ap[0] : 0.0;
    double h = ft ? ap[dto] : hfix;
    // the lane's slot of the interval's one store (lane k: drive k, lane m: timestep), a pointer of its own walking down with t
    double* gp = gs + (s * P.n_int + (t1 - 1)) * P.nd + lane;
    const int stl = (gs && lane < P.nd) ? 1 : 0;
    const bool want_h = ft && (!PAR || gs);      // the timestep derivative leaves through gs only
    // PAR: Acc = sum_t ZT_t in the wave's LDS slice (tile q of lane l, register r at accl[64 (4 q + r) + l]: every lane reads back what it
    // wrote itself, no barrier); lane k's sum_t a_{t,k} du_{t,k} in a register
    double* accl = scr + kScr;
    double accv = 0.0;
    // what the chunk's end needs waits in vector registers (the share's address per lane, p), as in the closed wide walk: the loop has no
    // scalar register to spare
    double* po = nullptr;
    int pv = 0;
    if constexpr (PAR) {
#pragma unroll
        for (int i = 0; i < 16; ++i) accl[64 * i + lane] = 0.0;
        po = part + item * (P.p + m) + lane;
        pv = P.p;
        asm volatile("" : "+v"(po), "+v"(pv));
    }
#pragma unroll 1
    for (int t = t1 - 1; t >= t0; --t) {
        // the interval below is requested before this interval's products
        if (t > t0) ap -= P.zdim;
        const double av_n = m > 0 ? ap[0] : 0.0;
        const double h_n = ft ? ap[dto] : hfix;
        const double al = av * cl;
        v4d Y[2][2], dY[2][2];
        // the image buffer's address is taken anew where it is used, so that no derived address is kept across the interval
        const double* __restrict__ img = P.img;
        asm volatile("" : "+s"(img));
        generator(img, m, al, base, lane, Y);
        const int sq = squarings(Y, h);      // the rule of the forward and the store kernel: one function
        const double sc = ldexp(1.0, -sq);
        const double hs = h * sc;
        // KT = lambda_{t+1} x_t^T (D layout); dY in A layout is KT with the block index swapped: it acts as K^T = x_t lambda^T
        {
            v4d lamA[2];
            lds_transpose16_multi<2>(scr, lam, lamA, g, j);
            v4d k00 = zero, k01 = zero, k10 = zero, k11 = zero;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                k00 = __builtin_amdgcn_mfma_f64_16x16x4f64(lamA[0][kk], xT[0][kk], k00, 0, 0, 0);
                k01 = __builtin_amdgcn_mfma_f64_16x16x4f64(lamA[0][kk], xT[1][kk], k01, 0, 0, 0);
                k10 = __builtin_amdgcn_mfma_f64_16x16x4f64(lamA[1][kk], xT[0][kk], k10, 0, 0, 0);
                k11 = __builtin_amdgcn_mfma_f64_16x16x4f64(lamA[1][kk], xT[1][kk], k11, 0, 0, 0);
            }
            dY[0][0] = sc * k00; dY[1][0] = sc * k01; dY[0][1] = sc * k10; dY[1][1] = sc * k11;      // dY(I, K) = KT[K][I] / 2^sq
        }
        // the state of the interval below is requested before this interval's chain
        {
            int ok = okx;      // the eight masks of the state's padding are made per interval, not kept in scalar registers
            asm volatile("" : "+v"(ok));
            if (t > t0) xp -= ns;
            load_xT(xp, n4, ok, xT);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) Y[q >> 1][q & 1] = hs * Y[q >> 1][q & 1];
        v4d R[2][2] = {{kInvFact[kDeg] * IdB, zero}, {zero, kInvFact[kDeg] * IdB}};
        v4d dR[2][2] = {{zero, zero}, {zero, zero}};
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) vstep(Y, dY, R, dR, kInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            transpose4(scr, R, Y, g, j);           // E, dE in A layout; Y, dY are free from here on
            transpose4(scr, dR, dY, g, j);
            vstep(Y, dY, R, dR, zero);
        }
        // dR = L(hG; K^T) = L(hG^T; K)^T in D layout: tile [I][J] against an A-layout tile (J, I) is the inner product with its transpose.
        // ZT = h dR into dY; the pass over the drive images also rebuilds G (base + sum al_u G_u, the order of `generator`) into Y.
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            dY[q >> 1][q & 1] = h * dR[q >> 1][q & 1];
            Y[q >> 1][q & 1] = base[q >> 1][q & 1];
        }
        int ln = lane;      // as in the closed walk: the lane compares are made per interval, not kept in scalar registers
        asm volatile("" : "+v"(ln));
        double out = 0.0, duv = 0.0;      // duv (PAR): lane k holds du_k = sum ZT . G_k; lanes >= m keep 0
        const double* __restrict__ imgc = P.img;
        asm volatile("" : "+s"(imgc));
#pragma unroll 1
        for (int u = 0; u < m; ++u) {
            const double a = bcast_lane(al, u);
            const double* __restrict__ Gu = imgc + (size_t)(1 + u) * 1024;
            double pu = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v4d t4 = load_image_tile(Gu + q * 256, lane);       // tile (J, I) = q against ZT[I][J]
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pu = fma(dY[q & 1][q >> 1][r], t4[r], pu);
                    Y[q >> 1][q & 1][r] = fma(a, t4[r], Y[q >> 1][q & 1][r]);
                }
            }
            const double du = wave_sum(pu);
            if constexpr (PAR) duv = ln == u ? du : duv;
            else out = ln == u ? du * cl : out;
        }
        if constexpr (PAR) out = ln < m ? duv * cl : out;
        if (want_h) {
            double ph = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) ph = fma(dR[q & 1][q >> 1][r], Y[q >> 1][q & 1][r], ph);
            const double dh = wave_sum(ph);
            out = ln == m ? dh : out;
        }
        if constexpr (PAR) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) accl[64 * (4 * q + r) + lane] += dY[q >> 1][q & 1][r];
            accv = fma(av, duv, accv);
        }
        {
            int st = stl;
            asm volatile("" : "+v"(st));
            if (st) *gp = out;
            gp -= P.nd;
        }
        vapplyT(R, lam);
        av = av_n;
        h = h_n;
    }
    if constexpr (PAR) {
        // the chunk's shares: one contraction of Acc per perturbation, the image tiles read once here; tile (J, I) = u against Acc[I][J]
        const int p = __builtin_amdgcn_readfirstlane(pv);
        int le = lane;
        asm volatile("" : "+v"(le));      // the lane compares are made here, not kept across the loop
        double acc_t = 0.0;
#pragma unroll 1
        for (int q = 0; q < p; ++q) {
            const double* __restrict__ Pq = P.img + (size_t)(1 + m + q) * 1024;
            double pq = 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const v4d t4 = load_image_tile(Pq + u * 256, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) pq = fma(accl[64 * (4 * (2 * (u & 1) + (u >> 1)) + r) + lane], t4[r], pq);
            }
            const double dq = wave_sum(pq);
            acc_t = le == q ? dq : acc_t;
        }
        if (le < p) po[0] = acc_t;
        if (le < m) po[p] = accv;
    }
}

}  // namespace

void qc_sweep32_open_launch_walk(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                                 int64_t chunk, int64_t n_chunks, double* gs, bool par, double* dgrad_theta, double* dgrad_scale, hipStream_t st) {
    const SweepParams P = qc_sweep_params(h, S, chunk, n_chunks);
    hipLaunchKernelGGL(qc_sweep32_open_store_kernel, dim3(qc_sweep_grid(P, kWaves)), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale,
                       dinit, (const double*)h->dXs.p, h->dXall.p);
    if (par) {
        hipLaunchKernelGGL(qc_sweep32_open_grad_kernel<true>, dim3(qc_sweep_grid(P, kOW<true>)), dim3(64 * kOW<true>), 0, st, P, dZ,
                           dtheta, dscale, (const double*)h->dXall.p, (const double*)h->dLs.p, gs, h->dPart.p);
        qc_sweep_launch_par_reduce(h, S, n_chunks, dgrad_theta, dgrad_scale, st);
    } else
        hipLaunchKernelGGL(qc_sweep32_open_grad_kernel<false>, dim3(qc_sweep_grid(P, kOW<false>)), dim3(64 * kOW<false>), 0, st, P, dZ,
                           dtheta, dscale, (const double*)h->dXall.p, (const double*)h->dLs.p, gs, (double*)nullptr);
}
