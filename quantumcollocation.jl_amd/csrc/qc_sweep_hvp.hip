// Sweep Hessian products: the tangent of the sweep pullback (qc_sweep_vjp.hip) along ONE direction (vZ, vinit, vtheta, vc, vcot) --
// forward over reverse.  For sample s, with phi_s = <C_s, x_final[s]>, g_s = dphi_s/d(a_t, h_t) (the pullback's grad_samples[s]) and
// q_s = dphi_s/dinit = W^T C_s (its grad_init[s]):
//     tgrad_samples[s] = d/de g_s(Z + e vZ, init + e vinit, theta + e vtheta, c + e vc; C + e vcot) at e = 0
//     tgrad_init[s]    = d/de q_s = Wdot^T C_s + W^T vcot_s
//     tgrad            = sum_s tgrad_samples[s], the plain sum in ascending s, in the layout of Z.
// With cot = dl/dX and vcot = d2l/dX2 Xdot (Xdot from qc_sweep_jvp) tgrad is the exact Hessian product of l(X(Z)); with vcot = 0 it is the
// curvature of the sweep map itself, sum_s <C_s, d2x_s/dZ2 v>, the term a Gauss-Newton product drops.
//
// With A_t = h_t G_s(a_t), Adot_t = vh_t G_s(a_t) + h_t Gdot_t, Gdot_t = sum_j vtheta[s,j] P_j + sum_k (vc[s,k] a_{t,k} + c[s,k] va_{t,k}) G_k
// (antisymmetric as G is), E_t = exp(A_t), Edot_t = L(A_t; Adot_t):
//     xdot_0 = vinit,                 xdot_{t+1} = E_t xdot_t + Edot_t x_t
//     lambdadot_{T-1} = vcot_s,       lambdadot_t = E_t^T lambdadot_{t+1} + Edot_t^T lambda_{t+1}
// and the derivative of every product of the gradient walk (qc_sweep_grad.hip; read its header and qc_sweep_jvp.hip's first).  The
// antisymmetry identities of that walk, x_t = E^T x_{t+1} and L(hG; E^T K) = E^T L(hG; K), hold for every e along the direction, so
// they may be differentiated as they stand.
//
// Scope: the pullback's closed scope -- antisymmetric drift, drives and perturbations, at most 16 state columns, any fid_kind -- in the
// "mfma16-sweep" form (2N <= 16, m <= 8: this file), and in the "mfma32-sweep" form of a descriptor whose wide has QC_SWEEP_WIDE_HESSIAN
// (qc_sweep32_hvp.hip: the walk on 2 x 2 tiles; this file's launch function routes to it and its seed kernel is this file's at ld = 32).
// Everything else: QC_ERR_UNSUPPORTED, "qc_sweep Hessian product: " + the reason.
//
// Launches of one call:
//   1. qc_sweep_jvp_kernel<M> (qc_sweep_jvp.hip, unchanged, through qc_sweep_jvp_launch_totals): the chunk totals W_c and their tangents
//      Wdot_c along (vZ, vtheta, vc) in h->dTotJ.
//   2. qc_sweep_hvp_seed_kernel, one workgroup per sample.  Up: (x, xdot) through the chunks with the loops of
//      qc_sweep_jvp_finish_kernel, stored at every chunk end (dXs, dXsT).  Down: lambda = cot, lambdadot = vcot;
//      lambdadot <- Q_c^T lambdadot + Qdot_c^T lambda, lambda <- Q_c^T lambda, stored at every chunk end (dLs, dLsT); with tgrad_init one
//      more step down to c = 0.  The totals lie 512 doubles apart (W, Wdot), not the 256 the chains of qc_sweep_seed.h step by, and
//      every step carries a pair: the loops are written out here.  ns <= 256: 4 ns + 512 doubles of LDS, at most 12 KiB.
//   3. qc_sweep_hvp_kernel<M>, M in {1, 2, 4, 6, 8}: work item, workgroup shape and chunk rule of the gradient walk (one wavefront per
//      (sample, chunk), four per workgroup, never synchronised, the chunk walked BACKWARDS).  Per interval, with x, xdot, lambda,
//      lambdadot the D-layout tiles of knot t+1:
//        KT = lambda x^T,  KTdot = lambdadot x^T + lambda xdot^T                         one LDS round trip (4 tiles), 12 MFMAs
//        Ga, Gadot; sq from ||h Ga||_1 by the forward kernel's rule (no tangent enters it)
//        gdot_h = -sum (KTdot . Ga + KT . Gadot)
//        Y = (h / 2^sq) Ga,  Ydot = (vh / 2^sq) Ga + (h / 2^sq) Gadot,  dY = (h / 2^sq) K,  dYdot = (vh / 2^sq) K + (h / 2^sq) Kdot
//        Horner, k = 10 .. 1, on the quadruple, nine products (36 MFMAs) a step:
//            R <- Y R + I/(k-1)!,  Rdot <- Ydot R + Y Rdot,  dR <- dY R + Y dR,  dRdot <- dYdot R + dY Rdot + Ydot dR + Y dRdot
//        per squaring the same nine products with the four transposed tiles (one LDS round trip) as left factors     36 MFMAs
//        ZT = E^T dE,  ZTdot = Edot^T dE + E^T dEdot                                                                   12 MFMAs
//        gdot_k = vc_k sum ZT . G_k + c_k sum ZTdot . G_k
//        xdot <- Edot^T x + E^T xdot, x <- E^T x, and lambda, lambdadot alike                                          24 MFMAs
//      and one vector store per interval (lane k: drive k, lane m: the timestep).
//      MFMAs per interval: 12 + 10 x 36 + 36 sq + 12 + 24 = 408 + 36 sq, against the gradient walk's 112 + 12 sq.
//   4. qc_sweep_vjp_reduce_kernel (qc_sweep_vjp.hip, unchanged, through qc_sweep_launch_plain_sum) on the tangent per-interval buffer.
// No atomics, sums in a fixed order: repeated calls return the same bits, and no output's bits depend on which others were asked for.
// A NULL direction is read as zeros through the same arithmetic: NULL and an explicit zero array give the same bits.
//
// Series degree: 10 at the forward kernel's threshold ||Y||_1 <= 1/8.  The twice-differentiated degree-d series misses
// sum_{k>d} k (k-1) ||Y||^(k-2) / k! ||dY|| ||Ydot|| <= 1.15 (1/8)^(d-1) / (d-1)! ||dY|| ||Ydot||: 9.5e-11 at d = 8 (too coarse for the
// 1e-9 of the tests once the squarings have doubled it a few times), 2e-14 at d = 10 (the bound of qc_mfma_exp_hess.hip).  The values
// (x, lambda, E) are therefore those of a degree-10 series, not the bits of the degree-8 kernels; they agree to 1e-17 relative.
//
// Registers: 18 + M tiles of 8 VGPRs are live in the Horner loop (base, its tangent, M drive tiles, the four states, Y / Ydot / dY / dYdot,
// the quadruple and its four accumulators).  The kernel is built for one wave per SIMD (__launch_bounds__(256, 1)): the 512-register
// budget holds every instantiation without a private segment.  gfx950 cross-compile: see the table in DESIGN.md ("Sweep Hessian products").
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_sweep16_common.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep16;         // threshold and squaring rule, tile load, generator, product and wave sum of the 16 x 16 form

constexpr int kHDeg = 10;           // see "Series degree" above: this file's own degree and table
constexpr int kHSeedT = 256;
constexpr int kHSlice = 4 * kTile;  // LDS of one wave: four transposition tiles

// 1 / k!, k = 0 .. 10
__constant__ const double kHInvFact[kHDeg + 1] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0,
                                                  1.0 / 40320.0, 1.0 / 362880.0, 1.0 / 3628800.0};

struct HvpSeedParams {
    int n, ns, n_chunks;
};

// The nine products of a step on the quadruple (R, Rdot, dR, dRdot) with the left factors (A, Adot, dA, dAdot):
//     R <- A R + C,  Rdot <- Adot R + A Rdot,  dR <- dA R + A dR,  dRdot <- dAdot R + dA Rdot + Adot dR + A dRdot
// a Horner step (A = Y ..., C = I / (k-1)!) or a squaring (A = E ..., C = 0).  Four accumulator chains, interleaved.
__device__ __forceinline__ void hstep(const v4d& A, const v4d& Ad, const v4d& dA, const v4d& dAd, v4d& R, v4d& Rd, v4d& dR, v4d& dRd, const v4d& C) {
    const v4d z = {0.0, 0.0, 0.0, 0.0};
    v4d r = C, rd = z, dr = z, q = z;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        q = __builtin_amdgcn_mfma_f64_16x16x4f64(dAd[kk], R[kk], q, 0, 0, 0);
        rd = __builtin_amdgcn_mfma_f64_16x16x4f64(Ad[kk], R[kk], rd, 0, 0, 0);
        dr = __builtin_amdgcn_mfma_f64_16x16x4f64(dA[kk], R[kk], dr, 0, 0, 0);
        r = __builtin_amdgcn_mfma_f64_16x16x4f64(A[kk], R[kk], r, 0, 0, 0);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        q = __builtin_amdgcn_mfma_f64_16x16x4f64(dA[kk], Rd[kk], q, 0, 0, 0);
        rd = __builtin_amdgcn_mfma_f64_16x16x4f64(A[kk], Rd[kk], rd, 0, 0, 0);
        dr = __builtin_amdgcn_mfma_f64_16x16x4f64(A[kk], dR[kk], dr, 0, 0, 0);
        q = __builtin_amdgcn_mfma_f64_16x16x4f64(Ad[kk], dR[kk], q, 0, 0, 0);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) q = __builtin_amdgcn_mfma_f64_16x16x4f64(A[kk], dRd[kk], q, 0, 0, 0);
    R = r;
    Rd = rd;
    dR = dr;
    dRd = q;
}

// One wavefront per (sample, chunk), walking the chunk backwards: the gradient walk with every product differentiated beside itself.
// xs / ls: x and lambda at the chunk ends, xts / lts: their tangents; tgs: S x (T-1) x nd.
template <int M>
__global__ __launch_bounds__(64 * kWaves, 1) void qc_sweep_hvp_kernel(const SweepParams P, const double* __restrict__ Z, const double* __restrict__ theta,
                                                                        const double* __restrict__ scale, const double* __restrict__ vZ,
                                                                        const double* __restrict__ vtheta, const double* __restrict__ vscale,
                                                                        const double* __restrict__ xs, const double* __restrict__ ls,
                                                                        const double* __restrict__ xts, const double* __restrict__ lts,
                                                                        double* __restrict__ tgs) {
    __shared__ double scr_all[kWaves * kHSlice];
    const WaveItem w = wave_item(kWaves);
    double* __restrict__ scr = scr_all + w.wq * kHSlice;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m;
    const bool ft = P.off_dt >= 0;
    const bool hasv = vZ != nullptr;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    // ---- once per wave: the sample's base tile and its tangent, the drive tiles, the four states at the chunk's end -----------------
    v4d base, based;
    base_tile(P.img, m, P.p, theta, vtheta, s, lane, base, based);
    v4d Gj[M];
    resident_tiles(P.img, m, lane, Gj);
    // lane l holds the sample's factor of drive min(l, m-1) and its tangent
    const int kl = lane < m ? lane : (m > 0 ? m - 1 : 0);
    const double cl = (scale && m > 0) ? scale[s * m + kl] : 1.0;
    const double vcl = (vscale && m > 0) ? vscale[s * m + kl] : 0.0;

    v4d x, xd, lam, lamd;
    {
        const int ns = P.n * P.nc;
        const double* __restrict__ xe = xs + item * ns;
        const double* __restrict__ le = ls + item * ns;
        const double* __restrict__ xte = xts + item * ns;
        const double* __restrict__ lte = lts + item * ns;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * r + g;
            const bool in = row < P.n && j < P.nc;
            x[r] = in ? xe[row + P.n * j] : 0.0;
            lam[r] = in ? le[row + P.n * j] : 0.0;
            xd[r] = in ? xte[row + P.n * j] : 0.0;
            lamd[r] = in ? lte[row + P.n * j] : 0.0;
        }
    }

    const double hfix = opaque_scalar(P.dt_fixed);
    const double* __restrict__ z = Z + (long long)(t1 - 1) * P.zdim;
    double av = m > 0 ? z[P.off_a + kl] : 0.0;
    double h = ft ? z[P.off_dt] : hfix;
    double vav = 0.0, vh = 0.0;
    if (hasv) {
        const double* __restrict__ vz = vZ + (long long)(t1 - 1) * P.zdim;
        if (m > 0) vav = vz[P.off_a + kl];
        if (ft) vh = vz[P.off_dt];
    }
#pragma unroll 1
    for (int t = t1 - 1; t >= t0; --t) {
        // the previous interval's controls, timestep and their tangents are requested before this interval's products
        const long long tn = t > t0 ? t - 1 : t;
        const double* __restrict__ zn = Z + tn * P.zdim;
        const double av_n = m > 0 ? zn[P.off_a + kl] : 0.0;
        const double h_n = ft ? zn[P.off_dt] : hfix;
        double vav_n = 0.0, vh_n = 0.0;
        const double* vZt = vZ;      // (opaque: the test is made per interval, not kept in two scalar registers)
        asm volatile("" : "+s"(vZt));
        if (vZt) {
            const double* __restrict__ vzn = vZt + tn * P.zdim;
            if (m > 0) vav_n = vzn[P.off_a + kl];
            if (ft) vh_n = vzn[P.off_dt];
        }
        const double al = av * cl;
        const double ald = fma(vav, cl, av * vcl);
        // kept loop-invariant, the M compares u < m live in two scalar registers each (M = 8 spills them): an opaque copy of m has them
        // made per interval instead
        int mu = m;
        asm volatile("" : "+s"(mu));
        v4d Ga, Gad;
        generator(base, based, Gj, mu, al, ald, Ga, Gad);
        const int sq = squarings(h, Ga);      // the rule of the forward kernel, from ||h Ga||_1 alone
        const double sc = ldexp(1.0, -sq);
        const double hs = h * sc, vhs = vh * sc;
        // K^T = lambda x^T of knot t+1 (D layout) and its tangent, from the A-layout forms of the four states
        v4d KT, KTd;
        {
            const v4d in[4] = {x, lam, xd, lamd};
            v4d tr[4];
            lds_transpose16_multi<4>(scr, in, tr, g, j);
            KT = mma16(tr[1], tr[0], zero);
            KTd = mma16(tr[3], tr[0], zero);
            KTd = mma16(tr[1], tr[2], KTd);
        }
        // kept loop-invariant, the lane compares below live in two scalar registers each and the larger instantiations spill them; an opaque
        // copy of the lane index has them made per interval instead (as qc_sweep_grad_kernel<8>)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        double out = 0.0;
        if (ft) {
            double ph = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) ph = fma(KTd[r], Ga[r], ph);
#pragma unroll
            for (int r = 0; r < 4; ++r) ph = fma(KT[r], Gad[r], ph);
            const double dhd = -wave_sum(ph);
            out = ln == mu ? dhd : out;
        }
        const v4d Y = hs * Ga;
        const v4d dY = hs * KT;
        v4d Yd, dYd;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Yd[r] = fma(vhs, Ga[r], hs * Gad[r]);
            dYd[r] = fma(vhs, KT[r], hs * KTd[r]);
        }
        v4d R = kHInvFact[kHDeg] * IdB, Rd = zero, dR = zero, dRd = zero;
#pragma unroll 1
        for (int k = kHDeg; k >= 1; --k) hstep(Y, Yd, dY, dYd, R, Rd, dR, dRd, kHInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            const v4d in[4] = {R, Rd, dR, dRd};
            v4d tr[4];
            lds_transpose16_multi<4>(scr, in, tr, g, j);      // the transposes in D layout = E, Edot, dE, dEdot in A layout
            hstep(tr[0], tr[1], tr[2], tr[3], R, Rd, dR, dRd, zero);
        }
        const v4d ZT = mma16(R, dR, zero);                       // E^T dE
        v4d ZTd = mma16(Rd, dR, zero);                           // Edot^T dE + E^T dEdot
        ZTd = mma16(R, dRd, ZTd);
#pragma unroll
        for (int u = 0; u < M; ++u) {
            if (u < mu) {
                double pu = 0.0, pud = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pu = fma(ZT[r], Gj[u][r], pu);
                    pud = fma(ZTd[r], Gj[u][r], pud);
                }
                const double du = wave_sum(pu);
                const double dud = wave_sum(pud);
                out = ln == u ? fma(dud, cl, du * vcl) : out;
            }
        }
        if (ln < P.nd) tgs[(s * P.n_int + t) * P.nd + ln] = out;
        {
            v4d nxd = mma16(Rd, x, zero);
            nxd = mma16(R, xd, nxd);
            v4d nld = mma16(Rd, lam, zero);
            nld = mma16(R, lamd, nld);
            x = mma16(R, x, zero);
            lam = mma16(R, lam, zero);
            xd = nxd;
            lamd = nld;
        }
        av = av_n;
        h = h_n;
        vav = vav_n;
        vh = vh_n;
    }
}

// One workgroup per sample.  tot: the sample's n_chunks pairs (W_c, Wdot_c) of ld x ld column-major matrices, l2 = ld^2 doubles each:
// ld = 16 for "mfma16-sweep" handles, 32 for "mfma32-sweep" ones (the two kernels below, as qc_sweep_jvp_finish_kernel).  Up, ascending chunks:
// xdot <- Q_c xdot + Qdot_c x, x <- Q_c x (the loops of qc_sweep_jvp_finish_kernel), both stored at every chunk end.  Down:
// lambda = cot, lambdadot = vcot (NULL: zeros) at the last chunk end; lambdadot <- Q_c^T lambdadot + Qdot_c^T lambda,
// lambda <- Q_c^T lambda for c = n_chunks-1 .. 1, stored at the end of chunk c-1; with tginit the step c = 0 as well, whose lambdadot is
// the sample's tgrad_init.
template <int ld, int l2>
__device__ __forceinline__ void hvp_seed(const HvpSeedParams& F, const double* __restrict__ tot, const double* __restrict__ src,
                                         const double* __restrict__ vsrc, const double* __restrict__ cot, const double* __restrict__ vcot,
                                         double* __restrict__ xs, double* __restrict__ xts, double* __restrict__ ls, double* __restrict__ lts,
                                         double* __restrict__ tginit) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int tid = threadIdx.x, n = F.n, ns = F.ns;
    const long long s = blockIdx.x;
    double* cur = sm;
    double* nxt = sm + ns;
    double* dcur = sm + 2 * ns;
    double* dnxt = sm + 3 * ns;
    double* Q = sm + 4 * ns;
    double* Qd = Q + l2;
    const double* __restrict__ Qs = tot + s * F.n_chunks * (long long)(2 * l2);
    const long long so = s * F.n_chunks * (long long)ns;
    for (int idx = tid; idx < ns; idx += kHSeedT) {
        cur[idx] = src[idx];
        dcur[idx] = vsrc ? vsrc[idx] : 0.0;
    }
    for (int c = 0; c < F.n_chunks; ++c) {
        __syncthreads();
        for (int idx = tid; idx < 2 * l2; idx += kHSeedT) Q[idx] = Qs[(long long)c * (2 * l2) + idx];
        __syncthreads();
        for (int idx = tid; idx < ns; idx += kHSeedT) {
            const int r = idx % n, col = idx / n;
            double acc = 0.0, dacc = 0.0;
            for (int q = 0; q < n; ++q) acc = fma(Q[r + ld * q], cur[q + n * col], acc);
            for (int q = 0; q < n; ++q) dacc = fma(Q[r + ld * q], dcur[q + n * col], dacc);
            for (int q = 0; q < n; ++q) dacc = fma(Qd[r + ld * q], cur[q + n * col], dacc);
            nxt[idx] = acc;
            dnxt[idx] = dacc;
            xs[so + (long long)c * ns + idx] = acc;
            xts[so + (long long)c * ns + idx] = dacc;
        }
        double* tmp = cur; cur = nxt; nxt = tmp;
        tmp = dcur; dcur = dnxt; dnxt = tmp;
    }
    __syncthreads();
    // lambda and its tangent at the final knot: the caller's cotangent and its direction, as read
    for (int idx = tid; idx < ns; idx += kHSeedT) {
        const double v = cot[s * ns + idx];
        const double vd = vcot ? vcot[s * ns + idx] : 0.0;
        cur[idx] = v;
        dcur[idx] = vd;
        ls[so + (long long)(F.n_chunks - 1) * ns + idx] = v;
        lts[so + (long long)(F.n_chunks - 1) * ns + idx] = vd;
    }
    for (int c = F.n_chunks - 1; c >= (tginit ? 0 : 1); --c) {
        __syncthreads();
        for (int idx = tid; idx < 2 * l2; idx += kHSeedT) Q[idx] = Qs[(long long)c * (2 * l2) + idx];
        __syncthreads();
        for (int idx = tid; idx < ns; idx += kHSeedT) {
            const int r = idx % n, col = idx / n;
            double acc = 0.0, dacc = 0.0;
            for (int q = 0; q < n; ++q) acc = fma(Q[q + ld * r], cur[q + n * col], acc);
            for (int q = 0; q < n; ++q) dacc = fma(Q[q + ld * r], dcur[q + n * col], dacc);
            for (int q = 0; q < n; ++q) dacc = fma(Qd[q + ld * r], cur[q + n * col], dacc);
            nxt[idx] = acc;
            dnxt[idx] = dacc;
            if (c > 0) {
                ls[so + (long long)(c - 1) * ns + idx] = acc;
                lts[so + (long long)(c - 1) * ns + idx] = dacc;
            } else {
                tginit[s * ns + idx] = dacc;
            }
        }
        double* tmp = cur; cur = nxt; nxt = tmp;
        tmp = dcur; dcur = dnxt; dnxt = tmp;
    }
}

__global__ __launch_bounds__(kHSeedT) void qc_sweep_hvp_seed_kernel(const HvpSeedParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                                                    const double* __restrict__ vsrc, const double* __restrict__ cot,
                                                                    const double* __restrict__ vcot, double* __restrict__ xs,
                                                                    double* __restrict__ xts, double* __restrict__ ls, double* __restrict__ lts,
                                                                    double* __restrict__ tginit) {
    constexpr int ld = 16, l2 = 256;
    hvp_seed<ld, l2>(F, tot, src, vsrc, cot, vcot, xs, xts, ls, lts, tginit);
}

// the same on the 32 x 32 totals of "mfma32-sweep" handles (qc_sweep32_jvp.hip): 2048 doubles a pair, 4 ns + 2048 doubles of LDS (ns <= 512: 32 KiB)
__global__ __launch_bounds__(kHSeedT) void qc_sweep32_hvp_seed_kernel(const HvpSeedParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                                                      const double* __restrict__ vsrc, const double* __restrict__ cot,
                                                                      const double* __restrict__ vcot, double* __restrict__ xs,
                                                                      double* __restrict__ xts, double* __restrict__ ls, double* __restrict__ lts,
                                                                      double* __restrict__ tginit) {
    constexpr int ld = 32, l2 = 1024;
    hvp_seed<ld, l2>(F, tot, src, vsrc, cot, vcot, xs, xts, ls, lts, tginit);
}

const char* const kHvpScope = "qc_sweep Hessian product: ";

// the argument checks both entry points share, in the order of the header's table
int hvp_check(qc_sweep* h, const char* who, const void* Z, const void* init, int64_t S, const void* theta, const void* cot, bool any_dir, bool any_out,
              bool v_theta, bool v_scale) {
    int rc = qc_sweep_check(h, who, &qc_sweep::hvp_ok, kHvpScope, &qc_sweep::hvp_why, Z, init, cot ? nullptr : "cot", S, theta);
    if (rc) return rc;
    const std::string pre = std::string(who) + ": ";
    if (!any_dir) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "every direction is NULL");
    if (!any_out) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "every output is NULL");
    if (v_theta && h->d.n_pert == 0) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "vtheta is given but the handle has no perturbations (n_pert = 0)");
    if (v_scale && h->d.m == 0) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "vscale is given but the handle has no drives (m = 0)");
    return QC_OK;
}

}  // namespace

// The pullback's closed scope (its reasons first: the per-sample form, antisymmetry, more than 16 columns) within the "mfma16-sweep" form,
// or within the "mfma32-sweep" form of a descriptor whose wide has QC_SWEEP_WIDE_HESSIAN (qc_sweep32_hvp.hip).
bool qc_sweep_hvp_scope(const qc_sweep_desc* d, std::string* why) {
    // the closed scope can pass in the "mfma64-sweep" form (QC_SWEEP_WIDE_64_GRAD): this scope refuses the form itself
    if (qc_sweep_desc_form(d) == QC_SWEEP_FORM_64) { *why = qc_sweep_form64_unserved(d, "Hessian products"); return false; }
    if (!qc_sweep_closed_scope(d, why)) return false;
    if (qc_sweep_desc_form(d) == QC_SWEEP_FORM_32 && !(d->wide & QC_SWEEP_WIDE_HESSIAN)) { *why = "Hessian products are not served in the mfma32-sweep form"; return false; }
    return true;
}

extern "C" int qc_sweep_desc_hvp_supported(const qc_sweep_desc* d, int32_t* supported) {
    int rc = qc_sweep_validate_desc(d);
    if (rc) return rc;
    if (!supported) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep_desc_hvp_supported: supported is NULL");
    std::string why;
    const bool ok = qc_sweep_hvp_scope(d, &why);
    *supported = ok ? 1 : 0;
    if (!ok) (void)qc_sweep_fail(nullptr, QC_ERR_UNSUPPORTED, kHvpScope + why);
    return QC_OK;
}

static int qc_sweep_hvp_launch(qc_sweep* h, const char* who, const double* dZ, const double* dinit, int64_t S, const double* dtheta,
                               const double* dscale, const double* dcot, const double* dvZ, const double* dvinit, const double* dvtheta,
                               const double* dvscale, const double* dvcot, double* dtgrad, double* dtgrad_samples, double* dtgrad_init, void* stream) {
    int rc = hvp_check(h, who, dZ, dinit, S, dtheta, dcot, dvZ || dvinit || dvtheta || dvscale || dvcot, dtgrad || dtgrad_samples || dtgrad_init,
                       dvtheta != nullptr, dvscale != nullptr);
    if (rc) return rc;
    std::string& slot = *qc_sweep_err_slot();
    qc_device_guard guard(h->device);
    QC_SIDE_HIP(h, slot, guard.err);
    hipStream_t st = (hipStream_t)stream;
    const int m = h->d.m;
    const int nd = m + (h->d.off_dt >= 0 ? 1 : 0);
    const int64_t n_int = h->d.T - 1;
    int64_t chunk, n_chunks;
    if ((rc = qc_sweep_jvp_launch_totals(h, dZ, S, dtheta, dscale, dvZ, dvtheta, dvscale, st, &chunk, &n_chunks))) return rc;
    const size_t n_state = (size_t)S * n_chunks * h->ns;
    QC_SIDE_HIP(h, slot, h->grow(h->dXs, n_state));
    QC_SIDE_HIP(h, slot, h->grow(h->dLs, n_state));
    QC_SIDE_HIP(h, slot, h->grow(h->dXsT, n_state));
    QC_SIDE_HIP(h, slot, h->grow(h->dLsT, n_state));
    const bool want_walk = (dtgrad || dtgrad_samples) && nd > 0;
    double* tgs = dtgrad_samples;
    if (want_walk && !tgs) {
        QC_SIDE_HIP(h, slot, h->grow(h->dTGsamp, (size_t)S * n_int * nd));
        tgs = h->dTGsamp.p;
    }
    HvpSeedParams F;
    F.n = h->n; F.ns = h->ns; F.n_chunks = (int)n_chunks;
    if (h->mfma32) {      // "mfma32-sweep" handles with wide_hessian: the seed at ld = 32, the walk of qc_sweep32_hvp.hip
        const size_t lds32 = ((size_t)4 * h->ns + 2048) * 8;      // at most 16 state columns of 32 rows: 32 KiB
        hipLaunchKernelGGL(qc_sweep32_hvp_seed_kernel, dim3((unsigned)S), dim3(kHSeedT), lds32, st, F, (const double*)h->dTotJ.p, dinit, dvinit, dcot,
                           dvcot, h->dXs.p, h->dXsT.p, h->dLs.p, h->dLsT.p, dtgrad_init);
        if (want_walk) qc_sweep32_hvp_launch_walk(h, dZ, S, dtheta, dscale, dvZ, dvtheta, dvscale, chunk, n_chunks, tgs, st);
    } else {
        const size_t lds = ((size_t)4 * h->ns + 512) * 8;      // at most 16 state columns: 12 KiB
        hipLaunchKernelGGL(qc_sweep_hvp_seed_kernel, dim3((unsigned)S), dim3(kHSeedT), lds, st, F, (const double*)h->dTotJ.p, dinit, dvinit, dcot, dvcot,
                           h->dXs.p, h->dXsT.p, h->dLs.p, h->dLsT.p, dtgrad_init);
        if (want_walk) {
            const SweepParams P = qc_sweep_params(h, S, chunk, n_chunks);
            const unsigned grid = qc_sweep_grid(P, kWaves);
#define QC_HVP_LAUNCH(M_)                                                                                                                 \
    hipLaunchKernelGGL(qc_sweep_hvp_kernel<M_>, dim3(grid), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale, dvZ, dvtheta, dvscale,       \
                       (const double*)h->dXs.p, (const double*)h->dLs.p, (const double*)h->dXsT.p, (const double*)h->dLsT.p, tgs)
            QC_SWEEP_FOR_M(m, QC_HVP_LAUNCH);
#undef QC_HVP_LAUNCH
        }
    }
    if (dtgrad) qc_sweep_launch_plain_sum(h, S, tgs, dtgrad, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qc_sweep_fail(h, QC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return QC_OK;
}

extern "C" int qc_sweep_hvp_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                                const double* dcot, const double* dvZ, const double* dvinit, const double* dvtheta, const double* dvscale,
                                const double* dvcot, double* dtgrad, double* dtgrad_samples, double* dtgrad_init, void* stream) {
    return qc_sweep_hvp_launch(h, "qc_sweep_hvp_dev", dZ, dinit, S, dtheta, dscale, dcot, dvZ, dvinit, dvtheta, dvscale, dvcot, dtgrad, dtgrad_samples,
                               dtgrad_init, stream);
}

// The host-buffer entry point: stage, launch on the handle's stream, copy back, synchronise.
extern "C" int qc_sweep_hvp(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale, const double* cot,
                            const double* vZ, const double* vinit, const double* vtheta, const double* vscale, const double* vcot, double* tgrad,
                            double* tgrad_samples, double* tgrad_init) {
    const char* who = "qc_sweep_hvp";
    int rc = hvp_check(h, who, Z, init, S, theta, cot, vZ || vinit || vtheta || vscale || vcot, tgrad || tgrad_samples || tgrad_init, vtheta != nullptr,
                       vscale != nullptr);
    if (rc) return rc;
    const size_t nS = (size_t)S, m = (size_t)h->d.m, p = (size_t)h->d.n_pert, ns = (size_t)h->ns, Zlen = (size_t)h->Zlen;
    const size_t n_samp = nS * (size_t)(h->d.T - 1) * (m + (h->d.off_dt >= 0 ? 1 : 0));
    qc_stage stage(h, qc_sweep_err_slot());
    const double* dZ = stage.in(h->sZ, Z, Zlen);
    const double* dinit = stage.in(h->sInit, init, ns);
    const double* dtheta = stage.in(h->sTheta, theta, nS * p);
    const double* dscale = stage.in(h->sScale, scale, nS * m);
    const double* dcot = stage.in(h->sCot, cot, nS * ns);
    const double* dvZ = stage.in(h->sVZ, vZ, Zlen);
    const double* dvinit = stage.in(h->sVinit, vinit, ns);
    const double* dvtheta = stage.in(h->sVth, vtheta, nS * p);
    const double* dvscale = stage.in(h->sVsc, vscale, nS * m);
    const double* dvcot = stage.in(h->sVcot, vcot, nS * ns);
    double* dtgrad = stage.out(h->sTgrad, tgrad, Zlen);
    double* dtsamp = stage.out(h->sTgradS, tgrad_samples, n_samp);
    double* dtginit = stage.out(h->sTginit, tgrad_init, nS * ns);
    if ((rc = stage.status())) return rc;
    if ((rc = qc_sweep_hvp_launch(h, who, dZ, dinit, S, dtheta, dscale, dcot, dvZ, dvinit, dvtheta, dvscale, dvcot, dtgrad, dtsamp, dtginit, h->stream)))
        return rc;
    return stage.finish();
}
