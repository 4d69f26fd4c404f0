// Open-system sweep gradients: the backward walk that READS the forward states instead of reversing the step.  The closed walk of
// qc_sweep_grad.hip (read its header first) rebuilds x_t = E^T x_{t+1}, which holds for orthogonal E only; for a Lindblad generator or a
// non-Hermitian effective Hamiltonian E^T is not E^-1, and where it exists the inverse amplifies rounding by exp(gamma sum h).  Handles
// created with reserved1[0] = QC_SWEEP_STORED_STATES take this walk for qc_sweep_grad*, qc_sweep_grad_params* and qc_sweep_vjp*, whatever
// their generators ("mfma16-sweep" form: 2N <= 16, m <= 8, at most 16 state columns).
//
// The identities that never used antisymmetry, with G = G_s(a_t), h = dt_t, E = exp(hG), lambda_t = E^T lambda_{t+1}, K = lambda_{t+1} x_t^T:
//     dphi/da_{t,k} = c_k <h L(hG^T; K), G_k>            (L(X; .)* = L(X^T; .))
//     dphi/dh_t     = <K, L(hG; G)> = <L(hG^T; K), G>    (L(hG; G) = G E: the derivative of exp(hG) along h)
//     dphi/dtheta_j = sum_t <h L(hG^T; K), P_j>,   dphi/dc_k = sum_t a_{t,k} <h L(hG^T; K), G_k>
// x_t is read, so K is known before the interval's exponential and ONE paired chain gives E and the Frechet tile; no state is reversed and
// no product with E^T trails the chain.  The chain runs in the transposed frame, L(hG^T; K) = L(hG; K^T)^T: on the A-layout images the
// forward kernel uses, in direction K^T = x_t lambda_{t+1}^T.  Three things follow from that choice:
//   * E comes out in D layout, which read as the A operand IS E^T: lambda <- E^T lambda needs no transpose (as in the closed walk);
//   * the D-layout tile of L(hG; K^T), multiplied elementwise with an A-layout image, is the inner product of its transpose L(hG^T; K)
//     with that matrix: the drive, timestep and perturbation derivatives are contractions with tiles already in registers;
//   * the squaring rule sees hG itself: ||hG||_1 <= 2^sq / 8, the norm and the count of the forward kernel, so the stored states and the
//     walk use the same scaling.  (Transposed tiles would take ||hG^T||_1 = ||hG||_inf and could choose another sq.)  The truncation
//     bounds of qc_sweep_grad.hip's header need ||Y|| <= 1/8 in ONE submultiplicative norm, for the matrix the series runs on: here Y = hG / 2^sq
//     in the 1-norm, as there; nothing in them uses antisymmetry.  The direction is not scaled by h inside the chain (dY = K^T / 2^sq):
//     the unscaled tile is the timestep derivative's, h times it the drives' and parameters'.
//
// Launches (after the totals and the seed, which are those of the closed walk; the seed leaves x and lambda at every chunk end):
//   A. qc_sweep_open_store_kernel<M>, one wavefront per (sample, chunk): from the chunk-start state (init, or the previous chunk's end in
//      h->dXs) the interval body of the forward kernel with x <- E x in place of W <- E W; x_t of every knot t = t0 .. t1-1 goes to
//      h->dXall[s][t][2N x cols].  The chunk's last exponential is not needed (x_{t1} is the next chunk's start): chunk - 1 exponentials.
//      MFMAs per interval: 32 + 4 sq + 4.
//   B. qc_sweep_open_grad_kernel<M, PAR>, one wavefront per (sample, chunk), backwards.  Per interval, lambda the D-layout tile of knot t+1:
//        x_t^T                      read from dXall straight into the B-operand layout of x^T (an index pattern, no LDS)
//        lambda_A                   one LDS round trip (one tile)
//        KT = lambda x_t^T          mma(lambda_A, x_t^T): 4 MFMAs; read as an A operand it acts as K^T = x_t lambda^T
//        Y = h G / 2^sq, dY = KT / 2^sq, eight Horner steps (R, dR) <- (Y R + I/(k-1)!, dY R + Y dR)        8 x 12 MFMAs
//        sq squarings (E, dE) <- (E E, E dE + dE E)                                                         12 MFMAs, one LDS round trip each
//        dphi/dh = sum dE . Ga;   ZT = h dE;   dphi/da_k = c_k sum ZT . G_k       wave sums in a fixed order
//        lambda <- E^T lambda                                                      4 MFMAs
//      MFMAs per interval: 4 + 96 + 12 sq + 4 = 104 + 12 sq (closed walk: 112 + 12 sq).  The m + 1 values of the interval leave through one
//      vector store.  PAR as in the closed walk: Acc = sum_t ZT_t and the scale sums in the wave's LDS slice, contracted at the chunk's end.
// Two launches rather than a forward phase inside the walk: the store kernel keeps the forward kernel's registers and occupancy, the walk's
// budget (M = 8, and the parameter flavour at M = 6, are at their limit) is not shared with a second loop, and nothing relies on a wave
// reading back through the vector cache what it has just written.
// No atomics; every sum in a fixed order; no output's bits depend on which others were asked for.
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_sweep16_common.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep16;

// x_t of every knot of the chunk, t = t0 .. t1-1, from the chunk-start state
template <int M>
__global__ __launch_bounds__(64 * kWaves, 2) void qc_sweep_open_store_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                               const double* __restrict__ theta, const double* __restrict__ scale,
                                                                               const double* __restrict__ init, const double* __restrict__ xs,
                                                                               double* __restrict__ xall) {
    __shared__ double scr_all[kWaves * kTile];
    const WaveItem w = wave_item(kWaves);
    double* __restrict__ scr = scr_all + w.wq * kTile;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, c = ch.c, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    const int ns = P.n * P.nc;

    const v4d base = base_tile(P.img, m, P.p, theta, s, lane);
    v4d Gj[M];
    resident_tiles(P.img, m, lane, Gj);
    const int kl = lane < m ? lane : (m > 0 ? m - 1 : 0);
    const double cl = (scale && m > 0) ? scale[s * m + kl] : 1.0;

    v4d x;
    {
        const double* __restrict__ x0 = c == 0 ? init : xs + (item - 1) * ns;      // the previous chunk's end: same sample, c >= 1
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * r + g;
            x[r] = (row < P.n && j < P.nc) ? x0[row + P.n * j] : 0.0;
        }
    }
    const double* __restrict__ z = Z + (long long)t0 * P.zdim;
    double av = m > 0 ? z[P.off_a + kl] : 0.0;
    const double hfix = opaque_scalar(P.dt_fixed);
    double h = ft ? z[P.off_dt] : hfix;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        double* __restrict__ xo = xall + (s * P.n_int + t) * ns;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * r + g;
            if (row < P.n && j < P.nc) xo[row + P.n * j] = x[r];
        }
        if (t + 1 == t1) break;      // x_{t1} is the next chunk's start
        const double* __restrict__ zn = Z + (long long)(t + 1) * P.zdim;
        const double av_n = m > 0 ? zn[P.off_a + kl] : 0.0;
        const double h_n = ft ? zn[P.off_dt] : hfix;
        const double al = av * cl;
        const v4d Ga = generator(base, Gj, m, al);
        const int sq = squarings(h, Ga);
        const v4d Y = (h * ldexp(1.0, -sq)) * Ga;
        v4d R = kInvFact[kDeg] * IdB;
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) R = mma16(Y, R, kInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            const v4d Et = lds_transpose16(scr, R, g, j);
            R = mma16(Et, R, zero);
        }
        const v4d Et = lds_transpose16(scr, R, g, j);     // E^T in D layout = E in A layout
        x = mma16(Et, x, zero);
        av = av_n;
        h = h_n;
    }
}

// x_t^T in the B-operand layout, straight from the stored state: lane (g, j) reg r = x[j][4r+g] at xp[4 n r], xp the lane's own pointer
// to x[j][g]; bit r of `ok` says whether the entry exists (j < n and 4r+g < cols), everything else of the tile is zero
__device__ __forceinline__ v4d load_xT(const double* __restrict__ xp, int n4, int ok) {
    v4d x;
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = ((ok >> r) & 1) ? xp[n4 * r] : 0.0;
    return x;
}

// One wavefront per (sample, chunk), walking the chunk backwards on the stored states.  The flavours and `part` / `gs` as
// qc_sweep_grad_kernel (qc_sweep_grad.hip).
template <int M, bool PAR = false>
__global__ __launch_bounds__(64 * kWaves, 2) void qc_sweep_open_grad_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                              const double* __restrict__ theta, const double* __restrict__ scale,
                                                                              const double* __restrict__ xall, const double* __restrict__ ls,
                                                                              double* __restrict__ gs, double* __restrict__ part) {
    constexpr bool kTight = M >= 6 || PAR;      // the flavours whose loop-invariant lane masks do not fit the scalar registers
    __shared__ double scr_all[kWaves * kWalkSlice<PAR>];
    const WaveItem w = wave_item(kWaves);
    double* __restrict__ scr = scr_all + w.wq * kWalkSlice<PAR>;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    const int ns = P.n * P.nc;

    // ---- once per wave: the sample's base tile, the drive tiles, the adjoint at the chunk's end ------------------------------------
    const v4d base = base_tile(P.img, m, P.p, theta, s, lane);
    v4d Gj[M];
    resident_tiles(P.img, m, lane, Gj);
    const int kl = lane < m ? lane : (m > 0 ? m - 1 : 0);
    const double cl = (scale && m > 0) ? scale[s * m + kl] : 1.0;

    v4d lam;
    {
        const double* __restrict__ le = ls + item * ns;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * r + g;
            lam[r] = (row < P.n && j < P.nc) ? le[row + P.n * j] : 0.0;
        }
    }
    // the lane's pointer into the stored states (knot t of sample s at xall + (s (T-1) + t) ns) and the mask of its entries
    int okx = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) okx |= (j < P.n && 4 * r + g < P.nc) ? (1 << r) : 0;
    const double* xp = xall + (s * P.n_int + (t1 - 1)) * ns + (okx ? j + P.n * g : 0);
    const int n4 = 4 * P.n;
    v4d xT = load_xT(xp, n4, okx);

    const double hfix = opaque_scalar(P.dt_fixed);
    // the lane's control of the interval (lane l: drive min(l, m-1)) and, `dto` entries further, the timestep: one pointer walking down
    const double* ap = Z + (long long)(t1 - 1) * P.zdim + P.off_a + kl;
    const int dto = P.off_dt - P.off_a - kl;
    double av = m > 0 ? ap[0] : 0.0;
    double h = ft ? ap[dto] : hfix;
    // the lane's slot of the interval's one store (lane k: drive k, lane m: timestep), a pointer of its own walking down with t
    double* gp = gs + (s * P.n_int + (t1 - 1)) * P.nd + lane;
    const int stl = (gs && lane < P.nd) ? 1 : 0;
    // PAR: the accumulators of qc_sweep_grad_kernel, at the same places of the wave's LDS slice
    double* accl = scr + 2 * kTile;
    if constexpr (PAR) {
#pragma unroll
        for (int r = 0; r < 4; ++r) accl[64 * r + lane] = 0.0;
        accl[320 + lane] = 0.0;
    }
#pragma unroll 1
    for (int t = t1 - 1; t >= t0; --t) {
        if (t > t0) ap -= P.zdim;      // the interval below is requested before this interval's products
        const double av_n = m > 0 ? ap[0] : 0.0;
        const double h_n = ft ? ap[dto] : hfix;
        const double al = av * cl;
        if constexpr (PAR) accl[256 + lane] = av;
        const v4d Ga = generator(base, Gj, m, al);
        const int sq = squarings(h, Ga);
        const double sc = ldexp(1.0, -sq);
        // KT = lambda_{t+1} x_t^T (D layout): as an A operand it acts as K^T = x_t lambda^T, the direction of the chain on hG
        const v4d lamA = lds_transpose16(scr, lam, g, j);
        const v4d KT = mma16(lamA, xT, zero);
        // the state of the interval below is requested before this interval's chain
        {
            int ok = okx;      // likewise the four masks of the state's padding
            if constexpr (kTight) asm volatile("" : "+v"(ok));
            if (t > t0) xp -= ns;
            xT = load_xT(xp, n4, ok);
        }
        const v4d Y = (h * sc) * Ga;
        const v4d dY = sc * KT;
        v4d R = kInvFact[kDeg] * IdB;
        v4d dR = zero;
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) step16(Y, dY, R, dR, kInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            const v4d in[2] = {R, dR};
            v4d tr[2];
            lds_transpose16_multi<2>(scr, in, tr, g, j);      // E^T, dE^T in D layout = E, dE in A layout
            step16(tr[0], tr[1], R, dR, zero);
        }
        // dR = L(hG; K^T) = L(hG^T; K)^T: against an A-layout tile it is its own transpose
        int ln = lane;      // as in qc_sweep_grad_kernel: the lane compares are made per interval, not kept in scalar registers
        if constexpr (kTight) asm volatile("" : "+v"(ln));
        double out = 0.0, duv = 0.0;      // duv (PAR): lane k holds du_k = sum ZT . G_k
        const v4d ZT = h * dR;
#pragma unroll
        for (int u = 0; u < M; ++u) {
            if (u < m) {      // (the branches also keep the wave sums apart: side by side their lane reads fill the scalar registers)
                double pu = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) pu = fma(ZT[r], Gj[u][r], pu);
                const double du = wave_sum(pu);
                if constexpr (PAR) duv = ln == u ? du : duv;
                else out = ln == u ? du * cl : out;
            }
        }
        double dh = 0.0;
        if (ft && (!PAR || gs)) {
            double ph = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) ph = fma(dR[r], Ga[r], ph);
            dh = wave_sum(ph);
        }
        if constexpr (PAR) {
#pragma unroll
            for (int r = 0; r < 4; ++r) accl[64 * r + lane] += ZT[r];
            accl[320 + lane] = fma(accl[256 + lane], duv, accl[320 + lane]);       // lanes >= m: duv = 0
            out = ln < m ? duv * cl : dh;
        } else {
            out = ln == m ? dh : out;
        }
        {
            int st = stl;
            if constexpr (kTight) asm volatile("" : "+v"(st));
            if (st) *gp = out;
            gp -= P.nd;
        }
        lam = mma16(R, lam, zero);
        av = av_n;
        h = h_n;
    }
    if constexpr (PAR) {
        v4d Acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) Acc[r] = accl[64 * r + lane];
        double acc_t = 0.0;
        for (int q = 0; q < P.p; ++q) {
            const v4d Pq = image_tile(P.img, 1 + m + q, lane);
            double pq = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) pq = fma(Acc[r], Pq[r], pq);
            const double dq = wave_sum(pq);
            acc_t = lane == q ? dq : acc_t;
        }
        double* __restrict__ po = part + item * (P.p + m);
        if (lane < P.p) po[lane] = acc_t;
        if (lane < m) po[P.p + lane] = accl[320 + lane];
    }
}

}  // namespace

void qc_sweep_open_launch_walk(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                               int64_t chunk, int64_t n_chunks, double* gs, bool want_par, double* dgrad_theta, double* dgrad_scale, hipStream_t st) {
    const SweepParams P = qc_sweep_params(h, S, chunk, n_chunks);
    const unsigned grid = qc_sweep_grid(P, kWaves);
#define QC_OPEN_LAUNCH(M_)                                                                                                                      \
    do {                                                                                                                                        \
        hipLaunchKernelGGL(qc_sweep_open_store_kernel<M_>, dim3(grid), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale, dinit,                  \
                           (const double*)h->dXs.p, h->dXall.p);                                                                                \
        if (want_par)                                                                                                                           \
            hipLaunchKernelGGL((qc_sweep_open_grad_kernel<M_, true>), dim3(grid), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale,               \
                               (const double*)h->dXall.p, (const double*)h->dLs.p, gs, h->dPart.p);                                             \
        else                                                                                                                                    \
            hipLaunchKernelGGL((qc_sweep_open_grad_kernel<M_, false>), dim3(grid), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale,              \
                               (const double*)h->dXall.p, (const double*)h->dLs.p, gs, (double*)nullptr);                                       \
    } while (0)
    QC_SWEEP_FOR_M(P.m, QC_OPEN_LAUNCH);
#undef QC_OPEN_LAUNCH
    if (want_par) qc_sweep_launch_par_reduce(h, S, n_chunks, dgrad_theta, dgrad_scale, st);
}
