// Open-system sweep gradients for "mfma64-sweep" handles (32 < 2N <= 64): the stored-state walk of qc_sweep_open_grad.hip with every matrix
// 4 x 4 tiles of 16 x 16 in LDS.  The mathematics is that file's (read its header first, then qc_sweep64_grad.hip for the tiles): with
// G = G_s(a_t), h = dt_t, E = exp(hG), lambda_t = E^T lambda_{t+1} and x_t READ from the stored forward states,
//     dE_h = h L(hG; x_t lambda_{t+1}^T)                                  (L: the Frechet derivative of exp at hG)
//     dphi/da_{t,k} = c_k sum_ab dE_h[a][b] G_k[b][a]
//     dphi/dtheta_q = sum_t sum_ab dE_h[a][b] P_q[b][a],    dphi/dc_k = sum_t a_{t,k} sum_ab dE_h[a][b] G_k[b][a]      (before the factor c_k)
//     dphi/dh_t     = lambda_{t+1}^T G x_{t+1}                             (no sign flip, defined at h = 0)
// Nothing asks anything of the generators.  Taken by handles whose descriptor has reserved1[0] = QC_SWEEP_STORED_STATES and wide =
// QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_STORED (with QC_SWEEP_WIDE_64_PARAMS for the parameter flavour),
// for qc_sweep_grad*, qc_sweep_grad_params* and qc_sweep_vjp*, antisymmetric generators included; at most 32 state columns.
// generator(), squarings() and chunk_range are the forward kernel's (qc_sweep64_common.h, qc_sweep_common.h): the forward step, the stored
// states and the walk choose the same sq from the same norm.
//
// Launches (after the totals and the seed of the closed walk, which leave x and lambda at every chunk end in h->dXs / h->dLs):
//   A. qc_sweep64_open_store_kernel, one workgroup of 16 waves per (sample, chunk): from the chunk-start state (init, or the previous
//      chunk's end) the interval body of qc_sweep_mfma64_kernel<false> with x <- E x in place of W <- E W; x_t of every knot
//      t = t0 .. t1-1 goes to h->dXall[s][t][2N x cols] (64-bit indices).  The chunk's last exponential is skipped; a chunk of one interval
//      writes its start state and forms no exponential at all.  LDS (kLdsBytes, the forward kernel's 135 168 B):
//          Y | Ra | Rb | xa | xb          64 x 64 | 64 x 64 | 64 x 64 | 64 x 32 | 64 x 32
//      Barriers of one interval, in order: T publishes x_t (written by load_state, or by the 4 nct waves of the previous interval's x
//      product) to the global store below it and to this interval's product; S inside squarings(): every wave has left the previous
//      interval's product (its reads of E), so Y and Ra are written behind it; one barrier behind those writes and one behind each of
//      the 8 + sq products (a product reads two buffers and writes a third).  The x product reads E and x and writes the other thin
//      buffer, which was last read (the global store, the previous product) in front of S.  red[] keeps the rule stated at squarings().
//      MFMAs per interval: (8 + sq) x 256 + 64 nct, nct = ceil(cols / 16).
//   B. qc_sweep64_open_grad_kernel<PAR>, one workgroup per (sample, chunk), backwards: the closed walk of qc_sweep64_grad.hip without the
//      ZT = E^T dE product and without x <- E^T x.  LDS: the walks' map (walk_lds, 152 064 B dynamic), unchanged:
//          Y | R | dR | x | lambda | u
//      exp_pair (qc_sweep64_common.h) leaves E in R and dE_h in dR when x holds x_t and lambda holds lambda_{t+1}: it is called as it
//      stands.  The timestep term is kt_dot with its two state arguments exchanged, taken from x_{t+1} and lambda_{t+1} while both are
//      still in LDS: at the top of interval t the buffer x still holds x_{t+1} (for the chunk's last interval x_{t1} from h->dXs), and
//      x_t, requested from dXall before the generator is formed, replaces it behind the term.
//      Barriers of one interval, in order, and what each stands between:
//          S   inside squarings(): stands between the write of lambda (behind the previous Ba) and its reads (kt_dot here, exp_pair
//              below), and between red[]'s writes and reads; every wave has left the previous tail (its reads of R and dR are in front
//              of Ba), so Y, R = I/8!, dR = 0 are written behind S.
//          K   every read of x_{t+1} (kt_dot; the previous interval's exp_pair read x in front of its last P) is done;  x <- x_t, two
//              elements a thread from registers
//          H0  inside exp_pair: publishes x_t with Y, R, dR; then U / P / W per Horner step, P / W per squaring, argued there.
//          tail: the wave's tile of dE_h (read back from dR: the tile the wave wrote itself, published by W), lambda' = E^T lambda
//                (waves 8 .. 8 + 4 nct - 1, registers), the contractions with the images, wave sums, part[w][.]
//          Ba  every read of E, dE_h and lambda is done and part[] is complete; lambda <- lambda'; wave 0 adds the 16 partials in
//              ascending wave order and stores.
//      part[] and runs[] keep the rules of qc_sweep64_grad.hip.  MFMAs per interval: 8 x (16 x (32 + 4 nct) + 4 nct x 16) + sq x 768
//      + 4 nct x 16 = 4096 + 1088 nct + 768 sq (closed walk: 4352 + 1152 nct + 768 sq).
//      PAR as qc_sweep64_grad_kernel<true>: the image loop runs over the m + p images, wave 0 keeps the chunk's running sums in runs[],
//      the chunk's shares go to par[item][p + m] and qc_sweep_par_reduce_kernel adds them; gs may be NULL.  Both flavours form the
//      per-interval values by the same operations on the same operands: the same bits.
// No atomics; every sum in a fixed order; no output's bits depend on which others were asked for.  Resources: DESIGN.md 5.8.17.
// Restated from qc_sweep64_grad.hip, not shared: the tail's image contraction and the parameter flavour's bookkeeping (one user each
// until now; lifting them into qc_sweep64_common.h would move the closed walk's registers, which has none to spare).
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_side.h"
#include "qc_sweep64_common.h"
#include "qc_sweep64_launch.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep64;

// x_t of every knot of the chunk, t = t0 .. t1-1, from the chunk-start state
__global__ __launch_bounds__(kThreads, 1) void qc_sweep64_open_store_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                              const double* __restrict__ theta, const double* __restrict__ scale,
                                                                              const double* __restrict__ init, const double* __restrict__ xs,
                                                                              double* __restrict__ xall) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double red[16];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, j = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), I = w & 3, J = w >> 2;
    const long long item = blockIdx.x;
    const ChunkRange ch = chunk_range(item, P.n_chunks, P.chunk, P.n_int);
    const int t0 = ch.t0, t1 = ch.t1, m = P.m, n = P.n, nc = P.nc;
    const int nct = nc > 16 ? 2 : 1;
    const long long s = ch.s;
    const bool ft = P.off_dt >= 0;
    const long long ns = (long long)n * nc;
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    double* const Y = sm;
    double* xc = sm + 3 * kMat;              // x_t
    double* xn = sm + 3 * kMat + kThin;      // where the product leaves x_{t+1}
    load_state(ch.c == 0 ? init : xs + (item - 1) * ns, n, nc, tid, xc);      // the previous chunk's end: same sample, c >= 1
    if (t1 - t0 < 2) {
        // one interval: the start state as it was read (every thread stores what it loaded itself), no exponential, no barrier
        double* __restrict__ o = xall + (s * P.n_int + t0) * ns;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int idx = tid + 1024 * e, row = idx & 63, col = idx >> 6;
            if (row < n && col < nc) o[row + n * col] = xc[col * kLd + row];
        }
        return;
    }
    double base[4];
    base_elems(P.img, m, P.p, theta, s, tid, base);
    const DriveLane dl = drive_lane(scale, m, s, lane);
    const int kl = dl.kl;
    const double cl = dl.cl;

    const double* __restrict__ z = Z + (long long)t0 * P.zdim;
    double av = drive_value(z, P.off_a, m, kl);
    const double hfix = opaque_scalar(P.dt_fixed);
    double h = ft ? z[P.off_dt] : hfix;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        __syncthreads();      // T
        {
            double* __restrict__ o = xall + (s * P.n_int + t) * ns;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int idx = tid + 1024 * e, row = idx & 63, col = idx >> 6;
                if (row < n && col < nc) o[row + n * col] = xc[col * kLd + row];
            }
        }
        if (t + 1 == t1) break;      // x_{t1} is the next chunk's start
        const double* __restrict__ zn = Z + (long long)(t + 1) * P.zdim;      // t + 1 < t1 <= T - 1
        const double av_n = drive_value(zn, P.off_a, m, kl);
        const double h_n = ft ? zn[P.off_dt] : hfix;
        double G[4];
        generator(P.img, m, av * cl, base, tid, G);
        const int sq = squarings(red, G, h, lane, w);      // barrier S; the rule of the forward kernel: one function
        const double hs = h * ldexp(1.0, -sq);
        int oR = kMat, oN = 2 * kMat;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Y[lds_at(tid, e)] = hs * G[e];
            sm[oR + lds_at(tid, e)] = on_diagonal(tid, e) ? kInvFact[kDeg] : 0.0;
        }
        __syncthreads();
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) {
            tile_mul(Y, sm + oR, sm + oN, I, J, g, j, kInvFact[k - 1]);
            __syncthreads();
            const int o = oR; oR = oN; oN = o;
        }
#pragma unroll 1
        for (int q = 0; q < sq; ++q) {
            tile_mul(sm + oR, sm + oR, sm + oN, I, J, g, j, 0.0);
            __syncthreads();
            const int o = oR; oR = oN; oN = o;
        }
        // x_{t+1} = E x_t: tile (I, J) of the thin product on the waves 0 .. 4 nct - 1; published by the next interval's T
        if (J < nct) store_tile(xn, I, J, g, j, chain<kRowStep, kColStep, 16>(row_frag(sm + oR, I, g, j), col_frag(xc, J, g, j), zero));
        double* const o = xc; xc = xn; xn = o;
        av = av_n;
        h = h_n;
    }
}

// values a wave leaves per interval: m + 1 <= 17; the parameter flavour adds the p <= 8 perturbation sums behind them, nd + p <= 25
template <bool PAR> constexpr int kPartLd = PAR ? 25 : 17;

// One workgroup per (sample, chunk), walking the chunk backwards on the stored states.  The flavours, `par` and `gs` as
// qc_sweep64_grad_kernel (qc_sweep64_grad.hip).
template <bool PAR>
__global__ __launch_bounds__(kThreads, 1) void qc_sweep64_open_grad_kernel(const SweepParams P, const double* __restrict__ Z, const double* __restrict__ theta,
                                                                             const double* __restrict__ scale, const double* __restrict__ xall,
                                                                             const double* __restrict__ xs, const double* __restrict__ ls,
                                                                             double* __restrict__ gs, double* __restrict__ par) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double red[16];
    __shared__ double part[16 * kPartLd<PAR>];
    __shared__ double runs[PAR ? kPartLd<true> : 1];      // PAR: wave 0's running chunk sums, one a lane (<false>: unused, not allocated)
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, j = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), I = w & 3, J = w >> 2;
    const int Jc = J & 1;                   // the wave's column tile of a thin matrix
    const long long item = blockIdx.x;
    const ChunkRange ch = chunk_range(item, P.n_chunks, P.chunk, P.n_int);
    const int t0 = ch.t0, t1 = ch.t1, m = P.m, nc = P.nc;
    const int nct = nc > 16 ? 2 : 1;
    const long long s = ch.s;
    const bool ft = P.off_dt >= 0;
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    const WalkLds lds = walk_lds(sm);
    const bool lam_wave = J >= 2 && Jc < nct;      // waves 8 .. 15 carry lambda's tile (I, Jc) through E^T

    // ---- once per item: the sample's base matrix, x_{t1} and lambda_{t1} at the chunk's end, x_{t1 - 1} (zero outside n x nc) ------------
    double base[4];
    base_elems(P.img, m, P.p, theta, s, tid, base);
    const DriveLane dl = drive_lane(scale, m, s, lane);
    const int kl = dl.kl;
    const double cl = dl.cl;
    const int ns = P.n * nc;
    // the thread's two entries of a stored knot (load_state's map: row idx & 63, column idx >> 6), and whether each exists
    const int xrow = lane, xcol = tid >> 6;      // e = 1: column xcol + 16
    // (bit e of okx; the mask waits in a vector register: kept as two lane masks it would take four of the scalar registers, and the walk has none to spare)
    const int okx = (xrow < P.n && xcol < nc ? 1 : 0) | (xrow < P.n && xcol + 16 < nc ? 2 : 0);
    const double* xp = xall + (s * P.n_int + (t1 - 1)) * ns + (okx ? xrow + P.n * xcol : 0);      // e = 1: 16 n further (bit 1 implies bit 0)
    int nsv = ns;      // a knot's length and the mask wait in vector registers: the walk has no scalar register to spare
    asm volatile("" : "+v"(nsv));
    load_state(xs + item * ns, P.n, nc, tid, lds.X);      // x_{t1}: the timestep term of the chunk's last interval reads it
    load_state(ls + item * ns, P.n, nc, tid, lds.L);

    const gptr G0 = (gptr)(unsigned long long)P.img;
    const double* __restrict__ z = Z + (long long)(t1 - 1) * P.zdim;
    double av = drive_value(z, P.off_a, m, kl);
    const double hfix = opaque_scalar(P.dt_fixed);
    double h = ft ? z[P.off_dt] : hfix;
    // PAR: as qc_sweep64_grad_kernel<true> (the images contracted per interval, the values a wave leaves, the lane's share)
    const int nd = PAR ? m + (ft ? 1 : 0) : P.nd;
    const int n_img = PAR ? m + P.p : m;
    const int n_val = PAR ? n_img + (ft ? 1 : 0) : P.nd;
    const int mine_img = !PAR || lane < m ? lane : lane >= nd ? lane - (nd - m) : -1;      // the image whose wave sum the lane keeps
    double* share = PAR ? par + item * (P.p + m) + (lane < m ? P.p + lane : lane - nd) : nullptr;
    if constexpr (PAR) asm volatile("" : "+v"(share));      // made here, not at the chunk's end
    if constexpr (PAR) {
        if (w == 0 && lane < kPartLd<true>) runs[lane] = 0.0;      // read and written by wave 0's lane `lane` alone: no barrier
    }
#pragma unroll 1
    for (int t = t1 - 1; t >= t0; --t) {
        // the previous interval's controls and timestep are requested before this interval's products, and so is this interval's stored
        // state, which is not needed before K
        const double* __restrict__ zn = Z + (long long)(t > t0 ? t - 1 : t) * P.zdim;
        const double av_n = drive_value(zn, P.off_a, m, kl);
        const double h_n = ft ? zn[P.off_dt] : hfix;
        int ok = okx;      // the two masks of the state's padding are made per interval
        asm volatile("" : "+v"(ok));
        const double xt0 = (ok & 1) ? xp[0] : 0.0;
        const double xt1 = (ok & 2) ? xp[16 * P.n] : 0.0;
        xp -= nsv;      // (not read below knot t0)
        double G[4];
        generator(P.img, m, av * cl, base, tid, G);
        const int sq = squarings(red, G, h, lane, w);      // barrier S; the rule of the forward and the store kernel: one function
        const double hs = h * ldexp(1.0, -sq);
        // lane k < m: drive k's wave sum; lane m: the timestep's, lambda_{t+1}^T G x_{t+1} (kt_dot with the states exchanged: no sign)
        double out = 0.0;
        if (ft && (!PAR || gs)) {
            const double dh = kt_dot(lds.L, lds.X, nc, G, lane, w);
            out = lane == m ? dh : out;
        }
        __syncthreads();      // K
        lds.X[xcol * kLd + xrow] = xt0;      // x_t over x_{t+1}; published by H0
        lds.X[(xcol + 16) * kLd + xrow] = xt1;
        exp_pair(lds, G, hs, sq, nct, tid, I, J, g, j);      // barriers H0, U / P / W per Horner step, P / W per squaring
        // the wave's tile of dE_h, lambda's tile through E^T, and the drive derivatives
        v4d D;
        {
            const double* __restrict__ pd = lds.dR + (16 * J + j) * kLd + 16 * I + g;
#pragma unroll
            for (int r = 0; r < 4; ++r) D[r] = pd[4 * r];
        }
        v4d nl = zero;
        if (lam_wave) nl = chain<kColStep, kColStep, 16>(col_frag(lds.R, I, g, j), col_frag(lds.L, Jc, g, j), zero);
        // the lane's elements dE_h[a = 16 I + 4 r + g][b = 16 J + j] against G_u[b][a] (column-major images: a * 64 + b)
        const gptr Ge = G0 + (16 * I + g) * 64 + 16 * J + j;
#pragma unroll 1
        for (int u = 0; u < n_img; ++u) {
            const gptr Gu = Ge + (size_t)(1 + u) * kImg;
            double pu = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) pu = fma(D[r], Gu[256 * r], pu);
            const double du = wave_sum(pu);
            out = mine_img == u ? du : out;
        }
        int ln = lane;      // as in the closed walk: the lane compares are made per interval, not kept in scalar registers
        if constexpr (PAR) asm volatile("" : "+v"(ln));
        if (ln < n_val) part[w * kPartLd<PAR> + lane] = out;
        __syncthreads();      // Ba
        if (lam_wave) store_tile(lds.L, I, Jc, g, j, nl);
        if (w == 0 && ln < n_val) {
            const double acc = part_sum<kPartLd<PAR>>(part, lane);
            if constexpr (PAR) {
                // lane k < m: du_k BEFORE the factor c_k against the unscaled control (no division by c); the timestep's lane adds
                // nothing that is read; lane nd + q: perturbation q's sum
                const double run = runs[lane];
                runs[lane] = ln < m ? fma(av, acc, run) : run + acc;
                if (gs && ln < nd) gs[(s * P.n_int + t) * nd + lane] = ln < m ? acc * cl : acc;
            } else {
                gs[(s * P.n_int + t) * P.nd + lane] = lane < m ? acc * cl : acc;
            }
        }
        av = av_n;
        h = h_n;
    }
    if constexpr (PAR) {
        // the chunk's shares: one vector store of p + m lanes
        int w0 = w;      // (the mask of wave 0 is not kept across the walk either)
        asm volatile("" : "+s"(w0));
        if (w0 == 0 && mine_img >= 0 && mine_img < n_img) *share = runs[lane];
    }
}

}  // namespace

int qc_sweep64_open_launch_walk(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale, int64_t chunk,
                                int64_t n_chunks, double* gs, bool want_par, double* par, hipStream_t st) {
    const SweepParams P = qc_sweep_params(h, S, chunk, n_chunks);
    QC_SWEEP64_LAUNCH(h, qc_sweep64_open_store_kernel, kLdsBytes, P, st, dZ, dtheta, dscale, dinit, (const double*)h->dXs.p, h->dXall.p);
    const auto walk = want_par ? qc_sweep64_open_grad_kernel<true> : qc_sweep64_open_grad_kernel<false>;
    QC_SWEEP64_LAUNCH(h, walk, kWalkLdsBytes, P, st, dZ, dtheta, dscale, (const double*)h->dXall.p, (const double*)h->dXs.p, (const double*)h->dLs.p, gs,
                      want_par ? par : (double*)nullptr);
    return QC_OK;
}
