// Sweep gradients and pullbacks for "mfma64-sweep" handles (32 < 2N <= 64, descriptors with QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 |
// QC_SWEEP_WIDE_64_GRAD): the closed adjoint walk of qc_sweep_grad.hip with every matrix 4 x 4 tiles of 16 x 16 in LDS.  The mathematics is
// that file's, line for line (read its header first, then qc_sweep32_grad.hip): antisymmetric generators make E orthogonal, so
//     x_t = E^T x_{t+1},  lambda_t = E^T lambda_{t+1}                  (no state stored inside a chunk),
//     one Frechet chain per interval in direction dY = (h / 2^sq) x_{t+1} lambda_{t+1}^T, run beside the Horner chain,
//     sq squarings dE <- E dE + dE E, E <- E E,      ZT = E^T dE,
//     dF/da_k = c_k sum ZT . G_k   (sum_ab ZT[a][b] G_k[b][a]),      dF/dh = -sum KT . G   (KT = lambda x^T).
// Degree, threshold, the 1/k! table, generator(), squarings() and chunk_range are the forward kernel's (qc_sweep64_common.h,
// qc_sweep_common.h): the walk chooses the forward step's sq from the same norm, and its R chain is tile_mul's chain, MFMA for MFMA.
//
// Work item: one WORKGROUP of 1024 threads per (sample, chunk), as in qc_sweep64.hip; wave w owns tile (I, J) = (w & 3, w >> 2) of every
// 64 x 64 product.  The chunk rule is the forward form's (kSweepFill64), unchanged.  States of up to 32 columns: x, lambda and u are
// 64 x 32 (4 x 2 tiles; the columns past nc are zero), wave w owns tile (w & 3, (w >> 2) & 1) of x (w < 8) or of lambda (w >= 8).
//
// LDS map (doubles; column stride 66 everywhere), 152 064 B dynamic + 2 304 B static of the CU's 160 KiB, one workgroup per CU:
//     Y | R | dR | x | lambda | u         64 x 64 | 64 x 64 | 64 x 64 | 64 x 32 | 64 x 32 | 64 x 32
// Six full matrices (Y, dY, two R and two dR buffers) would not fit.  Two things make the walk fit:
//   (a) dY has rank <= nc: dY R = (h / 2^sq) x (lambda^T R).  dY is never formed; the term is two thin products through
//       u = (h / 2^sq) R^T lambda (64 x nc): 4 nct tile chains of 16 for u and nct x 4 MFMAs a tile for x u^T (nct = 1 or 2 column tiles);
//   (b) a wave's tile of a product is 4 registers a lane, so R and dR are updated IN PLACE: every wave holds its tiles of the new R, dR in
//       registers across a barrier (all reads of the old ones are done), writes them over the old ones, and a second barrier publishes them.
// The LDS map, (a), (b) and the exponential pair itself are qc_sweep64_common.h's (walk_lds, exp_pair), shared with the noise walk of
// qc_sweep64_noise.hip; so are the state load, the timestep derivative (kt_dot) and the 16-wave sum (part_sum).
// Barriers of one interval, in order, and what each stands between:
//     S   inside squarings(): behind it every wave has left the previous interval -- its ZT and E^T x products (the last reads of R, dR)
//         are in front of Ba already; S stands between the writes of x, lambda (after Ba) and their reads by the timestep derivative,
//         and between red[]'s writes and reads.  Y, R = I/8!, dR = 0 are written behind S.
//     H0, U / P / W per Horner step, P / W per squaring: inside exp_pair, argued there.
//     tail:  ZT = E^T dE (registers), x' / lambda' = E^T x / E^T lambda (registers), the m contractions of ZT with the drive images
//            (global memory, L2-resident), wave sums, part[w][.]
//     Ba  every read of E, dE, x, lambda is done and part[] is complete;   x, lambda <- x', lambda';  wave 0 adds the 16 partials of each of
//         the m + 1 values in ascending wave order and stores them with one vector store into gs[s][t][.]
// red[] keeps the rule stated at squarings() (at least one barrier between a call and the next: there are 25 or more); part[] is written
// in the tail and read behind Ba, and its next writes are a whole interval of barriers later.
// E^T X needs no transposition: the A operand of E^T is the column fragment of E (qc_sweep64_common.h: col_frag), conflict-free by the stride.
//
// MFMAs per interval and workgroup, nct = ceil(nc / 16):  8 Horner steps x (16 x (32 + 4 nct) + 4 nct x 16) + sq x 16 x 48 + 16 x 16 (ZT)
// + 8 nct x 16 (x, lambda) = (4352 + 1152 nct) + 768 sq, against the forward kernel's (9 + sq) x 256 = 2304 + 256 sq.
// No atomics, sums in a fixed order: repeated calls give the same bits.  The stored-state walk is qc_sweep64_open_grad.hip's (QC_SWEEP_WIDE_64_STORED), on the same shared pieces; Hessian products are
// not served in this form; pushforwards are qc_sweep64_jvp.hip's (QC_SWEEP_WIDE_64_TANGENT), noise sweeps qc_sweep64_noise.hip's (QC_SWEEP_WIDE_64_NOISE), a second walk on the same shared pieces.
//
// The parameter flavour <true> (handles with QC_SWEEP_WIDE_64_PARAMS; qc_sweep_grad_params*, grad_theta / grad_scale of qc_sweep_vjp*) adds,
// per (sample, chunk), the p + m chunk shares
//     dF_s/dtheta_q: sum_{t in chunk} sum ZT_t . P_q,      dF_s/dc_k: sum_{t in chunk} a_{t,k} du_{t,k},   du_{t,k} = sum ZT_t . G_k
// (du BEFORE the factor c_k and a the unscaled control: no division by c, so the derivative is defined at c = 0).  The scheme of the
// smaller forms -- a running Acc = sum_t ZT_t, contracted once at the chunk's end -- does not fit: 32 KiB of LDS where 9 472 B are free,
// or four more registers a lane where none is.  Instead the tail's image loop runs over the m + p images (the perturbation images
// follow the drive images in P.img: the same four loads and one wave sum each), perturbation q's wave sum goes to lane nd + q, behind
// the timestep's lane, part[][] has rows of nd + p <= 25 values (3 200 B), and wave 0, which adds the 16 partials behind Ba anyway,
// keeps the chunk's running sums, one value a lane (lane k < m: += a_k acc; lane nd + q: += acc), and stores them after the chunk's
// last interval with one vector store into par[item][p + m] (perturbations, then drives: what qc_sweep_par_reduce_kernel reads).  The
// running sums live in runs[25] (200 B of LDS; static LDS 3 528 B in all), not in a register pair: held in registers the flavour needs
// 130 a lane and spills.  Not one MFMA is added.  Barriers: the widened part[] keeps part[]'s rule -- written in the tail, Ba stands
// between those writes and wave 0's reads, and the next writes are a whole interval of barriers later; runs[l] is written and read by
// lane l of wave 0 and by nobody else (zeroed by it before the walk, updated behind Ba, read back for the final store), so it needs no
// barrier at all.  With gs = NULL (only parameter outputs asked for) the timestep's KT sum
// and the per-interval store are skipped.  The flavour <false> is the walk as it was before the second flavour existed.
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_side.h"
#include "qc_sweep64_common.h"
#include "qc_sweep64_launch.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep64;

// values a wave leaves per interval: m + 1 <= 17; the parameter flavour adds the p <= 8 perturbation sums behind them, nd + p <= 25
template <bool PAR> constexpr int kPartLd = PAR ? 25 : 17;

// PAR = false: the per-interval derivatives only (`par` unused).  PAR = true, the parameter flavour, also accumulates the chunk's shares of
// dF_s/dtheta_q = sum_t sum(ZT_t . P_q) and dF_s/dc_k = sum_t a_{t,k} sum(ZT_t . G_k) and stores them at the chunk's end as
// par[item][p + m] (perturbations, then drives); `gs` may then be NULL (no per-interval store, no timestep derivative).
template <bool PAR>
__global__ __launch_bounds__(kThreads, 1) void qc_sweep64_grad_kernel(const SweepParams P, const double* __restrict__ Z, const double* __restrict__ theta,
                                                                        const double* __restrict__ scale, const double* __restrict__ xs,
                                                                        const double* __restrict__ ls, double* __restrict__ gs,
                                                                        double* __restrict__ par) {
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
    double* const mine = J >= 2 ? lds.L : lds.X;      // waves 8 .. 15 carry lambda's tile (I, Jc) through E^T, waves 0 .. 7 x's

    // ---- once per item: the sample's base matrix, the state and the adjoint at the chunk's end (zero outside n x nc) -----------------
    double base[4];
    base_elems(P.img, m, P.p, theta, s, tid, base);
    const DriveLane dl = drive_lane(scale, m, s, lane);
    const int kl = dl.kl;
    const double cl = dl.cl;
    load_state(xs + item * (P.n * nc), P.n, nc, tid, lds.X);
    load_state(ls + item * (P.n * nc), P.n, nc, tid, lds.L);

    const gptr G0 = (gptr)(unsigned long long)P.img;
    const double* __restrict__ z = Z + (long long)(t1 - 1) * P.zdim;
    double av = drive_value(z, P.off_a, m, kl);
    const double hfix = opaque_scalar(P.dt_fixed);
    double h = ft ? z[P.off_dt] : hfix;
    // PAR: the images contracted per interval (drives, then perturbations: they follow each other in P.img), the values a wave leaves
    // (perturbation q in lane nd + q, behind the timestep's lane)
    // (the scalar registers are as scarce here as the vector ones: nd is spelled m + ft and the share's address is made once, per lane,
    // so that neither P.nd, `par` nor the item's offset stays live across the walk)
    const int nd = PAR ? m + (ft ? 1 : 0) : P.nd;
    const int n_img = PAR ? m + P.p : m;
    const int n_val = PAR ? n_img + (ft ? 1 : 0) : P.nd;
    const int mine_img = !PAR || lane < m ? lane : lane >= nd ? lane - (nd - m) : -1;      // the image whose wave sum the lane keeps
    // the lane's share: perturbations, then drives (the layout qc_sweep_par_reduce_kernel reads)
    double* share = PAR ? par + item * (P.p + m) + (lane < m ? P.p + lane : lane - nd) : nullptr;
    if constexpr (PAR) asm volatile("" : "+v"(share));      // made here, not at the chunk's end
    if constexpr (PAR) {
        if (w == 0 && lane < kPartLd<true>) runs[lane] = 0.0;      // read and written by wave 0's lane `lane` alone: no barrier
    }
#pragma unroll 1
    for (int t = t1 - 1; t >= t0; --t) {
        // the previous interval's controls and timestep are requested before this interval's products
        const double* __restrict__ zn = Z + (long long)(t > t0 ? t - 1 : t) * P.zdim;
        const double av_n = drive_value(zn, P.off_a, m, kl);
        const double h_n = ft ? zn[P.off_dt] : hfix;
        double G[4];
        generator(P.img, m, av * cl, base, tid, G);
        const int sq = squarings(red, G, h, lane, w);      // barrier S; the rule of the forward kernel: one function
        const double hs = h * ldexp(1.0, -sq);
        // lane k < m: drive k's wave sum; lane m: the timestep's (sum KT . G, its sign at the store)
        double out = 0.0;
        if (ft && (!PAR || gs)) {
            const double dh = kt_dot(lds.X, lds.L, nc, G, lane, w);
            out = lane == m ? dh : out;
        }
        exp_pair(lds, G, hs, sq, nct, tid, I, J, g, j);      // barriers H0, U / P / W per Horner step, P / W per squaring
        // ZT = E^T dE, the wave's tile of x or lambda through E^T, and the drive derivatives
        const v4d ZT = chain<kColStep, kColStep, 16>(col_frag(lds.R, I, g, j), col_frag(lds.dR, J, g, j), zero);
        v4d nx = zero;
        if (Jc < nct) nx = chain<kColStep, kColStep, 16>(col_frag(lds.R, I, g, j), col_frag(mine, Jc, g, j), zero);
        // the lane's elements ZT[a = 16 I + 4 r + g][b = 16 J + j] against G_u[b][a] (column-major images: a * 64 + b)
        const gptr Ge = G0 + (16 * I + g) * 64 + 16 * J + j;
#pragma unroll 1
        for (int u = 0; u < n_img; ++u) {
            const gptr Gu = Ge + (size_t)(1 + u) * kImg;
            double pu = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) pu = fma(ZT[r], Gu[256 * r], pu);
            const double du = wave_sum(pu);
            out = mine_img == u ? du : out;
        }
        // PAR: kept loop-invariant, the lane compares of the tail live in scalar register pairs and the kernel spills some of them; an
        // opaque copy of the lane index has them made per interval instead
        int ln = lane;
        if constexpr (PAR) asm volatile("" : "+v"(ln));
        if (ln < n_val) part[w * kPartLd<PAR> + lane] = out;
        __syncthreads();      // Ba
        if (Jc < nct) store_tile(mine, I, Jc, g, j, nx);
        if (w == 0 && ln < n_val) {
            const double acc = part_sum<kPartLd<PAR>>(part, lane);
            if constexpr (PAR) {
                // lane k < m: du_k BEFORE the factor c_k against the unscaled control (no division by c); the timestep's lane adds
                // nothing that is read; lane nd + q: perturbation q's sum
                const double run = runs[lane];
                runs[lane] = ln < m ? fma(av, acc, run) : run + acc;
                if (gs && ln < nd) gs[(s * P.n_int + t) * nd + lane] = ln < m ? acc * cl : -acc;
            } else {
                gs[(s * P.n_int + t) * P.nd + lane] = lane < m ? acc * cl : -acc;
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

int qc_sweep64_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, int64_t chunk, int64_t n_chunks,
                           double* gs, bool want_par, double* par, hipStream_t st) {
    const SweepParams P = qc_sweep_params(h, S, chunk, n_chunks);
    const auto walk = want_par ? qc_sweep64_grad_kernel<true> : qc_sweep64_grad_kernel<false>;
    QC_SWEEP64_LAUNCH(h, walk, kWalkLdsBytes, P, st, dZ, dtheta, dscale, (const double*)h->dXs.p, (const double*)h->dLs.p, gs,
                      want_par ? par : (double*)nullptr);
    return QC_OK;
}
