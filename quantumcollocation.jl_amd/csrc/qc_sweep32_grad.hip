// Sweep gradients for "mfma32-sweep" handles (16 < 2N <= 32, wide descriptors): the adjoint walk of qc_sweep_grad.hip with every matrix
// 2 x 2 tiles of 16 x 16.  The mathematics is that file's, line for line (read its header first): antisymmetric generators make E
// orthogonal, so x_t = E^T x_{t+1} (no state stored inside a chunk), L(hG; E^T K) = E^T L(hG; K) with K = x_{t+1} lambda_{t+1}^T (the
// Frechet chain runs beside the Horner chain), one chain per interval serves all m drives, dF/da_k = c_k sum ZT . G_k,
// dF/dh = -sum KT . G.  Degree 8, threshold 1/8, the 1/k! table, the generator and the squaring rule are the forward kernel's: both files
// take them from qc_sweep32_common.h; the paired column step and the product with E^T are those of qc_sweep32_walk.h, shared with the
// stored-state walk of qc_sweep32_open_grad.hip; the wave sum and the work item are the family's (qc_sweep_common.h).  The walk
// restates drive_lane, load_state (qc_sweep32_common.h), exp_pair, outer_kt and contract_image (qc_sweep32_walk.h), which
// qc_sweep32_noise_grad_kernel and qc_sweep32_jvp_kernel call: here the calls move the registers or the time of <false> ("Shared and restated in the wide kernels").
//
// Launches of one call on such a handle (qc_sweep_grad_launch of qc_sweep_grad.hip routes here):
//   1. qc_sweep_mfma32_kernel: the forward chunk totals, column-major 32 x 32;
//   2. qc_sweep32_seed_kernel (qc_sweep_grad.hip: the seed of that file at ld = 32), one workgroup per sample: x at every chunk end, the
//      fidelities with the bits of qc_sweep_eval on the same handle, lambda at every chunk end;
//   3. qc_sweep32_grad_kernel<false>, one wavefront per (sample, chunk), walking the chunk backwards.  X[I][J] is the tile of rows 16 I .. and
//      columns 16 J ..; the state and the adjoint are 32 x <= 16: two tiles each.  "A D-layout tile read as the A operand is its
//      transpose" holds per tile, so for a D-layout matrix M the A operand (I, K) of M^T is the tile M[K][I] as it stands (an index
//      swap), and the A operand (I, K) of M is the tile M[I][K] transposed through LDS.  Per interval:
//        KT[I][J] = lambda_I x_J^T                    four tiles transposed in one LDS round trip, 4 tile products
//        dF/dh = -sum_IJ KT[I][J] . Ga[J][I]          elementwise against the generator's A-layout tiles
//        Y = h G / 2^sq,  dY(I, K) = (h / 2^sq) KT[K][I]
//        R_k = Y R_k+1 + I/(k-1)!,  dR_k = dY R_k+1 + Y dR_k+1,  k = 8 .. 1     one tile column at a time, in place: column J of the
//                                                     results needs column J of R and dR only; six accumulator tiles, six chains
//        sq squarings: dE <- E dE + dE E, E <- E E    E, dE as A operands: eight tiles transposed in two LDS round trips of four
//        ZT[I][J] = sum_K R[K][I]^T dR[K][J]          E^T dE
//        dF/da_k = c_k sum_IJ ZT[I][J] . G_k[J][I]    the drive images read again from the image buffer (qc_sweep32.hip), m wave sums
//        x_I <- sum_K R[K][I]^T x_K,  lambda likewise
//      and the m + 1 values of the interval leave through one vector store (lane k: drive k, lane m: timestep).
//      MFMAs per interval: 16 + 8 x 96 + 96 sq + 32 + 32 = 848 + 96 sq, against the forward kernel's 288 + 32 sq (2.9x - 3x).
//   4. qc_sweep_grad_reduce_kernel / qc_sweep_J_kernel of qc_sweep_grad.hip, unchanged (they do not depend on the size).
// No atomics, sums in a fixed order: repeated calls give the same bits.
//
// Parameter gradients and cotangents (descriptors with wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_PARAMS): the flavour <true> of the walk, the
// flavour <M, true> of qc_sweep_grad.hip restated on 2 x 2 tiles.  Besides everything above it keeps, per (sample, chunk) wave,
//     Acc[I][J] = sum_t ZT_t[I][J]   (four tiles; ZT carries the factor h_t)   and, in lane k,   sum_t a_{t,k} du_{t,k},
// du_{t,k} = sum_IJ ZT[I][J] . G_k[J][I] BEFORE the factor c_k (no division by c: defined at c = 0), a_{t,k} the unscaled control.  At the
// chunk's end Acc is contracted once with every perturbation's image, dF_s/dtheta_q = sum_t sum(ZT_t . P_q), and the p + m shares go
// to part[item][p + m]; qc_sweep_par_reduce_kernel (qc_sweep_grad.hip) adds them in ascending chunk order.  16 double adds and one fma a
// lane and interval, p contractions a chunk, no MFMA more.  With gs = NULL the per-interval store and the timestep's wave sum are skipped.
// Acc lives in LDS behind the wave's transposition tiles: held in registers (32 a lane) the flavour spilled four vector and sixteen scalar
// registers; in LDS, with the addresses the chunk's end needs parked in vector registers, it spills nothing.  Two waves a workgroup
// (2 x 16.9 KB of LDS) instead of four: one wave per SIMD either way, and no static allocation beyond 64 KB.  The flavour <false> is
// instruction for instruction the walk as it was before the second flavour existed.
// gfx950 cross-compile: <false> 256 VGPRs + 96 AGPRs, 106 SGPRs, 34816 B LDS (four waves); <true> 248 VGPRs + 96 AGPRs, 106 SGPRs,
// 33792 B LDS (two waves); no private segment, no spills in either.
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_sweep32_common.h"
#include "qc_sweep32_walk.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep32;

// One wavefront per (sample, chunk), walking the chunk backwards.  PAR = false: the per-interval derivatives
// only (`part` unused).  PAR = true, the parameter flavour (qc_sweep_grad_kernel<M, true> on 2 x 2 tiles), also keeps Acc = sum_t ZT_t
// (four tiles) and, in lane k, sum_t a_{t,k} du_{t,k} with du_{t,k} = sum ZT . G_k BEFORE the factor c_k (no division by c: defined at
// c = 0), contracts Acc with every perturbation's image once at the chunk's end and stores the chunk's shares as part[item][p + m];
// `gs` may then be NULL (no per-interval store, no timestep derivative).  The per-interval values of the two flavours are the same
// operations on the same operands: the same bits.
template <bool PAR>
constexpr int kGW = PAR ? 2 : kWaves;                      // waves a workgroup: one wave per SIMD either way (512 registers a wave)
template <bool PAR>
constexpr int kGSl = PAR ? kScr + 16 * 64 : kScr;          // doubles of LDS a wave: the transposition tiles, PAR: and Acc behind them

template <bool PAR>
__global__ __launch_bounds__(64 * kGW<PAR>) void qc_sweep32_grad_kernel(const SweepParams P, const double* __restrict__ Z, const double* __restrict__ theta,
                                                                       const double* __restrict__ scale, const double* __restrict__ xs,
                                                                       const double* __restrict__ ls, double* __restrict__ gs,
                                                                       double* __restrict__ part) {
    __shared__ double scr_all[kGW<PAR> * kGSl<PAR>];
    const WaveItem w = wave_item(kGW<PAR>);
    double* __restrict__ scr = scr_all + w.wq * kGSl<PAR>;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    // ---- once per wave: the sample's base matrix, the state and the adjoint at the chunk's end --------------------------------------
    v4d base[2][2];
    base_matrix(P.img, m, P.p, theta, s, lane, base);
    const int kl = lane < m ? lane : (m > 0 ? m - 1 : 0);
    const double cl = (scale && m > 0) ? scale[s * m + kl] : 1.0;

    v4d x[2], lam[2];
    {
        const int ns = P.n * P.nc;
        const double* __restrict__ xe = xs + item * ns;
        const double* __restrict__ le = ls + item * ns;
#pragma unroll
        for (int I = 0; I < 2; ++I)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * I + 4 * r + g;
                const bool in = row < P.n && j < P.nc;
                x[I][r] = in ? xe[row + P.n * j] : 0.0;
                lam[I][r] = in ? le[row + P.n * j] : 0.0;
            }
    }

    const double hfix = opaque_scalar(P.dt_fixed);
    const double* __restrict__ z = Z + (long long)(t1 - 1) * P.zdim;
    double av = m > 0 ? z[P.off_a + kl] : 0.0;
    double h = ft ? z[P.off_dt] : hfix;
    // PAR: Acc = sum_t ZT_t lives in the wave's LDS slice (tile q of lane l, register r at accl[64 (4 q + r) + l]: every lane reads back
    // what it wrote itself, no barrier, one read / write pair per interval off the MFMA chain); lane k's sum_t a_{t,k} du_{t,k} in a register
    double* accl = scr + kScr;
    double accv = 0.0;
    if constexpr (PAR) {
#pragma unroll
        for (int i = 0; i < 16; ++i) accl[64 * i + lane] = 0.0;
    }
    // what the chunk's end needs waits in vector registers (the share's address per lane, p), and the lane's address in gs walks down
    // in one: the loop has no scalar register to spare
    double* po = nullptr;
    double* gp = nullptr;
    int pv = 0;
    int nde = P.nd;                  // PAR without gs: 0, no lane stores
    if constexpr (PAR) {
        po = part + item * (P.p + m) + lane;
        pv = P.p;
        asm volatile("" : "+v"(po), "+v"(pv));
        nde = gs ? P.nd : 0;
        gp = gs ? gs + (s * P.n_int + (t1 - 1)) * nde + lane : nullptr;
        asm volatile("" : "+v"(gp));
    }
#pragma unroll 1
    for (int t = t1 - 1; t >= t0; --t) {
        // the previous interval's controls and timestep are requested before this interval's products
        const double* __restrict__ zn = Z + (long long)(t > t0 ? t - 1 : t) * P.zdim;
        const double av_n = m > 0 ? zn[P.off_a + kl] : 0.0;
        const double h_n = ft ? zn[P.off_dt] : hfix;
        const double al = av * cl;
        v4d Y[2][2], dY[2][2];
        // PAR: the image buffer's address is taken anew where it is used, so that no derived address is kept across the interval
        const double* __restrict__ img = P.img;
        if constexpr (PAR) asm volatile("" : "+s"(img));
        generator(img, m, al, base, lane, Y);
        const int sq = squarings(Y, h);      // the rule of the forward kernel: one function
        const double hs = h * ldexp(1.0, -sq);
        // KT = lambda x^T of knot t+1 (D layout), from the transposed tiles of both; dY in A layout is KT with the block index swapped
        {
            const v4d in[4] = {x[0], x[1], lam[0], lam[1]};
            v4d tr[4];
            lds_transpose16_multi<4>(scr, in, tr, g, j);
            v4d k00 = zero, k01 = zero, k10 = zero, k11 = zero;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                k00 = __builtin_amdgcn_mfma_f64_16x16x4f64(tr[2][kk], tr[0][kk], k00, 0, 0, 0);
                k01 = __builtin_amdgcn_mfma_f64_16x16x4f64(tr[2][kk], tr[1][kk], k01, 0, 0, 0);
                k10 = __builtin_amdgcn_mfma_f64_16x16x4f64(tr[3][kk], tr[0][kk], k10, 0, 0, 0);
                k11 = __builtin_amdgcn_mfma_f64_16x16x4f64(tr[3][kk], tr[1][kk], k11, 0, 0, 0);
            }
            dY[0][0] = k00; dY[1][0] = k01; dY[0][1] = k10; dY[1][1] = k11;      // dY(I, K) = KT[K][I]
        }
        // an opaque copy of the lane index: the lane compares below are made per interval instead of living in scalar registers across
        // the loop (as in qc_sweep_grad_kernel at M = 8)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        double out = 0.0, duv = 0.0;      // duv (PAR): lane k holds du_k = sum ZT . G_k; lanes >= m keep 0
        if (PAR ? nde > m : ft) {       // PAR: only with gs (nde = nd = m + 1)
            const double dh = -wave_sum(dot_tiles(dY, Y, 0.0));      // sum_IJ KT[I][J] . Ga[J][I] = sum_IK dY(I, K) . Ga(I, K)
            out = ln == m ? dh : out;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            Y[q >> 1][q & 1] = hs * Y[q >> 1][q & 1];
            dY[q >> 1][q & 1] = hs * dY[q >> 1][q & 1];
        }
        v4d R[2][2] = {{kInvFact[kDeg] * IdB, zero}, {zero, kInvFact[kDeg] * IdB}};
        v4d dR[2][2] = {{zero, zero}, {zero, zero}};
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) vstep(Y, dY, R, dR, kInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            transpose4(scr, R, Y, g, j);           // E, dE in A layout; Y, dY are free from here on
            transpose4(scr, dR, dY, g, j);
            vstep(Y, dY, R, dR, zero);
        }
        // ZT = E^T dE, into Y
#pragma unroll
        for (int J = 0; J < 2; ++J) {
            v4d z0 = zero, z1 = zero;
#pragma unroll
            for (int K = 0; K < 2; ++K) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    z0 = __builtin_amdgcn_mfma_f64_16x16x4f64(R[K][0][kk], dR[K][J][kk], z0, 0, 0, 0);
                    z1 = __builtin_amdgcn_mfma_f64_16x16x4f64(R[K][1][kk], dR[K][J][kk], z1, 0, 0, 0);
                }
            }
            Y[0][J] = z0;
            Y[1][J] = z1;
        }
        const double* __restrict__ imgc = P.img;
        if constexpr (PAR) asm volatile("" : "+s"(imgc));
#pragma unroll 1
        for (int u = 0; u < m; ++u) {
            const double* __restrict__ Gu = imgc + (size_t)(1 + u) * 1024;
            double pu = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v4d t4 = load_image_tile(Gu + q * 256, lane);       // tile (J, I) = q against ZT[I][J]
#pragma unroll
                for (int r = 0; r < 4; ++r) pu = fma(Y[q & 1][q >> 1][r], t4[r], pu);
            }
            const double du = wave_sum(pu);
            if constexpr (PAR) duv = ln == u ? du : duv;
            else out = ln == u ? du * cl : out;
        }
        if constexpr (PAR) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) accl[64 * (4 * q + r) + lane] += Y[q >> 1][q & 1][r];
            accv = fma(av, duv, accv);
            out = ln < m ? duv * cl : out;
            if (ln < nde) *gp = out;
            gp -= nde;
        } else {
            if (ln < P.nd) gs[(s * P.n_int + t) * P.nd + lane] = out;
        }
        vapplyT(R, x);
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

void qc_sweep32_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, int64_t chunk, int64_t n_chunks,
                            double* gs, bool par, double* dgrad_theta, double* dgrad_scale, hipStream_t st) {
    const SweepParams P = qc_sweep_params(h, S, chunk, n_chunks);
    const unsigned grid = qc_sweep_grid(P, kWaves);
    if (par) {
        hipLaunchKernelGGL(qc_sweep32_grad_kernel<true>, dim3(qc_sweep_grid(P, kGW<true>)), dim3(64 * kGW<true>), 0, st, P, dZ, dtheta, dscale, (const double*)h->dXs.p,
                           (const double*)h->dLs.p, gs, h->dPart.p);
        qc_sweep_launch_par_reduce(h, S, n_chunks, dgrad_theta, dgrad_scale, st);
    } else
        hipLaunchKernelGGL(qc_sweep32_grad_kernel<false>, dim3(grid), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale, (const double*)h->dXs.p,
                           (const double*)h->dLs.p, gs, (double*)nullptr);
}
