// Rollout sweeps for 32 < 2N <= 64 with up to 16 drives ("mfma64-sweep"): the forward sweep of qc_sweep.hip with every matrix 4 x 4
// tiles of 16 x 16 on v_mfma_f64_16x16x4_f64.  Taken only by descriptors with wide = QC_SWEEP_WIDE | QC_SWEEP_WIDE_64.  The
// mathematics is the family's (qc_sweep_common.h): Y = dt G_s(a_t) / 2^sq with ||Y||_1 <= 1/8 by squarings_of_norm on the largest
// column sum of |dt G|, the degree-kDeg Horner chain with the correctly rounded 1/k! table, sq squarings, W <- E_t W.  Sizes 34 .. 62 are
// zero-padded to 64: the exponential of the padded generator is the exponential of the true one plus an identity block.
//
// Work item.  A matrix is 128 VGPRs per lane, so base, Y, R and W do not fit in one wave's registers: the work item is one WORKGROUP
// of 16 waves per (sample, chunk of consecutive intervals) with the matrices in LDS, column-major with 66-double columns
// (qc_sweep64_common.h; the fragment reads of qc_mfma64_kernels.hip).  Four matrices, 135 168 B of the CU's 160 KiB, one workgroup per CU:
//     Y | Ra | Rb | W        Horner and the squarings alternate between Ra and Rb; W <- E W is written into the buffer Y has left,
//                            and the two exchange their roles for the next interval.
// Wave w owns output tile (w & 3, w >> 2) of every product: one chain of 16 MFMAs over ascending k, operands read from LDS as the chain
// advances, one workgroup barrier per product (the product reads two buffers and writes a third).  MFMAs per interval:
// (kDeg + sq + 1) x 256.  The sample's base matrix G_drift + sum theta P_j is formed once per item and stays in registers, four elements
// a thread; all threads assemble G_s(a_t) from the zero-padded column-major images (32 KiB a matrix, L2-resident) with the sample's
// `scale` folded into the amplitudes.  The number of drives is a loop bound; nothing is resident per drive, hence the limit of 16
// (lane u of a wave carries drive u's amplitude).  No atomics, no order that depends on scheduling: repeated calls give the same bits.
// The chunk total leaves as a full 64 x 64 column-major matrix (S x n_chunks x 4096 doubles of handle scratch);
// qc_sweep_finish_kernel (qc_sweep.hip) chains the totals with ld = 64.
//
// Noise-trajectory sweeps (handles that set QC_SWEEP_WIDE_64_NOISE; qc_sweep_noise.hip has the model and the zero-noise contract) are the
// flavour <true> of the same kernel: in interval t of sample s
//     G_{s,t} = G_drift + sum_j (theta[s,j] + xi[s,t,j]) P_j + sum_k c[s,k] a_{t,k} G_k.
// Nothing is resident per generator and the perturbation images follow the drives in the image buffer, so a per-interval perturbation is a
// longer loop bound, mt = m + p <= 24, and another coefficient source per lane (qc_sweep64_common.h: drive_lane for <false>, lane_coef for
// <true>, behind `if constexpr`; one load per lane and interval, requested one interval ahead).  Generator u < m is drive u, coefficient
// c[s,u] a_{t,u}, the product rounded as <false> rounds av * cl; generator m + j is perturbation j, coefficient noise[(s (T-1) + t) p + j],
// factor 1.  base_elems folds theta; the drives are added in ascending k, THEN the perturbations in ascending j.  At xi = +0.0 the extra
// fmas leave every value as it was (a -0 may become +0, nothing else) and everything behind the generator is the same code, so finals / fids
// of qc_sweep_noise_eval carry the bits of qc_sweep_eval on the same handle.
//
// Gradients and pullbacks of closed systems in this form: qc_sweep64_grad.hip, on handles that also set QC_SWEEP_WIDE_64_GRAD (without it
// their entry points answer QC_ERR_UNSUPPORTED, as they did); their parameter outputs with QC_SWEEP_WIDE_64_PARAMS as well.  Pushforwards in
// this form: qc_sweep64_jvp.hip, on handles that set QC_SWEEP_WIDE_64_TANGENT (any generators); the noise sweeps' gradient walk:
// qc_sweep64_noise.hip.  Out of scope in this form: Hessian products (their entry points answer QC_ERR_UNSUPPORTED on such a handle), a
// state-action form that skips the propagator for kets, more than 16 drives, 2N > 64.
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_side.h"
#include "qc_sweep64_common.h"
#include "qc_sweep64_launch.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep64;

// NOISE = false: the m drives, lane l of every wave fetching drive min(l, m - 1)'s control out of the knot (drive_lane; `noise` unused).
// NOISE = true, the noise sweeps: the mt = m + p generators, lane l fetching generator min(l, mt - 1)'s coefficient through its own pointer
// and stride (lane_coef), stepped per interval.  Either way generator() broadcasts lane u's; everything behind it is written once.
template <bool NOISE>
__global__ __launch_bounds__(kThreads, 1) void qc_sweep_mfma64_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                        const double* __restrict__ theta, const double* __restrict__ scale,
                                                                        const double* __restrict__ noise, double* __restrict__ tot) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double red[16];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, j = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), I = w & 3, J = w >> 2;
    const long long item = blockIdx.x;
    const ChunkRange ch = chunk_range(item, P.n_chunks, P.chunk, P.n_int);
    const int t0 = ch.t0, t1 = ch.t1, m = P.m, mt = NOISE ? m + P.p : m;
    const long long s = ch.s;
    const bool ft = P.off_dt >= 0;

    // ---- once per item: the sample's base matrix, the lane's coefficient source, W = I -----------------------------------------------
    double base[4];
    base_elems(P.img, m, P.p, theta, s, tid, base);
    int kl = 0, cstride = 0;      // <false>: the lane's drive; <true>: its pointer's step
    const double* cp = nullptr;
    double cl, av;
    if constexpr (NOISE) {
        const LaneCoef lc = lane_coef(P, lane, s, t0, Z, scale, noise);
        cp = lc.cp, cstride = lc.stride, cl = lc.cl;
    } else {
        const DriveLane d = drive_lane(scale, m, s, lane);
        kl = d.kl, cl = d.cl;
    }
    int oY = 0, oW = 3 * kMat;      // the buffers' roles; Ra = kMat, Rb = 2 kMat
#pragma unroll
    for (int e = 0; e < 4; ++e) sm[oW + lds_at(tid, e)] = on_diagonal(tid, e) ? 1.0 : 0.0;

    const double* __restrict__ z = Z + (long long)t0 * P.zdim;
    if constexpr (NOISE) av = *cp;
    else av = drive_value(z, P.off_a, m, kl);
    const double hfix = opaque_scalar(P.dt_fixed);      // keeps the two arms apart: no flat load (qc_mfma_common.h)
    double h = ft ? z[P.off_dt] : hfix;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        // the next interval's coefficients and timestep are requested before this interval's products
        const double* __restrict__ zn = Z + (long long)(t + 1 < t1 ? t + 1 : t) * P.zdim;
        double av_n;
        if constexpr (NOISE) {
            if (t + 1 < t1) cp += cstride;
            av_n = *cp;
        } else {
            av_n = drive_value(zn, P.off_a, m, kl);
        }
        const double h_n = ft ? zn[P.off_dt] : hfix;
        double G[4];
        generator(P.img, mt, av * cl, base, tid, G);      // the drives in ascending k, then (<true>) the perturbations in ascending j
        const int sq = squarings(red, G, h, lane, w);      // barrier S: every wave has left the previous interval's products
        const double hs = h * ldexp(1.0, -sq);
        // Horner: R_deg+1 = I/deg!,  R_k = Y R_k+1 + I/(k-1)!   (the last coefficient is exactly 1: a zero generator gives the identity bits)
        int oR = kMat, oN = 2 * kMat;
        // These writes rely on S: it orders them behind the previous interval's last product, which read E (in Ra or Rb) and the buffer
        // that is Y now (the only product without a barrier of its own behind it).  The barrier below and the product barriers are the
        // further barriers that red[] needs between two calls of squarings() (qc_sweep64_common.h).
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sm[oY + lds_at(tid, e)] = hs * G[e];
            sm[oR + lds_at(tid, e)] = on_diagonal(tid, e) ? kInvFact[kDeg] : 0.0;
        }
        __syncthreads();
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) {
            tile_mul(sm + oY, sm + oR, sm + oN, I, J, g, j, kInvFact[k - 1]);
            __syncthreads();      // a product reads two buffers and writes a third: one barrier per product
            const int o = oR; oR = oN; oN = o;
        }
#pragma unroll 1
        for (int q = 0; q < sq; ++q) {
            tile_mul(sm + oR, sm + oR, sm + oN, I, J, g, j, 0.0);
            __syncthreads();
            const int o = oR; oR = oN; oN = o;
        }
        tile_mul(sm + oR, sm + oW, sm + oY, I, J, g, j, 0.0);      // W <- E W into the buffer Y has left
        const int o = oY; oY = oW; oW = o;
        av = av_n;
        h = h_n;
    }
    __syncthreads();
    // column-major 64 x 64, a whole column per wave and request
    double* __restrict__ o = tot + item * kImg + tid;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[1024 * e] = sm[oW + lds_at(tid, e)];
}

}  // namespace

// the zero-padded column-major 64 x 64 image of one n x n column-major matrix
void qc_sweep64_image(const double* G, int n, double* img) {
    for (int c = 0; c < 64; ++c)
        for (int r = 0; r < 64; ++r) img[(size_t)c * 64 + r] = (r < n && c < n) ? G[(size_t)c * n + r] : 0.0;
}

int qc_sweep64_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, hipStream_t st, int64_t* chunk_out,
                             int64_t* n_chunks_out) {
    SweepParams P;
    if (int rc = qc_sweep_plan_totals(h, S, h->dTot, kImg, &P, chunk_out, n_chunks_out)) return rc;
    QC_SWEEP64_LAUNCH(h, qc_sweep_mfma64_kernel<false>, kLdsBytes, P, st, dZ, dtheta, dscale, (const double*)nullptr, h->dTot.p);
    return QC_OK;
}

int qc_sweep64_noise_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dnoise,
                                   hipStream_t st, int64_t* chunk_out, int64_t* n_chunks_out) {
    SweepParams P;
    if (int rc = qc_sweep_plan_totals(h, S, h->dTot, kImg, &P, chunk_out, n_chunks_out)) return rc;
    QC_SWEEP64_LAUNCH(h, qc_sweep_mfma64_kernel<true>, kLdsBytes, P, st, dZ, dtheta, dscale, dnoise, h->dTot.p);
    return QC_OK;
}
