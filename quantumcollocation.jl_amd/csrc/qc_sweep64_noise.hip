// Noise-trajectory sweeps for "mfma64-sweep" handles (32 < 2N <= 64) whose `wide` has QC_SWEEP_WIDE_64_NOISE: the two kernels of
// qc_sweep_noise.hip (read its header first: the model, the zero-noise contract, grad_noise; then qc_sweep32_noise.hip, how the wide form
// did it) with every matrix 4 x 4 tiles of 16 x 16 in LDS.  In interval t of sample s
//     G_{s,t} = G_drift + sum_j (theta[s,j] + xi[s,t,j]) P_j + sum_k c[s,k] a_{t,k} G_k.
// Nothing is resident per generator in this form: qc_sweep64::generator reads the images 1 .. m again every interval and the perturbation
// images follow the drives in the image buffer, so a per-interval perturbation is a longer loop bound, mt = m + p <= 24, and a per-lane
// coefficient source.  No tile limit: m <= 16, p <= QC_MAX_PERT.
//   * generator u < m is drive u, coefficient c[s,u] a_{t,u} (the product rounded as qc_sweep_mfma64_kernel's av * cl); generator m + j is
//     perturbation j, coefficient noise[(s (T-1) + t) p + j], factor 1.  Each lane that fetches a coefficient carries its own pointer and
//     stride (zdim or p) in vector registers and steps it per interval: one load per lane and interval, requested one interval ahead;
//   * base_elems folds theta; the drives are added in ascending k, THEN the perturbations in ascending j.  At xi = +0.0 the extra fmas leave
//     every value as it was (a -0 may become +0, nothing else), so finals / fids / grad / grad_samples carry the bits of qc_sweep_eval and
//     qc_sweep_grad on the same handle;
//   * everything behind the generator is qc_sweep_mfma64_kernel's / qc_sweep64_grad_kernel's, restated here (to be changed with them:
//     those files are not touched, so their kernels compile to what they compiled to before this file existed): squarings(), the Horner
//     chain through tile_mul / chain<>, the squarings, W <- E W or the adjoint step.  The chunk totals go to h->dTot (S x n_chunks x 4096)
//     and qc_sweep_finish_kernel follows at ld = 64; the gradient runs the seed, the walk below and the weighted reduction unchanged.
//
// Forward kernel, qc_sweep64_noise_kernel: qc_sweep_mfma64_kernel with mt generators; lane l of every wave fetches generator
// min(l, mt - 1)'s coefficient and generator() broadcasts lane u's.  LDS, barriers and MFMAs ((9 + sq) x 256 an interval) are that kernel's.
//
// Backward kernel, qc_sweep64_noise_grad_kernel: the closed walk of qc_sweep64_grad_kernel with mt generators and the tail's image loop over
// all mt images.  It keeps no running sums and no chunk share: the wave sums of an interval leave in that interval.  LDS map of the
// dynamic part, work item and the MFMA count ((4352 + 1152 nct) + 768 sq an interval) are that kernel's; static LDS is red[16],
// part[16 x 25] and coef[2 x 32], 3 840 B, so 155 904 B of the CU's 160 KiB.
// The walk has no register to spare, the scalar ones least of all, so the interval's coefficients do not travel in a lane of every wave:
//   coef[2][32]   the row of one interval, double-buffered by interval parity: entry u < mt the coefficient of generator u, scaled; entry
//                 31 the timestep (free timesteps; a fixed one is the kernel argument).
// Lanes 0 .. 31 of wave 0 fill it.  Lane l keeps, in vector registers made once per item, the source pointer and stride of entry l, its
// factor, and the address and stride of the value it stores per interval:
//     lane u < m          Z[t, off_a + u], stride zdim, factor c[s,u];         stores drive u's derivative, times c[s,u], into gs[s,t,u]
//     lane m + j < mt     noise[s,t,j], stride p, factor 1;                     stores sum ZT . P_j into gn[s,t,j]
//     lane mt             (repeats lane mt - 1's source; entry mt is not read)  factor -1: stores the timestep's derivative into gs[s,t,m]
//     lane 31             Z[t, off_dt], stride zdim, factor 1 (free timesteps); stores nothing
// (other lanes repeat lane mt - 1's source into entries nobody reads).  A lane whose buffer is absent keeps a null address and stride 0:
// which buffers are present changes which lanes store, never what they hold.  Every thread's generator loop reads coef[b + u] (an LDS
// broadcast) where qc_sweep64::generator broadcasts a lane, and the timestep from coef[b + 31].
// The wave sums of the interval: lane u < mt of every wave keeps sum ZT . image u, lane mt the timestep's sum KT . G (skipped when gs is
// absent); part[w][0 .. mt] as in the parameter flavour, and wave 0 adds the 16 partials behind Ba in ascending wave order.
// Barriers of one interval: S, H0, U / P / W per Horner step and P / W per squaring, Ba -- those of qc_sweep64_grad.hip, with the same
// reasons for Y, R, dR, x, lambda, u, red[] and part[].  For coef[]:
//     F   before the loop: publishes the first interval's half of the row (and, as S would, the states written once per item);
//     the half b of interval t is read in front of S of interval t (generator and timestep; both are in registers behind S);
//     wave 0 writes the other half, the next interval's, just in front of Ba of interval t: its last readers read it in front of S of
//     the interval before, a whole interval of barriers ago, and Ba stands between this write and its first read;
//     half b is written next in front of Ba of the next interval, behind that interval's S, hence behind every read of it.
// No atomics, sums in a fixed order: repeated calls give the same bits.
// gfx950 cross-compile: see the table in DESIGN.md 5.8.15; no private segment, no spills in either kernel.
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_side.h"
#include "qc_sweep64_common.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep64;

constexpr int kCoefLd = 32;       // one half of the coefficient row; entry kHEntry is the timestep
constexpr int kHEntry = 31;
constexpr int kPartLd = 25;       // values a wave leaves per interval: mt + 1 <= 25
constexpr size_t kGradLdsBytes = (size_t)(3 * kMat + 3 * kThin) * sizeof(double);      // 152 064 B, as qc_sweep64_grad.hip

// Where lane l finds the coefficient of generator min(l, mt - 1) in interval t, how far the next interval's lies, and the sample's factor
// (p >= 1: there always is a generator).
struct LaneCoef {
    const double* cp;
    int stride;          // doubles from one interval to the next: zdim for a drive lane, p for a perturbation lane
    double cl;           // c[s,k] for a drive lane, 1 for a perturbation lane
};

__device__ __forceinline__ LaneCoef lane_coef(const SweepParams& P, int lane, long long s, int t, const double* __restrict__ Z,
                                              const double* __restrict__ scale, const double* __restrict__ noise) {
    const int m = P.m, mt = m + P.p;
    const int kl = lane < mt ? lane : mt - 1;
    const bool drv = kl < m;
    LaneCoef c;
    c.cp = drv ? Z + (long long)t * P.zdim + P.off_a + kl : noise + (s * P.n_int + t) * (long long)P.p + (kl - m);
    c.stride = drv ? P.zdim : P.p;
    c.cl = (scale && drv) ? scale[s * m + kl] : 1.0;
    return c;
}

// Launch 1: the chunk totals.  Restates qc_sweep_mfma64_kernel (qc_sweep64.hip; to be changed with it) with mt generators.
__global__ __launch_bounds__(kThreads, 1) void qc_sweep64_noise_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                         const double* __restrict__ theta, const double* __restrict__ scale,
                                                                         const double* __restrict__ noise, double* __restrict__ tot) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double red[16];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, j = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), I = w & 3, J = w >> 2;
    const long long item = blockIdx.x;
    const ChunkRange ch = chunk_range(item, P.n_chunks, P.chunk, P.n_int);
    const int t0 = ch.t0, t1 = ch.t1, m = P.m, mt = m + P.p;
    const long long s = ch.s;
    const bool ft = P.off_dt >= 0;

    // ---- once per item: the sample's base matrix, the lane's coefficient source, W = I ----------------------------------------------
    double base[4];
    base_elems(P.img, m, P.p, theta, s, tid, base);
    const LaneCoef lc = lane_coef(P, lane, s, t0, Z, scale, noise);
    const double* cp = lc.cp;
    int oY = 0, oW = 3 * kMat;      // the buffers' roles; Ra = kMat, Rb = 2 kMat
#pragma unroll
    for (int e = 0; e < 4; ++e) sm[oW + lds_at(tid, e)] = on_diagonal(tid, e) ? 1.0 : 0.0;

    const double* __restrict__ z = Z + (long long)t0 * P.zdim;
    double av = *cp;
    const double hfix = opaque_scalar(P.dt_fixed);      // keeps the two arms apart: no flat load (qc_mfma_common.h)
    double h = ft ? z[P.off_dt] : hfix;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        // the next interval's coefficients and timestep are requested before this interval's products
        const double* __restrict__ zn = Z + (long long)(t + 1 < t1 ? t + 1 : t) * P.zdim;
        if (t + 1 < t1) cp += lc.stride;
        const double av_n = *cp;
        const double h_n = ft ? zn[P.off_dt] : hfix;
        double G[4];
        generator(P.img, mt, av * lc.cl, base, tid, G);      // the drives in ascending k, then the perturbations in ascending j
        const int sq = squarings(red, G, h, lane, w);      // its barrier: every wave has left the previous interval's products
        const double hs = h * ldexp(1.0, -sq);
        // Horner: R_deg+1 = I/deg!,  R_k = Y R_k+1 + I/(k-1)!; the barrier rules of qc_sweep_mfma64_kernel (these writes rely on the barrier
        // inside squarings(); red[] has a workgroup barrier between a call of squarings() and the next)
        int oR = kMat, oN = 2 * kMat;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sm[oY + lds_at(tid, e)] = hs * G[e];
            sm[oR + lds_at(tid, e)] = on_diagonal(tid, e) ? kInvFact[kDeg] : 0.0;
        }
        __syncthreads();
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) {
            tile_mul(sm + oY, sm + oR, sm + oN, I, J, g, j, kInvFact[k - 1]);
            __syncthreads();
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

// Launch 3: the backward walk.  Restates qc_sweep64_grad_kernel (qc_sweep64_grad.hip; to be changed with it) with mt generators, the
// coefficient row and per-lane stores.  gs (S x (T-1) x nd) and gn (S x (T-1) x p) may each be NULL, not both.
__global__ __launch_bounds__(kThreads, 1) void qc_sweep64_noise_grad_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                              const double* __restrict__ theta, const double* __restrict__ scale,
                                                                              const double* __restrict__ noise, const double* __restrict__ xs,
                                                                              const double* __restrict__ ls, double* __restrict__ gs,
                                                                              double* __restrict__ gn) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double red[16];
    __shared__ double part[16 * kPartLd];
    __shared__ double coef[2 * kCoefLd];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, j = lane & 15;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), I = w & 3, J = w >> 2;
    const int Jc = J & 1;                   // the wave's column tile of a thin matrix
    const bool second = J >= 2;             // waves 8 .. 15: lambda's tiles; waves 0 .. 7: x's and u's
    const long long item = blockIdx.x;
    const ChunkRange ch = chunk_range(item, P.n_chunks, P.chunk, P.n_int);
    const int t0 = ch.t0, t1 = ch.t1, m = P.m, nc = P.nc;
    const int nct = nc > 16 ? 2 : 1;
    const long long s = ch.s;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};
    double* const Yb = sm;
    double* const Rb = sm + kMat;
    double* const dRb = sm + 2 * kMat;
    double* const Xb = sm + 3 * kMat;
    double* const Lb = Xb + kThin;
    double* const Ub = Lb + kThin;
    double* const mine = second ? Lb : Xb;      // the thin matrix whose tile (I, Jc) this wave carries through E^T

    // ---- once per item: the sample's base matrix, the state and the adjoint at the chunk's end (zero outside n x nc) -----------------
    double base[4];
    base_elems(P.img, m, P.p, theta, s, tid, base);
    {
        const int ns = P.n * nc;
        const double* __restrict__ xe = xs + item * ns;
        const double* __restrict__ le = ls + item * ns;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int idx = tid + 1024 * e, row = idx & 63, col = idx >> 6;
            const bool in = row < P.n && col < nc;
            Xb[col * kLd + row] = in ? xe[row + P.n * col] : 0.0;
            Lb[col * kLd + row] = in ? le[row + P.n * col] : 0.0;
        }
    }
    const int mt = m + P.p, n_val = mt + (ft ? 1 : 0);
    // ---- once per item: the lane's source, factor and destination (the table of the header); only wave 0's lanes < 32 use them ---------
    const double* cp;
    int cstr;
    double cl;
    double* op = nullptr;
    int ostr = 0;
    {
        const LaneCoef lc = lane_coef(P, lane, s, t1 - 1, Z, scale, noise);
        const bool hl = ft && lane == kHEntry;
        cp = hl ? Z + (long long)(t1 - 1) * P.zdim + P.off_dt : lc.cp;
        cstr = hl ? P.zdim : lc.stride;
        cl = (ft && lane == mt) ? -1.0 : lc.cl;      // lane mt repeats a perturbation's source (factor 1): the timestep's sign instead
        const long long it = s * P.n_int + (t1 - 1);
        if (gs && (lane < m || (ft && lane == mt))) {
            op = gs + it * P.nd + (lane < m ? lane : m);
            ostr = P.nd;
        } else if (gn && lane >= m && lane < mt) {
            op = gn + it * P.p + (lane - m);
            ostr = P.p;
        }
    }
    // what is per lane stays in vector registers (the scalar ones are the scarcer)
    asm volatile("" : "+v"(cp), "+v"(cstr), "+v"(cl), "+v"(op), "+v"(ostr));
    const bool filler = w == 0 && lane < kCoefLd;
    if (filler) coef[lane] = *cp * cl;      // the first interval's half: t1 - 1 takes half 0
    __syncthreads();      // F

    const gptr G0 = (gptr)(unsigned long long)P.img;
    const double hfix = opaque_scalar(P.dt_fixed);
    const bool want_dh = ft && gs;
    int b = 0;      // the half of coef[] this interval reads
#pragma unroll 1
    for (int t = t1 - 1; t >= t0; --t) {
        // the previous interval's coefficient is requested before this interval's products
        double av_n = 0.0;
        if (filler) {
            if (t > t0) cp -= cstr;
            av_n = *cp;
        }
        const double h = ft ? coef[b + kHEntry] : hfix;
        double G[4];
        {      // qc_sweep64::generator with the coefficients out of the row
            const gptr Gt = G0 + tid;
#pragma unroll
            for (int e = 0; e < 4; ++e) G[e] = base[e];
#pragma unroll 1
            for (int u = 0; u < mt; ++u) {
                const double a = coef[b + u];
                const gptr Gu = Gt + (size_t)(1 + u) * kImg;
#pragma unroll
                for (int e = 0; e < 4; ++e) G[e] = fma(a, Gu[1024 * e], G[e]);
            }
        }
        const int sq = squarings(red, G, h, lane, w);      // barrier S; the rule of the forward kernel: one function
        const double hs = h * ldexp(1.0, -sq);
        // lane u < mt: generator u's wave sum; lane mt: the timestep's (sum KT . G, its sign at the store)
        double out = 0.0;
        if (want_dh) {
            // sum_ab KT[a][b] G[b][a] over the thread's elements G[b = lane][a = w + 16 e], KT[a][b] = sum_c lambda[a][c] x[b][c]
            double kt[4] = {0.0, 0.0, 0.0, 0.0};
            for (int c = 0; c < nc; ++c) {
                const double xv = Xb[c * kLd + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) kt[e] = fma(Lb[c * kLd + w + 16 * e], xv, kt[e]);
            }
            double ph = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) ph = fma(kt[e], G[e], ph);
            const double dh = wave_sum(ph);
            out = lane == mt ? dh : out;
        }
        // Horner: R_deg+1 = I/deg!, dR_deg+1 = 0;  R_k = Y R_k+1 + I/(k-1)!,  dR_k = dY R_k+1 + Y dR_k+1
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Yb[lds_at(tid, e)] = hs * G[e];
            Rb[lds_at(tid, e)] = on_diagonal(tid, e) ? kInvFact[kDeg] : 0.0;
            dRb[lds_at(tid, e)] = 0.0;
        }
        __syncthreads();      // H0
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) {
            if (!second && Jc < nct) {
                const v4d u = chain<kColStep, kColStep, 16>(col_frag(Rb, I, g, j), col_frag(Lb, Jc, g, j), zero);
                store_tile(Ub, I, Jc, g, j, hs * u);
            }
            __syncthreads();      // U
            const v4d c0 = I == J ? kInvFact[k - 1] * IdB : zero;
            const v4d nR = chain<kRowStep, kColStep, 16>(row_frag(Yb, I, g, j), col_frag(Rb, J, g, j), c0);
            v4d nD = chain<kRowStep, kColStep, 16>(row_frag(Yb, I, g, j), col_frag(dRb, J, g, j), zero);
            nD = chain<kRowStep, kRowStep, 4>(row_frag(Xb, I, g, j), row_frag(Ub, J, g, j), nD);
            if (nct > 1) nD = chain<kRowStep, kRowStep, 4>(row_frag(Xb, I, g, j) + 16 * kLd, row_frag(Ub, J, g, j) + 16 * kLd, nD);
            __syncthreads();      // P
            store_tile(Rb, I, J, g, j, nR);
            store_tile(dRb, I, J, g, j, nD);
            __syncthreads();      // W
        }
#pragma unroll 1
        for (int q = 0; q < sq; ++q) {
            const v4d nE = chain<kRowStep, kColStep, 16>(row_frag(Rb, I, g, j), col_frag(Rb, J, g, j), zero);
            v4d nD = chain<kRowStep, kColStep, 16>(row_frag(Rb, I, g, j), col_frag(dRb, J, g, j), zero);
            nD = chain<kRowStep, kColStep, 16>(row_frag(dRb, I, g, j), col_frag(Rb, J, g, j), nD);
            __syncthreads();      // P
            store_tile(Rb, I, J, g, j, nE);
            store_tile(dRb, I, J, g, j, nD);
            __syncthreads();      // W
        }
        // ZT = E^T dE, the wave's tile of x or lambda through E^T, and the derivatives of every generator
        const v4d ZT = chain<kColStep, kColStep, 16>(col_frag(Rb, I, g, j), col_frag(dRb, J, g, j), zero);
        v4d nx = zero;
        if (Jc < nct) nx = chain<kColStep, kColStep, 16>(col_frag(Rb, I, g, j), col_frag(mine, Jc, g, j), zero);
        // the lane's elements ZT[a = 16 I + 4 r + g][b = 16 J + j] against G_u[b][a] (column-major images: a * 64 + b)
        const gptr Ge = G0 + (16 * I + g) * 64 + 16 * J + j;
#pragma unroll 1
        for (int u = 0; u < mt; ++u) {
            const gptr Gu = Ge + (size_t)(1 + u) * kImg;
            double pu = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) pu = fma(ZT[r], Gu[256 * r], pu);
            const double du = wave_sum(pu);
            out = lane == u ? du : out;
        }
        // an opaque copy of the lane index: the lane compares of the tail are made per interval instead of living in scalar register pairs
        // across the walk (as in qc_sweep64_grad_kernel<true>)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        if (ln < n_val) part[w * kPartLd + lane] = out;
        if (w == 0 && ln < kCoefLd) coef[(b ^ kCoefLd) + lane] = av_n * cl;      // the next interval's half (header: coef[])
        __syncthreads();      // Ba
        if (Jc < nct) store_tile(mine, I, Jc, g, j, nx);
        if (w == 0 && ln < n_val) {
            double acc = part[lane];
#pragma unroll
            for (int i = 1; i < 16; ++i) acc += part[i * kPartLd + lane];
            if (op) *op = acc * cl;      // drives: c[s,k]; perturbations: 1; the timestep: -1
        }
        op -= ostr;
        b ^= kCoefLd;
    }
}

}  // namespace

int qc_sweep64_noise_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dnoise,
                                   hipStream_t st, int64_t* chunk_out, int64_t* n_chunks_out) {
    SweepParams P;
    if (int rc = qc_sweep_plan_totals(h, S, h->dTot, kImg, &P, chunk_out, n_chunks_out)) return rc;
    // per launch, as qc_sweep64_launch_totals: the attribute belongs to the (function, device) pair
    QC_SIDE_HIP(h, *qc_sweep_err_slot(), hipFuncSetAttribute(reinterpret_cast<const void*>(&qc_sweep64_noise_kernel),
                                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
    hipLaunchKernelGGL(qc_sweep64_noise_kernel, dim3((unsigned)P.items), dim3(kThreads), kLdsBytes, st, P, dZ, dtheta, dscale, dnoise, h->dTot.p);
    QC_SIDE_HIP(h, *qc_sweep_err_slot(), hipGetLastError());
    return QC_OK;
}

int qc_sweep64_noise_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dnoise,
                                 int64_t chunk, int64_t n_chunks, double* gs, double* gn, hipStream_t st) {
    const SweepParams P = qc_sweep_params(h, S, chunk, n_chunks);
    QC_SIDE_HIP(h, *qc_sweep_err_slot(), hipFuncSetAttribute(reinterpret_cast<const void*>(&qc_sweep64_noise_grad_kernel),
                                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGradLdsBytes));
    hipLaunchKernelGGL(qc_sweep64_noise_grad_kernel, dim3((unsigned)P.items), dim3(kThreads), kGradLdsBytes, st, P, dZ, dtheta, dscale, dnoise,
                       (const double*)h->dXs.p, (const double*)h->dLs.p, gs, gn);
    QC_SIDE_HIP(h, *qc_sweep_err_slot(), hipGetLastError());
    return QC_OK;
}
