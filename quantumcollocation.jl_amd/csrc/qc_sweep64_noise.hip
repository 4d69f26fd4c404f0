// The gradient walk of the noise-trajectory sweeps for "mfma64-sweep" handles (32 < 2N <= 64) whose `wide` has QC_SWEEP_WIDE_64_NOISE
// and QC_SWEEP_WIDE_64_GRAD: qc_sweep_noise_grad_kernel (qc_sweep_noise.hip; read its header first: the model, the zero-noise contract,
// grad_noise; then qc_sweep32_noise.hip, how the wide form did it) with every matrix 4 x 4 tiles of 16 x 16 in LDS.  The forward launch
// is the flavour <true> of qc_sweep_mfma64_kernel (qc_sweep64.hip: the generators of an interval, their order, the zero-noise bits); the
// gradient runs it, the seed, the walk below and the weighted reduction.
//
// qc_sweep64_noise_grad_kernel is the closed walk of qc_sweep64_grad_kernel with mt = m + p generators and the tail's image loop over all
// mt images.  The two walks are built on the same pieces of qc_sweep64_common.h -- the LDS map (walk_lds), load_state, generator_of,
// squarings, kt_dot, exp_pair (every barrier between S and Ba, with its reason), part_sum -- and differ in where a coefficient comes from
// and where a wave sum goes.  This one keeps no running sums and no chunk share: the wave sums of an interval leave in that interval.
// Work item and the MFMA count ((4352 + 1152 nct) + 768 sq an interval) are that kernel's; static LDS is red[16], part[16 x 25] and
// coef[2 x 32], 3 840 B, so 155 904 B of the CU's 160 KiB.  At xi = +0.0 fids / J / grad / grad_samples carry the bits of qc_sweep_grad.
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
// broadcast: generator_of with the row as its source) where generator() broadcasts a lane, and the timestep from coef[b + 31].
// The wave sums of the interval: lane u < mt of every wave keeps sum ZT . image u, lane mt the timestep's sum KT . G (skipped when gs is
// absent); part[w][0 .. mt] as in the parameter flavour, and wave 0 adds the 16 partials behind Ba in ascending wave order.
// Barriers of one interval: S (squarings), H0, U / P / W per Horner step and P / W per squaring (exp_pair), Ba (qc_sweep64_grad.hip), with
// the reasons given there for Y, R, dR, x, lambda, u, red[] and part[].  For coef[]:
//     F   before the loop: publishes the first interval's half of the row (and, as S would, the states written once per item);
//     the half b of interval t is read in front of S of interval t (generator and timestep; both are in registers behind S);
//     wave 0 writes the other half, the next interval's, just in front of Ba of interval t: its last readers read it in front of S of
//     the interval before, a whole interval of barriers ago, and Ba stands between this write and its first read;
//     half b is written next in front of Ba of the next interval, behind that interval's S, hence behind every read of it.
// No atomics, sums in a fixed order: repeated calls give the same bits.
// gfx950 cross-compile: see the table in DESIGN.md 5.8.16; no private segment, no spills.
#include <math.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_side.h"
#include "qc_sweep64_common.h"
#include "qc_sweep64_launch.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep64;

constexpr int kCoefLd = 32;       // one half of the coefficient row; entry kHEntry is the timestep
constexpr int kHEntry = 31;
constexpr int kPartLd = 25;       // values a wave leaves per interval: mt + 1 <= 25

// Launch 3: the backward walk.  gs (S x (T-1) x nd) and gn (S x (T-1) x p) may each be NULL, not both.
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
    load_state(xs + item * (P.n * nc), P.n, nc, tid, lds.X);
    load_state(ls + item * (P.n * nc), P.n, nc, tid, lds.L);
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
        generator_of(P.img, mt, [&](int u) { return coef[b + u]; }, base, tid, G);      // the row's entries where generator() broadcasts a lane
        const int sq = squarings(red, G, h, lane, w);      // barrier S; the rule of the forward kernel: one function
        const double hs = h * ldexp(1.0, -sq);
        // lane u < mt: generator u's wave sum; lane mt: the timestep's (sum KT . G, its sign at the store)
        double out = 0.0;
        if (want_dh) {
            const double dh = kt_dot(lds.X, lds.L, nc, G, lane, w);
            out = lane == mt ? dh : out;
        }
        exp_pair(lds, G, hs, sq, nct, tid, I, J, g, j);      // barriers H0, U / P / W per Horner step, P / W per squaring
        // ZT = E^T dE, the wave's tile of x or lambda through E^T, and the derivatives of every generator
        const v4d ZT = chain<kColStep, kColStep, 16>(col_frag(lds.R, I, g, j), col_frag(lds.dR, J, g, j), zero);
        v4d nx = zero;
        if (Jc < nct) nx = chain<kColStep, kColStep, 16>(col_frag(lds.R, I, g, j), col_frag(mine, Jc, g, j), zero);
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
            const double acc = part_sum<kPartLd>(part, lane);
            if (op) *op = acc * cl;      // drives: c[s,k]; perturbations: 1; the timestep: -1
        }
        op -= ostr;
        b ^= kCoefLd;
    }
}

}  // namespace

int qc_sweep64_noise_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dnoise,
                                 int64_t chunk, int64_t n_chunks, double* gs, double* gn, hipStream_t st) {
    const SweepParams P = qc_sweep_params(h, S, chunk, n_chunks);
    QC_SWEEP64_LAUNCH(h, qc_sweep64_noise_grad_kernel, kWalkLdsBytes, P, st, dZ, dtheta, dscale, dnoise, (const double*)h->dXs.p,
                      (const double*)h->dLs.p, gs, gn);
    return QC_OK;
}
