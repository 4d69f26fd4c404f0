// Sweep gradients: the adjoint of the rollout sweep of qc_sweep.hip.  For every sample s of
//     G_s(a) = G_drift + sum_j theta[s,j] P_j + sum_k c[s,k] a_k G_k,   x_{t+1} = E_t x_t,  E_t = exp(h_t G_s(a_t)),   F_s = phi(x_{T-1})
// the derivatives dF_s/da_{t,k} and dF_s/dh_t of every interval, and their weighted sum over the samples as a dense gradient over Z.
// With lambda_{T-1} = dphi/dx, lambda_t = E_t^T lambda_{t+1} and L(X; D) the Frechet derivative of exp at X in direction D,
//     dF_s/da_{t,k} = c[s,k] h <lambda_{t+1} x_t^T, L(hG; G_k)> = c[s,k] h <L(hG^T; lambda_{t+1} x_t^T), G_k>        (L(X; .)* = L(X^T; .)),
//     dF_s/dh_t     = <lambda_{t+1}, G x_{t+1}>:
// ONE Frechet chain per interval gives all m drive derivatives as inner products with the drive tiles.
//
// Scope: the "mfma16-sweep" form (2N <= 16, m <= 8), a unitary or ket fidelity, at most 16 state columns, and ANTISYMMETRIC drift,
// drives and perturbations (closed systems: every QuantumSystem).  Antisymmetry makes E orthogonal, which is used three times:
//   * x_t = E^T x_{t+1} reverses the forward step exactly, so no forward state is stored inside a chunk;
//   * E^T commutes with exp(s hG), so L(hG; E^T K) = E^T L(hG; K): with K = x_{t+1} lambda_{t+1}^T, known BEFORE the interval's
//     exponential, the chain in direction K runs beside the Horner chain of E itself and one product with E^T follows.  The order
//     problem (M_t needs x_t, which needs E) is gone: neither are the Horner / squaring intermediates kept, nor is the R chain computed twice;
//   * <lambda, G x> = -sum (lambda x^T)_ab G_ba, so the timestep derivative is an inner product of tiles already in registers.
// Everything else returns QC_ERR_UNSUPPORTED (Lindblad generators need stored forward states) -- unless the descriptor opts in with
// reserved1[0] = QC_SWEEP_STORED_STATES: such handles are routed to the stored-state walk of qc_sweep_open_grad.hip (wide handles that also
// set QC_SWEEP_WIDE_STORED: of qc_sweep32_open_grad.hip; "mfma64-sweep" handles that also set QC_SWEEP_WIDE_64_STORED: of qc_sweep64_open_grad.hip), whatever their generators, behind the same totals, seed (with lambda = g_r for the density fidelity) and reductions; qc_sweep_reverse_scope decides.
// Descriptors with QC_SWEEP_WIDE | QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD extend the closed scope to the "mfma64-sweep" form, 32 < 2N <= 64, with
// states of up to 32 columns: the seed at ld = 64 and the walk of qc_sweep64_grad.hip, the same reductions; parameter gradients there only for descriptors that also set QC_SWEEP_WIDE_64_PARAMS (the flavour <true> of that
// file's walk, then qc_sweep_par_reduce_kernel of this one).
// Wide descriptors (wide = QC_SWEEP_WIDE) extend the scope to the "mfma32-sweep" form, 2N <= 32: this file routes such handles to the
// seed and walk kernels of qc_sweep32_grad.hip and shares its reductions (launch 4) with them; parameter gradients there only for
// descriptors that also set QC_SWEEP_WIDE_PARAMS (the flavour <true> of that file's walk, then qc_sweep_par_reduce_kernel of this one).
//
// Launches of one call:
//   1. the forward chunk totals: qc_sweep_mfma16_kernel of qc_sweep.hip, unchanged, same chunk rule;
//   2. qc_sweep_seed_kernel (ld = 16; qc_sweep32_seed_kernel, ld = 32, on wide handles: one body, fid_seed<LD>, on the chains of
//      qc_sweep_seed.h), one workgroup per sample: chains the totals in ascending order exactly as qc_sweep_finish_kernel does (the
//      fidelities carry the bits of qc_sweep_eval), stores x at every chunk end, F_s, lambda_{T-1} = dphi/dx by the definitions of
//      qc_fidelity.hip (|t| / n: (t_r g_r + t_i g_i) / (n^2 F), not special-cased at t = 0, as there; |t|^2 forms: 2 (t_r g_r + t_i g_i) / n^2),
//      then chains the transposed totals back down and stores lambda at every chunk end;
//   3. qc_sweep_grad_kernel, one wavefront per (sample, chunk), walking the chunk BACKWARDS; every matrix one 16 x 16 tile in registers
//      (lane maps: qc_mfma_kernels.hip header; A layout: lane (g, i) reg kk = A[i][4kk+g]; B / D layout: lane (g, j) reg r = X[4r+g][j];
//      a D-layout tile read as the A operand acts as its transpose).  Per interval, with x, lambda the D-layout tiles of knot t+1:
//        x_A, lambda_A             one LDS round trip (two tiles transposed)
//        KT = lambda x^T           mma(lambda_A, x_A): D layout of K^T; read as an A operand it acts as K
//        dF/dh = -sum KT . Ga      elementwise with the generator's A-layout tile
//        Y = h G / 2^sq, ||Y||_1 <= 1/8, dY = (h / 2^sq) K          (threshold, degree 8 and 1/k! table of the forward kernel)
//        R_k = Y R_k+1 + I/(k-1)!,   dR_k = dY R_k+1 + Y dR_k+1      k = 8 .. 1     (12 MFMAs a step)
//        sq squarings  dE <- E dE + dE E,  E <- E E                  (12 MFMAs and one LDS round trip each: E^T, dE^T as A operands)
//        ZT = E^T dE                h L(hG; x_t lambda_{t+1}^T): read against an A-layout tile it is its own transpose
//        dF/da_k = c_k sum ZT . G_k   m wave reductions in a fixed order (DPP row sums, then four row values)
//        x <- E^T x,  lambda <- E^T lambda                            (E in D layout IS the A operand E^T: no transpose)
//      and the m + 1 values of the interval leave through one vector store (lane k: drive k, lane m: timestep).
//      MFMAs per interval: 4 + 8 x 12 + 12 sq + 4 + 4 + 4 = 112 + 12 sq, against the forward kernel's 40 + 4 sq (2.8x - 3x).
//   4. qc_sweep_grad_reduce_kernel / qc_sweep_J_kernel: grad = sum_s w_s dF_s in ascending s, one thread per entry of Z (every entry that is
//      not a control or timestep of knots 0 .. T-2 is written as +0.0); J = sum_s w_s F_s by a fixed tree.  No atomics anywhere: repeated
//      calls give the same bits.
//
// Parameter gradients (qc_sweep_grad_params*): the derivatives with respect to the sample's own parameters,
//     dF_s/dtheta[s,j] = sum_t sum(ZT_t . P_j),     dF_s/dc[s,k] = sum_t a_{t,k} sum(ZT_t . G_k)      (du_{t,k} before the factor c_k),
// from the flavour <M, true> of the walk: Acc = sum_t ZT_t over the chunk (contracted with the perturbation tiles once, at the chunk's
// end) and lane k's sum_t a_{t,k} du_{t,k}, both kept in the wave's LDS slice; the chunk's shares go to scratch S x n_chunks x (p + m)
// and qc_sweep_par_reduce_kernel adds them in ascending chunk order.  The flavour <M, false> is the walk qc_sweep_grad_dev launches,
// instruction for instruction what it was before the second flavour existed.
//
// Truncation of the once-differentiated series: the degree-8 polynomial's derivative misses sum_{k>=9} k ||Y||^(k-1) / k! ||dY||
// <= 1.15 (1/8)^8 / 8! ||dY|| = 1.7e-12 ||dY||; over the 2^sq factors of the squarings the directions add up to h ||c_k G_k||, so the
// relative error of a drive derivative is 1.7e-12, three orders inside the tests' 1e-9.  The degree stays 8.
//
// Pullbacks (qc_sweep_vjp.hip): the same walks behind a seed that takes lambda_{T-1} from the caller; qc_sweep16_launch_walk below is the
// launch of this file's walk for both, qc_sweep_closed_scope what the two scopes share.
//
// gfx950 cross-compile: see the table in DESIGN.md ("Sweep gradients"); no private segment, no spills in any instantiation.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "qc_mfma_common.h"
#include "qc_sweep16_common.h"
#include "qc_sweep_internal.h"
#include "qc_sweep_seed.h"

namespace {

using namespace qc_sweep16;         // the series, the generator, the squaring rule, the step and the wave sum
using qc_sweep_seed::kSeedT;        // threads of the seed workgroup
constexpr int kRedT = 256;

struct SeedParams {
    int n, ns, n_chunks, fid_kind, fid_form, fid_n;
};

struct ReduceParams {
    int zdim, off_a, off_dt, m, nd;
    long long T, Zlen, S;
};

// One wavefront per (sample, chunk), walking the chunk backwards.  PAR = false: the per-interval derivatives only (`part` unused).
// PAR = true, the parameter flavour, also accumulates the chunk's shares of dF_s/dtheta_j = sum_t sum(ZT_t . P_j) and
// dF_s/dc_k = sum_t a_{t,k} sum(ZT_t . G_k) and stores them at the chunk's end as part[item][p + m]; `gs` may then be NULL (no
// per-interval store, no timestep derivative).
template <int M, bool PAR = false>
__global__ __launch_bounds__(64 * kWaves, 2) void qc_sweep_grad_kernel(const SweepParams P, const double* __restrict__ Z, const double* __restrict__ theta,
                                                                         const double* __restrict__ scale, const double* __restrict__ xs,
                                                                         const double* __restrict__ ls, double* __restrict__ gs,
                                                                         double* __restrict__ part) {
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

    // ---- once per wave: the sample's base tile, the drive tiles, the state and the adjoint at the chunk's end --------------------
    const v4d base = base_tile(P.img, m, P.p, theta, s, lane);
    v4d Gj[M];
    resident_tiles(P.img, m, lane, Gj);
    const int kl = lane < m ? lane : (m > 0 ? m - 1 : 0);
    const double cl = (scale && m > 0) ? scale[s * m + kl] : 1.0;

    v4d x, lam;
    {
        const int ns = P.n * P.nc;
        const double* __restrict__ xe = xs + item * ns;
        const double* __restrict__ le = ls + item * ns;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * r + g;
            const bool in = row < P.n && j < P.nc;
            x[r] = in ? xe[row + P.n * j] : 0.0;
            lam[r] = in ? le[row + P.n * j] : 0.0;
        }
    }

    const double hfix = opaque_scalar(P.dt_fixed);
    const double* __restrict__ z = Z + (long long)(t1 - 1) * P.zdim;
    double av = m > 0 ? z[P.off_a + kl] : 0.0;
    double h = ft ? z[P.off_dt] : hfix;
    // PAR: Acc = sum_t ZT_t (lane l, register r at accl[64 r + l]) and lane k's sum_t a_{t,k} du_{t,k} (accl[320 + l]; du BEFORE the
    // factor c_k: no division by c) live in the wave's LDS slice, and the interval's unscaled controls wait there (accl[256 + l]) for
    // the interval's end: every lane reads back what it wrote itself (no barrier), one read / write pair per interval off the MFMA
    // chain.  Held in registers they do not fit beside M = 6 at three waves per SIMD.
    double* accl = scr + 2 * kTile;
    if constexpr (PAR) {
#pragma unroll
        for (int r = 0; r < 4; ++r) accl[64 * r + lane] = 0.0;
        accl[320 + lane] = 0.0;
    }
#pragma unroll 1
    for (int t = t1 - 1; t >= t0; --t) {
        // the previous interval's controls and timestep are requested before this interval's products
        const double* __restrict__ zn = Z + (long long)(t > t0 ? t - 1 : t) * P.zdim;
        const double av_n = m > 0 ? zn[P.off_a + kl] : 0.0;
        const double h_n = ft ? zn[P.off_dt] : hfix;
        const double al = av * cl;
        if constexpr (PAR) accl[256 + lane] = av;
        const v4d Ga = generator(base, Gj, m, al);
        const int sq = squarings(h, Ga);      // the rule of the forward kernel
        const double hs = h * ldexp(1.0, -sq);
        // K^T = lambda x^T of knot t+1 (D layout) from the A-layout forms of both
        v4d KT;
        {
            const v4d in[2] = {x, lam};
            v4d tr[2];
            lds_transpose16_multi<2>(scr, in, tr, g, j);
            KT = mma16(tr[1], tr[0], zero);
        }
        // M = 8: kept loop-invariant, the eight lane compares below live in 16 scalar registers and the kernel spills one; an opaque
        // copy of the lane index has them made per interval instead (8 v_cmp)
        int ln = lane;
        if constexpr (M >= 8 || (PAR && M >= 6)) asm volatile("" : "+v"(ln));
        double out = 0.0, duv = 0.0;      // duv (PAR): lane k holds du_k = sum ZT . G_k
        if (ft && (!PAR || gs)) {
            double ph = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) ph = fma(KT[r], Ga[r], ph);
            const double dh = -wave_sum(ph);
            out = ln == m ? dh : out;
        }
        const v4d Y = hs * Ga;
        const v4d dY = hs * KT;
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
        const v4d ZT = mma16(R, dR, zero);                       // E^T dE
#pragma unroll
        for (int u = 0; u < M; ++u) {
            if (u < m) {
                double pu = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) pu = fma(ZT[r], Gj[u][r], pu);
                const double du = wave_sum(pu);
                if constexpr (PAR) duv = ln == u ? du : duv;
                else out = ln == u ? du * cl : out;
            }
        }
        if constexpr (PAR) {
#pragma unroll
            for (int r = 0; r < 4; ++r) accl[64 * r + lane] += ZT[r];
            accl[320 + lane] = fma(accl[256 + lane], duv, accl[320 + lane]);       // lanes >= m: duv = 0
            out = ln < m ? duv * cl : out;
            if (gs && lane < P.nd) gs[(s * P.n_int + t) * P.nd + lane] = out;
        } else {
            if (lane < P.nd) gs[(s * P.n_int + t) * P.nd + lane] = out;
        }
        x = mma16(R, x, zero);
        lam = mma16(R, lam, zero);
        av = av_n;
        h = h_n;
    }
    if constexpr (PAR) {
        // the chunk's shares: one contraction of Acc per perturbation, the tiles read once here
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

// grad_theta[s][j] / grad_scale[s][k] = the chunk shares of sample s added in ascending chunk order; one thread per (s, parameter)
__global__ __launch_bounds__(kRedT) void qc_sweep_par_reduce_kernel(long long S, int n_chunks, int p, int m, const double* __restrict__ part,
                                                                    double* __restrict__ gth, double* __restrict__ gsc) {
    const int np = p + m;
    const long long i = (long long)blockIdx.x * kRedT + threadIdx.x;
    if (i >= S * np) return;
    const long long s = i / np;
    const int q = (int)(i - s * np);
    const double* __restrict__ src = part + s * n_chunks * np + q;
    double acc = 0.0;
    for (int c = 0; c < n_chunks; ++c) acc += src[(long long)c * np];
    if (q < p) { if (gth) gth[s * p + q] = acc; }
    else if (gsc) gsc[s * m + (q - p)] = acc;
}

// The body of both seed kernels, one workgroup per sample; LD is the leading dimension of the totals.  Up (qc_sweep_seed.h): x at every
// chunk end; F_s and lambda = dphi/dx at the final state; down: lambda at every chunk end.
template <int LD>
__device__ __forceinline__ void fid_seed(const SeedParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                         const double* __restrict__ gr, const double* __restrict__ gi, double* __restrict__ xs,
                                         double* __restrict__ ls, double* __restrict__ fids, double* sm) {
    __shared__ double red[2][kSeedT / 64];
    __shared__ double coef[3];
    const int tid = threadIdx.x, ns = F.ns;
    const long long s = blockIdx.x;
    qc_sweep_seed::Lds L(sm, ns);
    const double* __restrict__ Qs = tot + s * F.n_chunks * (long long)(LD * LD);
    double* __restrict__ lo = ls + s * F.n_chunks * (long long)ns;
    qc_sweep_seed::chain_up<LD>(L, F.n, ns, F.n_chunks, Qs, src, xs + s * F.n_chunks * (long long)ns);
    double* cur = L.cur;
    double ar = 0.0, ai = 0.0;
    for (int i = tid; i < ns; i += kSeedT) {
        const double xi = cur[i];
        ar = fma(gr[i], xi, ar);
        ai = fma(gi[i], xi, ai);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ar += __shfl_xor(ar, off, 64);
        ai += __shfl_xor(ai, off, 64);
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = ar; red[1][tid >> 6] = ai; }
    __syncthreads();
    if (tid == 0) {
        const double tr = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        const double ti = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        const double nn = (double)F.fid_n;
        double Fv, fac;      // the mapping and the gradient factor of qc_fidelity_kernel (qc_fidelity.hip)
        if (F.fid_kind == QC_FID_UNITARY) {
            if (F.fid_form == QC_FID_FORM_ABS2) { Fv = (tr * tr + ti * ti) / (nn * nn); fac = 2.0 / (nn * nn); }
            else { Fv = sqrt(tr * tr + ti * ti) / nn; fac = 1.0 / (nn * nn * Fv); }
        } else { Fv = tr * tr + ti * ti; fac = 2.0; }
        double cr = tr, ci = ti;
        if (F.fid_kind == QC_FID_DENSITY) { Fv = tr; cr = 1.0; ci = 0.0; fac = 1.0; }      // F = Re t is linear: lambda = g_r as stored
        fids[s] = Fv;
        coef[0] = cr; coef[1] = ci; coef[2] = fac;
    }
    __syncthreads();
    const double tr = coef[0], ti = coef[1], fac = coef[2];
    for (int idx = tid; idx < ns; idx += kSeedT) {
        const double v = (tr * gr[idx] + ti * gi[idx]) * fac;
        cur[idx] = v;
        lo[(long long)(F.n_chunks - 1) * ns + idx] = v;
    }
    qc_sweep_seed::chain_down<LD>(L, F.n, ns, F.n_chunks, Qs, lo, nullptr);
}

__global__ __launch_bounds__(kSeedT) void qc_sweep_seed_kernel(const SeedParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                                               const double* __restrict__ gr, const double* __restrict__ gi,
                                                               double* __restrict__ xs, double* __restrict__ ls, double* __restrict__ fids) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    fid_seed<16>(F, tot, src, gr, gi, xs, ls, fids, sm);
}

__global__ __launch_bounds__(kSeedT) void qc_sweep64_seed_kernel(const SeedParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                                                 const double* __restrict__ gr, const double* __restrict__ gi,
                                                                 double* __restrict__ xs, double* __restrict__ ls, double* __restrict__ fids) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    fid_seed<64>(F, tot, src, gr, gi, xs, ls, fids, sm);
}

__global__ __launch_bounds__(kSeedT) void qc_sweep32_seed_kernel(const SeedParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                                                 const double* __restrict__ gr, const double* __restrict__ gi,
                                                                 double* __restrict__ xs, double* __restrict__ ls, double* __restrict__ fids) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    fid_seed<32>(F, tot, src, gr, gi, xs, ls, fids, sm);
}

// grad[i] = sum_s w_s dF_s/dZ_i in ascending s for the controls and timesteps of knots 0 .. T-2, +0.0 everywhere else
__global__ __launch_bounds__(kRedT) void qc_sweep_grad_reduce_kernel(const ReduceParams R, const double* __restrict__ gs, const double* __restrict__ w,
                                                                     double* __restrict__ grad) {
    const long long i = (long long)blockIdx.x * kRedT + threadIdx.x;
    if (i >= R.Zlen) return;
    const long long t = i / R.zdim;
    const int o = (int)(i - t * R.zdim);
    int k = -1;
    if (t < R.T - 1) {
        if (o >= R.off_a && o < R.off_a + R.m) k = o - R.off_a;
        else if (o == R.off_dt) k = R.m;       // off_dt = -1: never
    }
    double acc = 0.0;
    if (k >= 0) {
        const long long stride = (R.T - 1) * R.nd;
        const double* __restrict__ p = gs + t * R.nd + k;
        const double w1 = 1.0 / (double)R.S;
        for (long long s = 0; s < R.S; ++s) acc = fma(w ? w[s] : w1, p[s * stride], acc);
    }
    grad[i] = acc;
}

// J = sum_s w_s F_s: thread i sums s = i, i + 256, ... in ascending order, then a fixed tree over the 256 partial sums
__global__ __launch_bounds__(kRedT) void qc_sweep_J_kernel(long long S, const double* __restrict__ fids, const double* __restrict__ w, double* __restrict__ J) {
    __shared__ double part[kRedT];
    const int tid = threadIdx.x;
    const double w1 = 1.0 / (double)S;
    double acc = 0.0;
    for (long long s = tid; s < S; s += kRedT) acc = fma(w ? w[s] : w1, fids[s], acc);
    part[tid] = acc;
    __syncthreads();
    for (int off = kRedT / 2; off > 0; off >>= 1) {
        if (tid < off) part[tid] += part[tid + off];
        __syncthreads();
    }
    if (tid == 0) *J = part[0];
}

}  // namespace

// The tolerance of the antisymmetry test: max |G + G^T| <= 64 eps max |G| per matrix.  iso generators of exactly Hermitian operators are
// exactly antisymmetric; 64 eps admits operators that were symmetrised or scaled in floating point, and stays ten orders below any
// dissipator worth the name.
// What the gradient and the pullback (qc_sweep_vjp.hip) ask of a descriptor alike: an MFMA form, antisymmetric matrices, at most 16 state columns.
bool qc_sweep_closed_scope(const qc_sweep_desc* d, std::string* why) {
    const int n = 2 * d->N;
    if (!qc_sweep_desc_is_mfma(d)) { *why = qc_sweep_per_sample_why(d); return false; }
    const bool form64 = qc_sweep_desc_form(d) == QC_SWEEP_FORM_64;      // served only with QC_SWEEP_WIDE_64_GRAD (qc_sweep64_grad.hip)
    if (form64 && !(d->wide & QC_SWEEP_WIDE_64_GRAD)) { *why = qc_sweep_form64_why(d); return false; }
    const double* sets[3] = {d->G_drift, d->G_drives, d->G_pert};
    const int counts[3] = {1, d->m, d->n_pert};
    const char* names[3] = {"G_drift", "drive generator", "perturbation generator"};
    for (int q = 0; q < 3; ++q)
        for (int k = 0; k < counts[q]; ++k) {
            const double* G = sets[q] + (size_t)k * n * n;
            double big = 0.0, asym = 0.0;
            for (int c = 0; c < n; ++c)
                for (int r = 0; r < n; ++r) {
                    big = fmax(big, fabs(G[(size_t)c * n + r]));
                    asym = fmax(asym, fabs(G[(size_t)c * n + r] + G[(size_t)r * n + c]));
                }
            if (!(asym <= 64.0 * 2.220446049250313e-16 * big)) {
                *why = std::string(names[q]) + (q ? " " + std::to_string(k) : std::string()) +
                       " is not antisymmetric (open-system generators are not served: their gradients need stored forward states)";
                return false;
            }
        }
    const int nc = d->state_cols == 0 ? d->N : d->state_cols;
    if (form64) {      // x and lambda are 4 x 2 tiles there: a full unitary of N <= 32 fits
        if (nc > 32) { *why = "states of more than 32 columns are not served in the mfma64-sweep form (2N = " + std::to_string(n) + ", state_cols = " + std::to_string(nc) + ")"; return false; }
        return true;
    }
    if (nc > 16) { *why = "states of more than 16 columns are not served (state_cols = " + std::to_string(nc) + ")"; return false; }
    return true;
}

// Reverse mode of a descriptor: reserved1[0] chooses the walk.  0: the closed walk and its scope above.  QC_SWEEP_STORED_STATES: the
// stored-state walk of qc_sweep_open_grad.hip, which asks nothing of the generators: the "mfma16-sweep" form, at most 16 state columns;
// the "mfma32-sweep" form only for descriptors that opt in with QC_SWEEP_WIDE_STORED (the 2 x 2-tile walk of qc_sweep32_open_grad.hip);
// the "mfma64-sweep" form only for descriptors that opt in with QC_SWEEP_WIDE_64_STORED (the 4 x 4-tile walk of qc_sweep64_open_grad.hip, at
// most 32 state columns).
bool qc_sweep_reverse_scope(const qc_sweep_desc* d, std::string* why) {
    if (d->reserved1[0] != QC_SWEEP_STORED_STATES) return qc_sweep_closed_scope(d, why);
    const qc_sweep_form form = qc_sweep_desc_form(d);
    if (form == QC_SWEEP_FORM_PER_SAMPLE) { *why = qc_sweep_per_sample_why(d); return false; }
    if (form == QC_SWEEP_FORM_64) {      // only with QC_SWEEP_WIDE_64_STORED (which needs QC_SWEEP_WIDE_64_GRAD): the 4 x 4-tile walk of qc_sweep64_open_grad.hip
        if (!(d->wide & QC_SWEEP_WIDE_64_STORED)) { *why = qc_sweep_form64_unserved(d, "stored-state gradients"); return false; }
        const int nc64 = d->state_cols == 0 ? d->N : d->state_cols;
        if (nc64 > 32) { *why = "states of more than 32 columns are not served in the mfma64-sweep form (2N = " + std::to_string(2 * d->N) + ", state_cols = " + std::to_string(nc64) + ")"; return false; }
        return true;
    }
    if (form == QC_SWEEP_FORM_32 && !(d->wide & QC_SWEEP_WIDE_STORED)) { *why = "stored-state gradients are not served in the mfma32-sweep form"; return false; }
    const int nc = d->state_cols == 0 ? d->N : d->state_cols;
    if (nc > 16) { *why = "states of more than 16 columns are not served (state_cols = " + std::to_string(nc) + ")"; return false; }
    return true;
}

// the gradient's scope whatever reserved1[0] says: what the noise gradient (qc_sweep_noise.hip) keeps asking
bool qc_sweep_closed_grad_scope(const qc_sweep_desc* d, std::string* why) {
    if (!qc_sweep_closed_scope(d, why)) return false;
    if (d->fid_kind == QC_SWEEP_FID_NONE) { *why = "the handle has no fidelity (QC_SWEEP_FID_NONE)"; return false; }
    if (d->fid_kind == QC_FID_DENSITY) { *why = "the density-operator fidelity is not served"; return false; }
    return true;
}

bool qc_sweep_grad_scope(const qc_sweep_desc* d, std::string* why) {
    if (d->reserved1[0] != QC_SWEEP_STORED_STATES) return qc_sweep_closed_grad_scope(d, why);
    if (!qc_sweep_reverse_scope(d, why)) return false;
    if (d->fid_kind == QC_SWEEP_FID_NONE) { *why = "the handle has no fidelity (QC_SWEEP_FID_NONE)"; return false; }
    return true;      // QC_FID_DENSITY included: its seed is lambda = g_r
}

extern "C" int qc_sweep_desc_grad_supported(const qc_sweep_desc* d, int32_t* supported) {
    int rc = qc_sweep_validate_desc(d);
    if (rc) return rc;
    if (!supported) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep_desc_grad_supported: supported is NULL");
    std::string why;
    const bool ok = qc_sweep_grad_scope(d, &why);
    *supported = ok ? 1 : 0;
    if (!ok) (void)qc_sweep_fail(nullptr, QC_ERR_UNSUPPORTED, "qc_sweep gradients: " + why);
    return QC_OK;
}

// The backward walk of "mfma16-sweep" handles, for the gradient above and the pullback of qc_sweep_vjp.hip: qc_sweep_grad_kernel<M, false>, or
// with `par` the flavour <M, true> (gs may then be NULL) followed by qc_sweep_par_reduce_kernel out of h->dPart.  x and lambda at the chunk
// ends are read from h->dXs / h->dLs; scratch is the caller's.
void qc_sweep16_launch_walk(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, int64_t chunk, int64_t n_chunks,
                            double* gs, bool want_par, double* dgrad_theta, double* dgrad_scale, hipStream_t st) {
    const SweepParams P = qc_sweep_params(h, S, chunk, n_chunks);
    const unsigned grid = qc_sweep_grid(P, kWaves);
#define QC_GRAD_LAUNCH(M_)                                                                                                                      \
    do {                                                                                                                                        \
        if (want_par)                                                                                                                           \
            hipLaunchKernelGGL((qc_sweep_grad_kernel<M_, true>), dim3(grid), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale,                    \
                               (const double*)h->dXs.p, (const double*)h->dLs.p, gs, h->dPart.p);                                               \
        else                                                                                                                                    \
            hipLaunchKernelGGL((qc_sweep_grad_kernel<M_, false>), dim3(grid), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale,                   \
                               (const double*)h->dXs.p, (const double*)h->dLs.p, gs, (double*)nullptr);                                         \
    } while (0)
    QC_SWEEP_FOR_M(P.m, QC_GRAD_LAUNCH);
#undef QC_GRAD_LAUNCH
    if (want_par) qc_sweep_launch_par_reduce(h, S, n_chunks, dgrad_theta, dgrad_scale, st);
}

// grad_theta / grad_scale out of the chunk shares in h->dPart (qc_sweep_par_reduce_kernel), for the walk above and the stored-state walk
void qc_sweep_launch_par_reduce(qc_sweep* h, int64_t S, int64_t n_chunks, double* dgrad_theta, double* dgrad_scale, hipStream_t st) {
    const int m = h->d.m, p = h->d.n_pert;
    hipLaunchKernelGGL(qc_sweep_par_reduce_kernel, dim3((unsigned)((S * (p + m) + kRedT - 1) / kRedT)), dim3(kRedT), 0, st, (long long)S,
                       (int)n_chunks, p, m, (const double*)h->dPart.p, dgrad_theta, dgrad_scale);
}

// Launch 2 (the fidelity's seed) and launch 4 (the weighted reductions) of a gradient call, for the entry points below and the noise sweep
// of qc_sweep_noise.hip.  The seed reads the chunk totals of h->dTot and writes h->dXs / h->dLs (grown by the caller) and the S fidelities.
void qc_sweep_launch_fid_seed(qc_sweep* h, int64_t S, int64_t n_chunks, const double* dinit, double* dfids, hipStream_t st) {
    SeedParams F;
    F.n = h->n; F.ns = h->ns; F.n_chunks = (int)n_chunks;
    F.fid_kind = h->d.fid_kind; F.fid_form = h->d.fid_form; F.fid_n = h->fid_n;
    // at most 16 state columns: 16 KiB; "mfma64-sweep": at most 32, 64 KiB and the kernel's static words, hence the opt-in
    const size_t lds = qc_sweep_seed::lds_bytes(h->ns, h->mfma64 ? 64 : h->mfma32 ? 32 : 16);
    const auto seed = h->mfma64 ? qc_sweep64_seed_kernel : h->mfma32 ? qc_sweep32_seed_kernel : qc_sweep_seed_kernel;
    if (h->mfma64)      // a refusal shows as the launch's error, which the caller reads
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&qc_sweep64_seed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(seed, dim3((unsigned)S), dim3(kSeedT), lds, st, F, (const double*)h->dTot.p, dinit, (const double*)h->dgr,
                       (const double*)h->dgi, h->dXs.p, h->dLs.p, dfids);
}

// dgrad = sum_s w_s gsamp[s] over Z (qc_sweep_grad_reduce_kernel) and dJ = sum_s w_s dfids[s] (qc_sweep_J_kernel); either may be NULL
void qc_sweep_launch_weighted(qc_sweep* h, int64_t S, const double* gsamp, const double* dweights, const double* dfids, double* dgrad, double* dJ,
                              hipStream_t st) {
    if (dgrad) {
        ReduceParams R;
        R.zdim = h->d.zdim; R.off_a = h->d.off_a; R.off_dt = h->d.off_dt; R.m = h->d.m; R.nd = h->d.m + (h->d.off_dt >= 0 ? 1 : 0);
        R.T = h->d.T; R.Zlen = h->Zlen; R.S = S;
        hipLaunchKernelGGL(qc_sweep_grad_reduce_kernel, dim3((unsigned)((h->Zlen + kRedT - 1) / kRedT)), dim3(kRedT), 0, st, R, gsamp, dweights, dgrad);
    }
    if (dJ) hipLaunchKernelGGL(qc_sweep_J_kernel, dim3(1), dim3(kRedT), 0, st, (long long)S, dfids, dweights, dJ);
}

// "mfma32-sweep" handles made without QC_SWEEP_WIDE_PARAMS, in scope or not: the refusal of both parameter entry points
static const char* const kNoWideParGrad = "qc_sweep gradients: parameter gradients are not served in the mfma32-sweep form";
// "mfma64-sweep" handles made with QC_SWEEP_WIDE_64_GRAD but without QC_SWEEP_WIDE_64_PARAMS (without the former the gradient's own scope
// refuses, as before)
static int no_par_grad64(qc_sweep* h) {
    return qc_sweep_fail(h, QC_ERR_UNSUPPORTED, "qc_sweep gradients: parameter gradients are not served in the mfma64-sweep form (2N = " + std::to_string(h->n) + ")");
}

// the argument checks of all four entry points, in the order of the header
static int grad_check(qc_sweep* h, const char* who, const double* Z, const double* init, int64_t S, const double* theta, bool any_out, bool g_theta,
                      bool g_scale) {
    int rc = qc_sweep_check(h, who, &qc_sweep::grad_ok, "qc_sweep gradients: ", &qc_sweep::grad_why, Z, init, nullptr, S, theta);
    if (rc) return rc;
    const std::string pre = std::string(who) + ": ";
    if (!any_out) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "every output is NULL");
    if (g_theta && h->d.n_pert == 0) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "grad_theta is given but the handle has no perturbations (n_pert = 0)");
    if (g_scale && h->d.m == 0) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "grad_scale is given but the handle has no drives (m = 0)");
    return QC_OK;
}

// Both device entry points.  Without dgrad_theta / dgrad_scale this is qc_sweep_grad_dev as it always was: the same launches of the same
// kernels.  With either, the walk is the parameter flavour, which also serves the per-interval outputs when they are asked for.
static int qc_sweep_grad_launch(qc_sweep* h, const char* who, const double* dZ, const double* dinit, int64_t S, const double* dtheta,
                                const double* dscale, const double* dweights, double* dfids, double* dJ, double* dgrad, double* dgrad_samples,
                                double* dgrad_theta, double* dgrad_scale, void* stream) {
    int rc = grad_check(h, who, dZ, dinit, S, dtheta, dfids || dJ || dgrad || dgrad_samples || dgrad_theta || dgrad_scale, dgrad_theta != nullptr,
                        dgrad_scale != nullptr);
    if (rc) return rc;
    std::string& slot = *qc_sweep_err_slot();
    qc_device_guard guard(h->device);
    QC_SIDE_HIP(h, slot, guard.err);
    hipStream_t st = (hipStream_t)stream;
    const int m = h->d.m, p = h->d.n_pert;
    const int nd = m + (h->d.off_dt >= 0 ? 1 : 0);
    const int64_t n_int = h->d.T - 1;
    int64_t chunk, n_chunks;
    rc = qc_sweep_launch_totals(h, dZ, S, dtheta, dscale, st, &chunk, &n_chunks);
    if (rc) return rc;
    const size_t n_state = (size_t)S * n_chunks * h->ns;
    QC_SIDE_HIP(h, slot, h->grow(h->dXs, n_state));
    QC_SIDE_HIP(h, slot, h->grow(h->dLs, n_state));
    if (!dfids) {
        QC_SIDE_HIP(h, slot, h->grow(h->dGfid, (size_t)S));
        dfids = h->dGfid.p;
    }
    const bool want_par = dgrad_theta || dgrad_scale;
    const bool want_grad = (dgrad || dgrad_samples) && nd > 0;
    double* gsamp = dgrad_samples;
    if (want_grad && !gsamp) {
        QC_SIDE_HIP(h, slot, h->grow(h->dGsamp, (size_t)S * n_int * nd));
        gsamp = h->dGsamp.p;
    }
    if (want_par) QC_SIDE_HIP(h, slot, h->grow(h->dPart, (size_t)S * n_chunks * (p + m)));
    if (h->stored && (want_grad || want_par)) QC_SIDE_HIP(h, slot, h->grow(h->dXall, (size_t)S * (size_t)n_int * h->ns));
    qc_sweep_launch_fid_seed(h, S, n_chunks, dinit, dfids, st);
    if (h->mfma64 && h->stored && h->wide64_stored) {      // the 4 x 4-tile stored-state walk (qc_sweep64_open_grad.hip), whatever the generators
        if ((want_grad || want_par) &&      // want_par: only on handles with QC_SWEEP_WIDE_64_PARAMS (the entry points refuse the others)
            (rc = qc_sweep64_open_launch_walk(h, dZ, dinit, S, dtheta, dscale, chunk, n_chunks, want_grad ? gsamp : nullptr, want_par, h->dPart.p, st)))
            return rc;
        if (want_par) qc_sweep_launch_par_reduce(h, S, n_chunks, dgrad_theta, dgrad_scale, st);
    } else if (h->mfma64 && h->wide64_grad) {      // the 4 x 4-tile form: its own walk (qc_sweep64_grad.hip), then the reductions below
        if ((want_grad || want_par) &&      // want_par: only on handles with QC_SWEEP_WIDE_64_PARAMS (the entry points refuse the others)
            (rc = qc_sweep64_launch_walk(h, dZ, S, dtheta, dscale, chunk, n_chunks, want_grad ? gsamp : nullptr, want_par, h->dPart.p, st)))
            return rc;
        if (want_par) qc_sweep_launch_par_reduce(h, S, n_chunks, dgrad_theta, dgrad_scale, st);
    } else if (h->stored) {      // reserved1[0] = QC_SWEEP_STORED_STATES: the walk of qc_sweep_open_grad.hip, whatever the generators
        if (want_grad || want_par)      // (an "mfma32-sweep" handle is in scope only with QC_SWEEP_WIDE_STORED: the 2 x 2-tile walk)
            (h->mfma32 ? qc_sweep32_open_launch_walk : qc_sweep_open_launch_walk)(h, dZ, dinit, S, dtheta, dscale, chunk, n_chunks,
                                                                                 want_grad ? gsamp : nullptr, want_par, dgrad_theta, dgrad_scale, st);
    } else if (h->mfma32) {      // the 2 x 2-tile form: its own walk (qc_sweep32_grad.hip), then the reductions below
        if (want_grad || want_par)      // want_par: only on handles with QC_SWEEP_WIDE_PARAMS (the entry points refuse the others)
            qc_sweep32_launch_walk(h, dZ, S, dtheta, dscale, chunk, n_chunks, want_grad ? gsamp : nullptr, want_par, dgrad_theta, dgrad_scale, st);
    } else if (want_grad || want_par)
        qc_sweep16_launch_walk(h, dZ, S, dtheta, dscale, chunk, n_chunks, want_grad ? gsamp : nullptr, want_par, dgrad_theta, dgrad_scale, st);
    qc_sweep_launch_weighted(h, S, gsamp, dweights, dfids, dgrad, dJ, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qc_sweep_fail(h, QC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return QC_OK;
}

extern "C" int qc_sweep_grad_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                                 const double* dweights, double* dfids, double* dJ, double* dgrad, double* dgrad_samples, void* stream) {
    return qc_sweep_grad_launch(h, "qc_sweep_grad_dev", dZ, dinit, S, dtheta, dscale, dweights, dfids, dJ, dgrad, dgrad_samples, nullptr, nullptr,
                                stream);
}

extern "C" int qc_sweep_grad_params_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                                        const double* dweights, double* dfids, double* dJ, double* dgrad, double* dgrad_samples,
                                        double* dgrad_theta, double* dgrad_scale, void* stream) {
    if (h && h->mfma32 && !h->wide_par) return qc_sweep_fail(h, QC_ERR_UNSUPPORTED, kNoWideParGrad);
    if (h && h->wide64_grad && !h->wide64_par) return no_par_grad64(h);
    return qc_sweep_grad_launch(h, "qc_sweep_grad_params_dev", dZ, dinit, S, dtheta, dscale, dweights, dfids, dJ, dgrad, dgrad_samples, dgrad_theta,
                                dgrad_scale, stream);
}

// Both host-buffer entry points: stage, launch on the handle's stream, copy back, synchronise.
static int qc_sweep_grad_host(qc_sweep* h, const char* who, const double* Z, const double* init, int64_t S, const double* theta, const double* scale,
                              const double* weights, double* fids, double* J, double* grad, double* grad_samples, double* grad_theta,
                              double* grad_scale) {
    int rc = grad_check(h, who, Z, init, S, theta, fids || J || grad || grad_samples || grad_theta || grad_scale, grad_theta != nullptr,
                        grad_scale != nullptr);
    if (rc) return rc;
    const size_t nS = (size_t)S, m = (size_t)h->d.m, p = (size_t)h->d.n_pert, Zlen = (size_t)h->Zlen;
    const size_t n_samp = nS * (size_t)(h->d.T - 1) * (m + (h->d.off_dt >= 0 ? 1 : 0));
    qc_stage stage(h, qc_sweep_err_slot());
    const double* dZ = stage.in(h->sZ, Z, Zlen);
    const double* dinit = stage.in(h->sInit, init, (size_t)h->ns);
    const double* dtheta = stage.in(h->sTheta, theta, nS * p);
    const double* dscale = stage.in(h->sScale, scale, nS * m);
    const double* dweights = stage.in(h->sW, weights, nS);
    double* dfids = stage.out(h->sFids, fids, nS);
    double* dJ = stage.out(h->sJ, J, 1);
    double* dgrad = stage.out(h->sGrad, grad, Zlen);
    double* dsamp = stage.out(h->sGradS, grad_samples, n_samp);
    double* dgth = stage.out(h->sGth, grad_theta, nS * p);
    double* dgsc = stage.out(h->sGsc, grad_scale, nS * m);
    if ((rc = stage.status())) return rc;
    if ((rc = qc_sweep_grad_launch(h, who, dZ, dinit, S, dtheta, dscale, dweights, dfids, dJ, dgrad, dsamp, dgth, dgsc, h->stream))) return rc;
    return stage.finish();
}

extern "C" int qc_sweep_grad(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale,
                             const double* weights, double* fids, double* J, double* grad, double* grad_samples) {
    return qc_sweep_grad_host(h, "qc_sweep_grad", Z, init, S, theta, scale, weights, fids, J, grad, grad_samples, nullptr, nullptr);
}

extern "C" int qc_sweep_grad_params(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale,
                                    const double* weights, double* fids, double* J, double* grad, double* grad_samples, double* grad_theta,
                                    double* grad_scale) {
    if (h && h->mfma32 && !h->wide_par) return qc_sweep_fail(h, QC_ERR_UNSUPPORTED, kNoWideParGrad);
    if (h && h->wide64_grad && !h->wide64_par) return no_par_grad64(h);
    return qc_sweep_grad_host(h, "qc_sweep_grad_params", Z, init, S, theta, scale, weights, fids, J, grad, grad_samples, grad_theta, grad_scale);
}
