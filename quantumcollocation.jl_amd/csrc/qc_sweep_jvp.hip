// Sweep pushforwards: the tangent of the map (Z, init, theta, c) -> x_final[s] of the rollout sweep along ONE direction
// (vZ, vinit, vtheta, vc) -- the forward-mode counterpart of qc_sweep_vjp.hip.  With G_s(a) = G_drift + sum_j theta[s,j] P_j +
// sum_k c[s,k] a_k G_k and x_{t+1} = E_t x_t, E_t = exp(h_t G_s(a_t)), x_0 = init:
//     d(hG)_t = vh_t G_s(a_t) + h_t ( sum_j vtheta[s,j] P_j + sum_k ( vc[s,k] a_{t,k} + c[s,k] va_{t,k} ) G_k )
//     xdot_0 = vinit,    xdot_{t+1} = E_t xdot_t + L(h_t G; d(hG)_t) x_t          (L: the Frechet derivative of exp)
//     tfinals[s] = xdot_{T-1},    tfids[s] = <dF/dx(x_final[s]), xdot_{T-1}>.
// Nothing is reversed, so no antisymmetry is asked for: Lindblad generators are served like any others (the adjoint walks of
// qc_sweep_grad.hip are not: they reverse the state with E^T).
//
// "mfma16-sweep" handles (2N <= 16, up to 8 drives); "mfma32-sweep" handles made with QC_SWEEP_WIDE_TANGENT take qc_sweep32_jvp.hip for the
// chunk totals and share the finish kernel and the entry points below.  qc_sweep_jvp_kernel<M> has the work item, workgroup shape and chunk rule of
// qc_sweep_mfma16_kernel (qc_sweep.hip; read its header first): one wavefront per (sample, chunk), kWaves of them per workgroup,
// never synchronised.  Every product of the forward kernel is differentiated next to itself, with the tangent tile in the lane map
// of the tile it belongs to:
//   once per wave   Bdot = sum_j vtheta[s,j] P_j (A layout), the lane's vc[s,k] beside c[s,k]
//   coefficients    al = a c,  aldot = va c + a vc
//   generators      Ga = base + sum al_u G_u,  Gadot = Bdot + sum aldot_u G_u
//   squarings       sq from ||h Ga||_1 by the forward kernel's rule; the tangent never influences it (a non-finite direction cannot
//                   change what the other outputs see)
//   scaled tiles    Y = (h 2^-sq) Ga,  Ydot = (vh 2^-sq) Ga + (h 2^-sq) Gadot
//   Horner          Rdot <- Ydot R + Y Rdot (from the old R), R <- Y R + I/(k-1)!           8 x 12 MFMAs on three independent chains
//   per squaring    Rdot <- E Rdot + Edot E, R <- E E         (E, Edot as left factors: two LDS transposes in one round trip)  12 MFMAs
//   totals          Wdot <- E Wdot + Edot W, W <- E W                                                                             12 MFMAs
// 108 + 12 sq MFMAs per interval against the forward 36 + 4 sq.  The R / W chain is the forward kernel's operation for operation
// (same expressions for Ga, sq, Y, the same table, the same product order; an MFMA is an exact ascending-k fma chain), so W carries
// the forward kernel's bits.  The once-differentiated degree-8 series at ||Y||_1 <= 1/8 truncates at 1.7e-12 relative.
// The wave stores W and Wdot: S x n_chunks x 2 tiles of handle scratch.
//
// qc_sweep_jvp_finish_kernel, one workgroup per sample, has the loops and the reduction order of qc_sweep_finish_kernel:
// x <- init, xdot <- vinit; for ascending chunks xdot <- Q_c xdot + Qdot_c x, then x <- Q_c x; finals / fids carry the bits of
// qc_sweep_eval on the same handle.  A NULL direction is read as zeros through the same arithmetic: NULL and an explicit zero array
// give the same bits.  No atomics, sums in a fixed order: repeated calls return the same bits, and no output's bits depend on which
// others were asked for.  The totals are ld x ld, ld = 16 ("mfma32-sweep": 32, as qc_sweep_finish_kernel), the loops the same.  Its
// dynamic LDS is 4 ns + 2 ld^2 doubles (x, its successor, their tangents, one chunk total and its tangent);
// ns = 2N x state_cols reaches 4096 entries (qc_sweep_validate_desc), which is 135168 bytes = 132 KiB of the 160 KiB of a CU (ld = 32:
// 144 KiB).  Above 64 KiB the launch opts in with hipFuncSetAttribute; an MI355X accepts it up to ns = 4096
// (tests/test_sweep_many_columns.py, tests/test_sweep_wide_jvp.py).  Should the runtime refuse the attribute on a wide handle, Q and Qdot
// pass through one ld^2 slot one after the other (136 KiB): the sums keep their order and so their bits; a refusal of that is an error
// return.  "mfma64-sweep" handles made with QC_SWEEP_WIDE_64_TANGENT take qc_sweep64_jvp.hip for the chunk totals and the ld = 64
// instantiation qc_sweep64_jvp_finish_kernel: 4 ns + 8192 doubles, which bounds their scope at ns = 2048 (128 KiB; every full unitary of
// the form, N = 32 with 32 columns included); two slots only there, and a refused attribute is an error return.
//
// gfx950 cross-compile: see the table in DESIGN.md ("Sweep pushforwards"); no private segment, no spills in any instantiation.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "qc_mfma_common.h"
#include "qc_sweep16_common.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep16;

constexpr int kFinT = 256;          // threads of the finish workgroup, as qc_sweep_finish_kernel's
constexpr int kJvpNs64 = 2048;      // "mfma64-sweep": the largest state (2N x state_cols) the finish kernel at ld = 64 holds beside two totals

struct JvpFinParams {
    int n, ns, n_chunks, fid_kind, fid_form, fid_n;
    int one_slot;                // ld = 32 only: Q and Qdot pass through one slot of ld x ld doubles, one after the other (the same sums, the same bits)
};

template <int M>
__global__ __launch_bounds__(64 * kWaves, 2) void qc_sweep_jvp_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                        const double* __restrict__ theta, const double* __restrict__ scale,
                                                                        const double* __restrict__ vZ, const double* __restrict__ vtheta,
                                                                        const double* __restrict__ vscale, double* __restrict__ tot) {
    __shared__ double scr_all[kWaves * 2 * kTile];
    const WaveItem w = wave_item(kWaves);
    double* __restrict__ scr = scr_all + w.wq * (2 * kTile);
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m;
    const bool ft = P.off_dt >= 0;
    const bool hasv = vZ != nullptr;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    // ---- once per wave: the sample's base tile, its tangent, and the drive tiles -------------------------------------------
    v4d base, based;
    base_tile(P.img, m, P.p, theta, vtheta, s, lane, base, based);
    v4d Gj[M];
    resident_tiles(P.img, m, lane, Gj);
    // lane l holds the sample's factor of drive min(l, m-1) and its tangent
    const int kl = lane < m ? lane : (m > 0 ? m - 1 : 0);
    const double cl = (scale && m > 0) ? scale[s * m + kl] : 1.0;
    const double vcl = (vscale && m > 0) ? vscale[s * m + kl] : 0.0;

    const double* __restrict__ z = Z + (long long)t0 * P.zdim;
    double av = m > 0 ? z[P.off_a + kl] : 0.0;
    const double hfix = opaque_scalar(P.dt_fixed);
    double h = ft ? z[P.off_dt] : hfix;
    double vav = 0.0, vh = 0.0;
    if (hasv) {
        const double* __restrict__ vz = vZ + (long long)t0 * P.zdim;
        if (m > 0) vav = vz[P.off_a + kl];
        if (ft) vh = vz[P.off_dt];
    }
    v4d W = IdB, Wd = zero;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        // the next interval's controls, timestep and their tangents are requested before this interval's products
        const long long tn = t + 1 < t1 ? t + 1 : t;
        const double* __restrict__ zn = Z + tn * P.zdim;
        const double av_n = m > 0 ? zn[P.off_a + kl] : 0.0;
        const double h_n = ft ? zn[P.off_dt] : hfix;
        double vav_n = 0.0, vh_n = 0.0;
        if (hasv) {
            const double* __restrict__ vzn = vZ + tn * P.zdim;
            if (m > 0) vav_n = vzn[P.off_a + kl];
            if (ft) vh_n = vzn[P.off_dt];
        }
        const double al = av * cl;
        const double ald = fma(vav, cl, av * vcl);
        v4d Ga, Gad;
        generator(base, based, Gj, m, al, ald, Ga, Gad);
        const int sq = squarings(h, Ga);      // the forward kernel's rule: the tangent has no say in sq
        const double sc = ldexp(1.0, -sq);
        const v4d Y = (h * sc) * Ga;
        v4d Yd;
        {
            const double hs = h * sc, vhs = vh * sc;
#pragma unroll
            for (int r = 0; r < 4; ++r) Yd[r] = fma(vhs, Ga[r], hs * Gad[r]);
        }
        // Horner on the pair: Rdot_k = Ydot R_k+1 + Y Rdot_k+1,  R_k = Y R_k+1 + I/(k-1)!
        v4d R = kInvFact[kDeg] * IdB, Rd = zero;
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k) step16(Y, Yd, R, Rd, kInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            const v4d in[2] = {R, Rd};
            v4d tr[2];
            lds_transpose16_multi<2>(scr, in, tr, g, j);      // E^T, Edot^T in D layout = E, Edot in A layout
            step16(tr[0], tr[1], R, Rd, zero);
        }
        const v4d in[2] = {R, Rd};
        v4d tr[2];
        lds_transpose16_multi<2>(scr, in, tr, g, j);
        step16(tr[0], tr[1], W, Wd, zero);
        av = av_n;
        h = h_n;
        vav = vav_n;
        vh = vh_n;
    }
    double* __restrict__ o = tot + item * 512;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        o[j * 16 + 4 * r + g] = W[r];
        o[256 + j * 16 + 4 * r + g] = Wd[r];
    }
}

// One workgroup per sample: x = Q_last ... Q_0 init and its tangent in ascending order, final state, fidelity and their tangents.
// The x loop, the fidelity sums and their mapping are qc_sweep_finish_kernel's (ld = 16), so finals / fids carry its bits.
// With t = (g_r . x) + i (g_i . x) and tdot likewise from xdot:  dF = (t_r tdot_r + t_i tdot_i) / (n^2 F) for |t| / n (not special-cased
// at t = 0), 2 (t_r tdot_r + t_i tdot_i) / n^2 for |t|^2 / n^2, 2 (...) for a ket, tdot_r for a density operator (qc_fidelity.hip).
// The totals are ld x ld, l2 = ld^2 doubles each: 16 for "mfma16-sweep" handles, 32 for "mfma32-sweep" ones (the two kernels below).
template <int ld, int l2>
__device__ __forceinline__ void jvp_finish(const JvpFinParams& F, const double* __restrict__ tot, const double* __restrict__ src,
                                           const double* __restrict__ vsrc, const double* __restrict__ gr, const double* __restrict__ gi,
                                           double* __restrict__ finals, double* __restrict__ fids, double* __restrict__ tfinals,
                                           double* __restrict__ tfids) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double red[4][kFinT / 64];
    const int tid = threadIdx.x, n = F.n, ns = F.ns;
    const long long s = blockIdx.x;
    double* cur = sm;
    double* nxt = sm + ns;
    double* dcur = sm + 2 * ns;
    double* dnxt = sm + 3 * ns;
    double* Q = sm + 4 * ns;
    double* Qd = Q + l2;
    for (int idx = tid; idx < ns; idx += kFinT) {
        cur[idx] = src[idx];
        dcur[idx] = vsrc ? vsrc[idx] : 0.0;
    }
    const double* __restrict__ Qs = tot + s * F.n_chunks * (long long)(2 * l2);
    for (int c = 0; c < F.n_chunks; ++c) {
        if (ld == 32 && F.one_slot) {
            // Q, then Qdot in its place: dnxt keeps the tangent's sum between the two passes, every chain in the order of the loop below
            __syncthreads();
            for (int idx = tid; idx < l2; idx += kFinT) Q[idx] = Qs[(long long)c * (2 * l2) + idx];
            __syncthreads();
            for (int idx = tid; idx < ns; idx += kFinT) {
                const int r = idx % n, col = idx / n;
                double acc = 0.0, dacc = 0.0;
                for (int q = 0; q < n; ++q) acc = fma(Q[r + ld * q], cur[q + n * col], acc);
                for (int q = 0; q < n; ++q) dacc = fma(Q[r + ld * q], dcur[q + n * col], dacc);
                nxt[idx] = acc;
                dnxt[idx] = dacc;
            }
            __syncthreads();
            for (int idx = tid; idx < l2; idx += kFinT) Q[idx] = Qs[(long long)c * (2 * l2) + l2 + idx];
            __syncthreads();
            for (int idx = tid; idx < ns; idx += kFinT) {
                const int r = idx % n, col = idx / n;
                double dacc = dnxt[idx];
                for (int q = 0; q < n; ++q) dacc = fma(Q[r + ld * q], cur[q + n * col], dacc);
                dnxt[idx] = dacc;
            }
            double* tmp = cur; cur = nxt; nxt = tmp;
            tmp = dcur; dcur = dnxt; dnxt = tmp;
            continue;
        }
        __syncthreads();
        for (int idx = tid; idx < 2 * l2; idx += kFinT) Q[idx] = Qs[(long long)c * (2 * l2) + idx];
        __syncthreads();
        for (int idx = tid; idx < ns; idx += kFinT) {
            const int r = idx % n, col = idx / n;
            double acc = 0.0, dacc = 0.0;
            for (int q = 0; q < n; ++q) acc = fma(Q[r + ld * q], cur[q + n * col], acc);
            for (int q = 0; q < n; ++q) dacc = fma(Q[r + ld * q], dcur[q + n * col], dacc);
            for (int q = 0; q < n; ++q) dacc = fma(Qd[r + ld * q], cur[q + n * col], dacc);
            nxt[idx] = acc;
            dnxt[idx] = dacc;
        }
        double* tmp = cur; cur = nxt; nxt = tmp;
        tmp = dcur; dcur = dnxt; dnxt = tmp;
    }
    __syncthreads();
    if (finals)
        for (int idx = tid; idx < ns; idx += kFinT) finals[s * ns + idx] = cur[idx];
    if (tfinals)
        for (int idx = tid; idx < ns; idx += kFinT) tfinals[s * ns + idx] = dcur[idx];
    if (!fids && !tfids) return;
    double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
    for (int i = tid; i < ns; i += kFinT) {
        const double xi = cur[i], di = dcur[i];
        ar = fma(gr[i], xi, ar);
        ai = fma(gi[i], xi, ai);
        br = fma(gr[i], di, br);
        bi = fma(gi[i], di, bi);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ar += __shfl_xor(ar, off, 64);
        ai += __shfl_xor(ai, off, 64);
        br += __shfl_xor(br, off, 64);
        bi += __shfl_xor(bi, off, 64);
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = ar; red[1][tid >> 6] = ai; red[2][tid >> 6] = br; red[3][tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        const double tr = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        const double ti = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        const double dr = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
        const double di = (red[3][0] + red[3][1]) + (red[3][2] + red[3][3]);
        const double nn = (double)F.fid_n;
        double Fv;      // the mapping of qc_sweep_finish_kernel, written out again
        if (F.fid_kind == QC_FID_UNITARY) Fv = F.fid_form == QC_FID_FORM_ABS2 ? (tr * tr + ti * ti) / (nn * nn) : sqrt(tr * tr + ti * ti) / nn;
        else if (F.fid_kind == QC_FID_KET) Fv = tr * tr + ti * ti;
        else Fv = tr;
        if (fids) fids[s] = Fv;
        if (tfids) {
            const double dot = tr * dr + ti * di;
            double dF;
            if (F.fid_kind == QC_FID_UNITARY) dF = F.fid_form == QC_FID_FORM_ABS2 ? 2.0 * dot / (nn * nn) : dot / (nn * nn * Fv);
            else if (F.fid_kind == QC_FID_KET) dF = 2.0 * dot;
            else dF = dr;
            tfids[s] = dF;
        }
    }
}

__global__ __launch_bounds__(kFinT) void qc_sweep_jvp_finish_kernel(const JvpFinParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                                                    const double* __restrict__ vsrc, const double* __restrict__ gr,
                                                                    const double* __restrict__ gi, double* __restrict__ finals,
                                                                    double* __restrict__ fids, double* __restrict__ tfinals,
                                                                    double* __restrict__ tfids) {
    constexpr int ld = 16, l2 = 256;
    jvp_finish<ld, l2>(F, tot, src, vsrc, gr, gi, finals, fids, tfinals, tfids);
}

// the same on the 32 x 32 totals of "mfma32-sweep" handles (qc_sweep32_jvp.hip), as qc_sweep_finish_kernel takes ld = 32 for them
__global__ __launch_bounds__(kFinT) void qc_sweep32_jvp_finish_kernel(const JvpFinParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                                                      const double* __restrict__ vsrc, const double* __restrict__ gr,
                                                                      const double* __restrict__ gi, double* __restrict__ finals,
                                                                      double* __restrict__ fids, double* __restrict__ tfinals,
                                                                      double* __restrict__ tfids) {
    constexpr int ld = 32, l2 = 1024;
    jvp_finish<ld, l2>(F, tot, src, vsrc, gr, gi, finals, fids, tfinals, tfids);
}

// the same on the 64 x 64 totals of "mfma64-sweep" handles (qc_sweep64_jvp.hip), as qc_sweep_finish_kernel takes ld = 64 for them: the
// two-slot path only (the one-slot branch is compiled out: ld != 32), 4 ns + 8192 doubles, 128 KiB at the scope's ns = 2048
__global__ __launch_bounds__(kFinT) void qc_sweep64_jvp_finish_kernel(const JvpFinParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                                                      const double* __restrict__ vsrc, const double* __restrict__ gr,
                                                                      const double* __restrict__ gi, double* __restrict__ finals,
                                                                      double* __restrict__ fids, double* __restrict__ tfinals,
                                                                      double* __restrict__ tfids) {
    constexpr int ld = 64, l2 = 4096;
    jvp_finish<ld, l2>(F, tot, src, vsrc, gr, gi, finals, fids, tfinals, tfids);
}

// the argument checks both entry points share, in the order of the header's table
int jvp_check(qc_sweep* h, const char* who, const void* Z, const void* init, int64_t S, const void* theta, bool any_dir, bool any_out, bool v_theta,
              bool v_scale, bool any_fid) {
    int rc = qc_sweep_check(h, who, &qc_sweep::jvp_ok, "qc_sweep pushforward: ", &qc_sweep::jvp_why, Z, init, nullptr, S, theta);
    if (rc) return rc;
    const std::string pre = std::string(who) + ": ";
    if (!any_dir) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "every direction is NULL");
    if (!any_out) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "every output is NULL");
    if (v_theta && h->d.n_pert == 0) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "vtheta is given but the handle has no perturbations (n_pert = 0)");
    if (v_scale && h->d.m == 0) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "vscale is given but the handle has no drives (m = 0)");
    if (any_fid && h->d.fid_kind == QC_SWEEP_FID_NONE)
        return qc_sweep_fail(h, QC_ERR_INVALID, pre + "fidelities or their tangents requested from a handle created without one");
    return QC_OK;
}

}  // namespace

bool qc_sweep_jvp_scope(const qc_sweep_desc* d, std::string* why) {
    const qc_sweep_form form = qc_sweep_desc_form(d);
    if (form == QC_SWEEP_FORM_16) return true;
    if (form == QC_SWEEP_FORM_32) {
        if (d->wide & QC_SWEEP_WIDE_TANGENT) return true;      // qc_sweep32_jvp.hip
        *why = "pushforwards are not served in the mfma32-sweep form";
        return false;
    }
    if (form == QC_SWEEP_FORM_64 && (d->wide & QC_SWEEP_WIDE_64_TANGENT)) {      // qc_sweep64_jvp.hip
        // the finish kernel keeps x, its successor, their tangents and two 64 x 64 totals in LDS: (4 ns + 8192) doubles, 128 KiB at ns = 2048
        const int64_t ns = 2 * (int64_t)d->N * (d->state_cols == 0 ? d->N : d->state_cols);
        if (ns <= kJvpNs64) return true;
        *why = "the handle takes the mfma64-sweep form (2N = " + std::to_string(2 * d->N) + "), which serves pushforwards of states of at most " +
               std::to_string(kJvpNs64) + " entries (ns = 2N x state_cols = " + std::to_string(ns) + ")";
        return false;
    }
    *why = form == QC_SWEEP_FORM_64 ? qc_sweep_form64_unserved(d, "pushforwards") : qc_sweep_per_sample_why(d);
    return false;
}

extern "C" int qc_sweep_desc_jvp_supported(const qc_sweep_desc* d, int32_t* supported) {
    int rc = qc_sweep_validate_desc(d);
    if (rc) return rc;
    if (!supported) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep_desc_jvp_supported: supported is NULL");
    std::string why;
    const bool ok = qc_sweep_jvp_scope(d, &why);
    *supported = ok ? 1 : 0;
    if (!ok) (void)qc_sweep_fail(nullptr, QC_ERR_UNSUPPORTED, "qc_sweep pushforward: " + why);
    return QC_OK;
}

// The chunk totals W_c and their tangents Wdot_c, for the pushforward below and the Hessian product of qc_sweep_hvp.hip: grows h->dTotJ
// and launches qc_sweep_jvp_kernel<M> on `st` (S x n_chunks x 2 tiles of 256 doubles); "mfma32-sweep" handles go to
// qc_sweep32_jvp.hip (S x n_chunks x 2 matrices of 1024 doubles).
int qc_sweep_jvp_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, const double* dvZ,
                               const double* dvtheta, const double* dvscale, hipStream_t st, int64_t* chunk_out, int64_t* n_chunks_out) {
    if (h->mfma64) return qc_sweep64_jvp_launch_totals(h, dZ, S, dtheta, dscale, dvZ, dvtheta, dvscale, st, chunk_out, n_chunks_out);
    if (h->mfma32) return qc_sweep32_jvp_launch_totals(h, dZ, S, dtheta, dscale, dvZ, dvtheta, dvscale, st, chunk_out, n_chunks_out);
    SweepParams P;
    if (int rc = qc_sweep_plan_totals(h, S, h->dTotJ, 512, &P, chunk_out, n_chunks_out)) return rc;
#define QC_JVP_LAUNCH(M_)                                                                                                                    \
    hipLaunchKernelGGL(qc_sweep_jvp_kernel<M_>, dim3(qc_sweep_grid(P, kWaves)), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale, dvZ, dvtheta, \
                       dvscale, h->dTotJ.p)
    QC_SWEEP_FOR_M(P.m, QC_JVP_LAUNCH);
#undef QC_JVP_LAUNCH
    return QC_OK;
}

static int qc_sweep_jvp_launch(qc_sweep* h, const char* who, const double* dZ, const double* dinit, int64_t S, const double* dtheta,
                               const double* dscale, const double* dvZ, const double* dvinit, const double* dvtheta, const double* dvscale,
                               double* dfinals, double* dfids, double* dtfinals, double* dtfids, void* stream) {
    int rc = jvp_check(h, who, dZ, dinit, S, dtheta, dvZ || dvinit || dvtheta || dvscale, dfinals || dfids || dtfinals || dtfids, dvtheta != nullptr,
                       dvscale != nullptr, dfids || dtfids);
    if (rc) return rc;
    std::string& slot = *qc_sweep_err_slot();
    qc_device_guard guard(h->device);
    QC_SIDE_HIP(h, slot, guard.err);
    hipStream_t st = (hipStream_t)stream;
    int64_t chunk, n_chunks;
    if ((rc = qc_sweep_jvp_launch_totals(h, dZ, S, dtheta, dscale, dvZ, dvtheta, dvscale, st, &chunk, &n_chunks))) return rc;
    JvpFinParams F;
    F.n = h->n; F.ns = h->ns; F.n_chunks = (int)n_chunks;
    F.fid_kind = h->d.fid_kind; F.fid_form = h->d.fid_form; F.fid_n = h->fid_n;
    F.one_slot = 0;
    if (h->mfma64) {
        // 4 ns + 2 x 4096 doubles: 128 KiB of the 160 at ns = 2048 (the scope's bound); two slots only, a refused attribute is an error return
        const size_t lds64 = ((size_t)4 * h->ns + 8192) * 8;
        QC_SIDE_HIP(h, slot, hipFuncSetAttribute(reinterpret_cast<const void*>(&qc_sweep64_jvp_finish_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds64));
        hipLaunchKernelGGL(qc_sweep64_jvp_finish_kernel, dim3((unsigned)S), dim3(kFinT), lds64, st, F, (const double*)h->dTotJ.p, dinit, dvinit,
                           (const double*)h->dgr, (const double*)h->dgi, dfinals, dfids, dtfinals, dtfids);
    } else if (h->mfma32) {
        // 4 ns + 2 x 1024 doubles: 144 KiB of the 160 at ns = 4096
        size_t lds32 = ((size_t)4 * h->ns + 2048) * 8;
        const void* fn = reinterpret_cast<const void*>(&qc_sweep32_jvp_finish_kernel);
        // QC_SWEEP_JVP_ONE_SLOT=<non-zero integer> (diagnostic override; garbage and 0: not set): every launch, at any ns, as though the
        // two-slot request below had been refused.  The bits are the same by design, so each such launch says so on stderr.
        static const bool force_one_slot = getenv("QC_SWEEP_JVP_ONE_SLOT") && atoi(getenv("QC_SWEEP_JVP_ONE_SLOT")) != 0;
        if (force_one_slot) {
            F.one_slot = 1;
            lds32 = ((size_t)4 * h->ns + 1024) * 8;
            if (lds32 > 64 * 1024) QC_SIDE_HIP(h, slot, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds32));
            fprintf(stderr, "qcolloc: QC_SWEEP_JVP_ONE_SLOT is active: pushforward finish kernel through one slot\n");
        } else if (lds32 > 64 * 1024) {
            hipError_t ea = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds32);
            if (ea != hipSuccess) {
                // the runtime refuses the two-slot size: Q and Qdot through one slot (136 KiB at ns = 4096)
                (void)hipGetLastError();
                F.one_slot = 1;
                lds32 = ((size_t)4 * h->ns + 1024) * 8;
                ea = lds32 > 64 * 1024 ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds32) : hipSuccess;
            }
            QC_SIDE_HIP(h, slot, ea);
        }
        hipLaunchKernelGGL(qc_sweep32_jvp_finish_kernel, dim3((unsigned)S), dim3(kFinT), lds32, st, F, (const double*)h->dTotJ.p, dinit, dvinit,
                           (const double*)h->dgr, (const double*)h->dgi, dfinals, dfids, dtfinals, dtfids);
    } else {
        const size_t lds = ((size_t)4 * h->ns + 512) * 8;      // at most 4096 state entries: 132 KiB of the 160
        if (lds > 64 * 1024)
            QC_SIDE_HIP(h, slot, hipFuncSetAttribute(reinterpret_cast<const void*>(&qc_sweep_jvp_finish_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(qc_sweep_jvp_finish_kernel, dim3((unsigned)S), dim3(kFinT), lds, st, F, (const double*)h->dTotJ.p, dinit, dvinit,
                           (const double*)h->dgr, (const double*)h->dgi, dfinals, dfids, dtfinals, dtfids);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qc_sweep_fail(h, QC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return QC_OK;
}

extern "C" int qc_sweep_jvp_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                                const double* dvZ, const double* dvinit, const double* dvtheta, const double* dvscale, double* dfinals,
                                double* dfids, double* dtfinals, double* dtfids, void* stream) {
    return qc_sweep_jvp_launch(h, "qc_sweep_jvp_dev", dZ, dinit, S, dtheta, dscale, dvZ, dvinit, dvtheta, dvscale, dfinals, dfids, dtfinals, dtfids,
                               stream);
}

// The host-buffer entry point: stage, launch on the handle's stream, copy back, synchronise.
extern "C" int qc_sweep_jvp(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale, const double* vZ,
                            const double* vinit, const double* vtheta, const double* vscale, double* finals, double* fids, double* tfinals,
                            double* tfids) {
    const char* who = "qc_sweep_jvp";
    int rc = jvp_check(h, who, Z, init, S, theta, vZ || vinit || vtheta || vscale, finals || fids || tfinals || tfids, vtheta != nullptr,
                       vscale != nullptr, fids || tfids);
    if (rc) return rc;
    const size_t nS = (size_t)S, m = (size_t)h->d.m, p = (size_t)h->d.n_pert, ns = (size_t)h->ns, Zlen = (size_t)h->Zlen;
    qc_stage stage(h, qc_sweep_err_slot());
    const double* dZ = stage.in(h->sZ, Z, Zlen);
    const double* dinit = stage.in(h->sInit, init, ns);
    const double* dtheta = stage.in(h->sTheta, theta, nS * p);
    const double* dscale = stage.in(h->sScale, scale, nS * m);
    const double* dvZ = stage.in(h->sVZ, vZ, Zlen);
    const double* dvinit = stage.in(h->sVinit, vinit, ns);
    const double* dvtheta = stage.in(h->sVth, vtheta, nS * p);
    const double* dvscale = stage.in(h->sVsc, vscale, nS * m);
    double* dfinals = stage.out(h->sFinals, finals, nS * ns);
    double* dfids = stage.out(h->sFids, fids, nS);
    double* dtfinals = stage.out(h->sTfin, tfinals, nS * ns);
    double* dtfids = stage.out(h->sTfid, tfids, nS);
    if ((rc = stage.status())) return rc;
    if ((rc = qc_sweep_jvp_launch(h, who, dZ, dinit, S, dtheta, dscale, dvZ, dvinit, dvtheta, dvscale, dfinals, dfids, dtfinals, dtfids, h->stream)))
        return rc;
    return stage.finish();
}
