// Rollout sweeps: ONE trajectory of controls, S systems that differ by a few parameters, S final states and S fidelities
// (the reference's robustness check, unitary_sampling_problem.jl:204-244: `unitary_rollout(traj.a, timesteps, systems(zeta))[:, end]`
// and `iso_vec_unitary_fidelity` for every zeta of a grid).  Sample s is
//     G_s(a) = G_drift + sum_{j<p} theta[s,j] P_j + sum_{k<m} c[s,k] a_k G_k,      x_{t+1} = exp(dt_t G_s(a_t)) x_t,  x_0 = init.
// The work is S (T-1) independent 2N x 2N exponentials and S ordered products.
//
// 2N <= 16, up to 8 drives ("mfma16-sweep"): one wavefront per (sample, chunk of consecutive intervals) on v_mfma_f64_16x16x4_f64, every
// matrix one 16 x 16 tile in registers (lane maps: qc_mfma_kernels.hip header; sizes below 16 zero-padded -- the exponential of the
// padded generator is the exponential of the true one plus an identity block).  Once per wave: the sample's base tile
// G_drift + sum theta P_j and the m drive tiles, all in A layout; the sample's factors c[s,k] are folded into the control values.  Per
// interval: Y = dt G_s(a_t) / 2^sq with ||Y||_1 <= 1/8 (wave-uniform sq), the degree-8 Taylor polynomial in Horner form
// R_k = Y R_k+1 + I/(k-1)! (threshold, degree and truncation 4e-14 of qc_mfma_exp.hip, without its Frechet chains), sq squarings, and
// W <- E_t W onto the running chunk product.  Squarings and the product need E as the LEFT factor; a D-layout tile read as the A
// operand acts as its transpose (qc_mfma_exp.hip header), so E^T is made by an LDS transpose and used as the A operand -- an identity
// for every matrix, antisymmetric generator or not (Lindblad generators are not).  MFMAs per interval: 8 x 4 + 4 sq + 4.
// Nothing leaves registers / LDS until the chunk's total is done; the totals go to handle scratch, S x n_chunks tiles.
// A second launch, one workgroup per sample, chains the totals onto init in ascending order, stores the final state and evaluates
// the fidelity (definitions of qc_fidelity.hip).  No atomics, no order that depends on scheduling: repeated calls give the same bits.
//
// 16 < 2N <= 64, or more than 8 drives ("rollout-per-sample"): a small kernel writes the sample's generator set (perturbed drift,
// scaled drives), the rollout kernels of qc_rollout.hip run on it, and the same final-state / fidelity launch follows.  Correctness,
// not speed.
//
// A descriptor with wide = QC_SWEEP_WIDE takes the matrix cores up to 2N = 32: 16 < 2N <= 32 with up to 8 drives is "mfma32-sweep"
// (qc_sweep32.hip, 2 x 2 tiles a matrix); the second launch below is shared, with ld = 32.  wide = 0 is the routing above, unchanged.
// `wide` is a bit field: bit 1 (QC_SWEEP_WIDE_PARAMS, only together with bit 0) changes nothing here -- the form, the launch and the
// forward sweep are those of wide = 1; it lets qc_sweep_grad_params* and qc_sweep_vjp* serve the parameter outputs in that form.
// Bits 3, 4, 6 and 8 (QC_SWEEP_WIDE_STORED, _TANGENT, _NOISE, _HESSIAN) likewise: each lets one more family of entry points serve that form.
// Bit 10 (QC_SWEEP_WIDE_64, only together with bit 0) takes the matrix cores up to 2N = 64: 32 < 2N <= 64 with up to 16 drives is
// "mfma64-sweep" (qc_sweep64.hip: 4 x 4 tiles a matrix in LDS, one workgroup per (sample, chunk), its own fill constant in the chunk
// rule); the second launch below is shared, with ld = 64.  That form serves the forward sweep only -- gradients, pullbacks, pushforwards,
// Hessian products and noise sweeps answer QC_ERR_UNSUPPORTED there -- and descriptors with 2N <= 32 ignore the bit completely.
// Bits 11 and 13 (QC_SWEEP_WIDE_64_GRAD, only with bit 10; QC_SWEEP_WIDE_64_PARAMS, only with bit 11) change nothing here either: they let
// qc_sweep_grad* / qc_sweep_vjp*, and then their parameter outputs, serve that form (qc_sweep64_grad.hip).  Bit 14
// (QC_SWEEP_WIDE_64_TANGENT, only with bit 10) likewise: it lets qc_sweep_jvp* serve that form (qc_sweep64_jvp.hip), any generators.  Bit 16
// (QC_SWEEP_WIDE_64_NOISE, only with bit 10) likewise: it lets qc_sweep_noise_* serve that form (qc_sweep64_noise.hip).  Bit 18
// (QC_SWEEP_WIDE_64_STORED, only with bit 11) likewise: with reserved1[0] = QC_SWEEP_STORED_STATES it lets qc_sweep_grad* / qc_sweep_vjp* serve
// that form by the stored-state walk, any generators (qc_sweep64_open_grad.hip).
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "qc_mfma_common.h"
#include "qc_side.h"
#include "qc_sweep16_common.h"
#include "qc_sweep_internal.h"

namespace {

using namespace qc_sweep16;         // constants, table, tile load, generator, squaring rule and product of the 16 x 16 form

constexpr int kSMmax = 8;           // drive tiles a wave keeps in registers
constexpr int kFinT = 256;          // threads of the final-state / fidelity workgroup
constexpr long long kSweepFill = 2048;   // waves that give every SIMD a couple: 256 CUs x 4 SIMDs x 2
constexpr long long kSweepFill64 = 256;  // "mfma64-sweep": an item is a workgroup of 16 waves whose 135 168 B of LDS leave room for one per CU: 256 CUs x 1
constexpr int kSMmax64 = 16;             // drives of the "mfma64-sweep" form: nothing is resident per drive, lane u of a wave carries drive u's amplitude

struct FinParams {
    int n, ns, ld, n_chunks, fid_kind, fid_form, fid_n;
    long long src_stride;        // 0: every sample starts from the same state (init); ns: per-sample states (per-sample form)
};

template <int M>
__global__ __launch_bounds__(64 * kWaves, 2) void qc_sweep_mfma16_kernel(const SweepParams P, const double* __restrict__ Z,
                                                                           const double* __restrict__ theta, const double* __restrict__ scale,
                                                                           double* __restrict__ tot) {
    __shared__ double scr_all[kWaves * kTile];
    const WaveItem w = wave_item(kWaves);
    double* __restrict__ scr = scr_all + w.wq * kTile;
    if (w.item >= P.items) return;
    const ChunkRange ch = chunk_range(w.item, P.n_chunks, P.chunk, P.n_int);
    const int lane = w.lane, t0 = ch.t0, t1 = ch.t1, g = lane >> 4, j = lane & 15;
    const long long item = w.item, s = ch.s;
    const int m = P.m;
    const bool ft = P.off_dt >= 0;
    const v4d IdB = identity_B(g, j);
    const v4d zero = {0.0, 0.0, 0.0, 0.0};

    // ---- once per wave: the sample's base tile and the drive tiles ---------------------------------------------------------
    const v4d base = base_tile(P.img, m, P.p, theta, s, lane);
    v4d Gj[M];
    resident_tiles(P.img, m, lane, Gj);
    // lane l holds the sample's factor of drive min(l, m-1); folded into the control values
    const int kl = lane < m ? lane : (m > 0 ? m - 1 : 0);
    const double cl = (scale && m > 0) ? scale[s * m + kl] : 1.0;

    const double* __restrict__ z = Z + (long long)t0 * P.zdim;
    double av = m > 0 ? z[P.off_a + kl] : 0.0;
    const double hfix = opaque_scalar(P.dt_fixed);      // keeps the two arms apart: no flat load (qc_mfma_common.h)
    double h = ft ? z[P.off_dt] : hfix;
    v4d W = IdB;
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        // the next interval's controls and timestep are requested before this interval's products
        const double* __restrict__ zn = Z + (long long)(t + 1 < t1 ? t + 1 : t) * P.zdim;
        const double av_n = m > 0 ? zn[P.off_a + kl] : 0.0;
        const double h_n = ft ? zn[P.off_dt] : hfix;
        const double al = av * cl;
        const v4d Ga = generator(base, Gj, m, al);
        const int sq = squarings(h, Ga);
        const double sc = ldexp(1.0, -sq);
        const v4d Y = (h * sc) * Ga;
        // Horner: R_deg+1 = I/deg!,  R_k = Y R_k+1 + I/(k-1)!
        // (the coefficients 1 / (k-1)! from a table of correctly rounded constants: the last one is exactly 1, so a zero generator gives
        //  exactly the identity; computed in the loop they cost two f64 divisions a step)
        v4d R = kInvFact[kDeg] * IdB;
#pragma unroll 1
        for (int k = kDeg; k >= 1; --k)        // (unrolled, the eight scaled identities are hoisted out of the interval loop: 64 VGPRs)
            R = mma16(Y, R, kInvFact[k - 1] * IdB);
        for (int q = 0; q < sq; ++q) {
            const v4d Et = lds_transpose16(scr, R, g, j);
            R = mma16(Et, R, zero);
        }
        const v4d Et = lds_transpose16(scr, R, g, j);     // E^T in D layout = E in A layout
        W = mma16(Et, W, zero);
        av = av_n;
        h = h_n;
    }
    double* __restrict__ o = tot + item * 256;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[j * 16 + 4 * r + g] = W[r];
}

// The generator set of one sample for the rollout kernels: [G_drift + sum theta_j P_j | c_k G_k], column-major n x n each
__global__ __launch_bounds__(256) void qc_sweep_gen_kernel(int n2, int m, int p, const double* __restrict__ G, const double* __restrict__ theta_s,
                                                           const double* __restrict__ scale_s, double* __restrict__ out) {
    const int total = (1 + m) * n2;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int mat = idx / n2, e = idx - mat * n2;
        double v = G[idx];
        if (mat == 0) {
            for (int q = 0; q < p; ++q) v = fma(theta_s[q], G[(size_t)(1 + m + q) * n2 + e], v);
        } else if (scale_s) {
            v *= scale_s[mat - 1];
        }
        out[idx] = v;
    }
}

// One workgroup per sample: x = Q_last ... Q_0 src (ascending order), final state, fidelity.
// Fidelity from t = (g_r . x) + i (g_i . x):  unitary |t| / n or |t|^2 / n^2,  ket |t|^2,  density operator Re t  (qc_fidelity.hip).
__global__ __launch_bounds__(kFinT) void qc_sweep_finish_kernel(const FinParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                                                const double* __restrict__ gr, const double* __restrict__ gi,
                                                                double* __restrict__ finals, double* __restrict__ fids) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double red[2][kFinT / 64];
    const int tid = threadIdx.x, n = F.n, ns = F.ns, ld = F.ld, l2 = ld * ld;
    const long long s = blockIdx.x;
    double* cur = sm;
    double* nxt = sm + ns;
    double* Q = sm + 2 * ns;
    const double* __restrict__ x0 = src + s * F.src_stride;
    for (int idx = tid; idx < ns; idx += kFinT) cur[idx] = x0[idx];
    const double* __restrict__ Qs = tot + s * F.n_chunks * (long long)l2;
    for (int c = 0; c < F.n_chunks; ++c) {
        __syncthreads();
        for (int idx = tid; idx < l2; idx += kFinT) Q[idx] = Qs[(long long)c * l2 + idx];
        __syncthreads();
        for (int idx = tid; idx < ns; idx += kFinT) {
            const int r = idx % n, col = idx / n;
            double acc = 0.0;
            for (int q = 0; q < n; ++q) acc = fma(Q[r + ld * q], cur[q + n * col], acc);
            nxt[idx] = acc;
        }
        double* tmp = cur; cur = nxt; nxt = tmp;
    }
    __syncthreads();
    if (finals)
        for (int idx = tid; idx < ns; idx += kFinT) finals[s * ns + idx] = cur[idx];
    if (!fids) return;
    double ar = 0.0, ai = 0.0;
    for (int i = tid; i < ns; i += kFinT) {
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
        double Fv;      // the mapping of qc_fidelity_kernel (qc_fidelity.hip), written out again: sharing it changed that kernel's generated code
        if (F.fid_kind == QC_FID_UNITARY) Fv = F.fid_form == QC_FID_FORM_ABS2 ? (tr * tr + ti * ti) / (nn * nn) : sqrt(tr * tr + ti * ti) / nn;
        else if (F.fid_kind == QC_FID_KET) Fv = tr * tr + ti * ti;
        else Fv = tr;
        fids[s] = Fv;
    }
}

}  // namespace

// the pieces the family's other files share (qc_sweep_internal.h)
static thread_local std::string g_swerr;
int qc_sweep_fail(qc_side* h, int code, const std::string& msg) { return qc_side_fail(h, &g_swerr, code, msg); }
std::string* qc_sweep_err_slot() { return &g_swerr; }

// The launch rule, in one place.  n_chunks = 1 once the samples alone give every SIMD a couple of waves; fewer samples split the
// trajectory, up to ceil(sqrt(T-1)) chunks (beyond that the ordered chain of the second launch outweighs what the first gains).
// "mfma64-sweep": the same rule with items that are whole workgroups, one per CU -- n_chunks = 1 once S >= 256.
void qc_sweep_chunks(qc_sweep_form form, int64_t S, int64_t T, int64_t* chunk, int64_t* n_chunks) {
    const int64_t n_int = T - 1, fill = form == QC_SWEEP_FORM_64 ? kSweepFill64 : kSweepFill;
    const int64_t want = S >= fill ? 1 : (fill + S - 1) / S;
    int64_t r = 1;
    while (r * r < n_int) ++r;
    const int64_t nch = want < r ? want : r;
    *chunk = (n_int + nch - 1) / nch;
    *n_chunks = (n_int + *chunk - 1) / *chunk;
}

int qc_sweep_plan_totals(qc_sweep* h, int64_t S, qc_buf& buf, size_t doubles_per_item, SweepParams* P, int64_t* chunk, int64_t* n_chunks) {
    int64_t ch, nch;
    qc_sweep_chunks(h->mfma64 ? QC_SWEEP_FORM_64 : QC_SWEEP_FORM_16, S, h->d.T, &ch, &nch);
    QC_SIDE_HIP(h, g_swerr, h->grow(buf, (size_t)S * nch * doubles_per_item));
    *P = qc_sweep_params(h, S, ch, nch);
    *chunk = ch;      // as before: untouched when the allocation fails
    *n_chunks = nch;
    return QC_OK;
}

int qc_sweep_validate_desc(const qc_sweep_desc* d) {
    if (!d) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: NULL descriptor");
    if (d->N < 1) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: N must be >= 1");
    if (d->m < 0) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: m must be >= 0");
    if (d->T < 2) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: T must be >= 2");
    if (d->T > (1ll << 30)) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: T too large");
    if (d->zdim < 1 || d->global_dim < 0) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: bad zdim / global_dim");
    if (d->off_a < 0 || (int64_t)d->off_a + d->m > d->zdim) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: off_a outside the knot (m entries from off_a must fit inside zdim)");
    if (d->off_dt < -1 || d->off_dt >= d->zdim) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: off_dt outside the knot");
    if (d->n_pert < 0 || d->n_pert > QC_MAX_PERT) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: n_pert must be in 0 .. QC_MAX_PERT (8)");
    if (d->n_pert > 0 && !d->G_pert) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: n_pert > 0 but G_pert is NULL");
    if (!d->G_drift) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: G_drift is NULL");
    if (d->m > 0 && !d->G_drives) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: m > 0 but G_drives is NULL");
    if (d->state_cols < 0) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: state_cols must be >= 0");
    const int nc = d->state_cols == 0 ? d->N : d->state_cols;
    if (d->fid_kind != QC_SWEEP_FID_NONE) {
        if (d->fid_kind != QC_FID_UNITARY && d->fid_kind != QC_FID_KET && d->fid_kind != QC_FID_DENSITY)
            return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: unknown fid_kind");
        if (d->fid_form != QC_FID_FORM_ABS && d->fid_form != QC_FID_FORM_ABS2) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: unknown fid_form");
        if (!d->goal_iso) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: a fidelity needs goal_iso");
        if (d->fid_kind == QC_FID_UNITARY) {
            if (nc != d->N) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: the unitary fidelity needs state_cols = 0 or N");
            if (d->subspace) {
                if (d->n_sub < 1 || d->n_sub > d->N) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: n_sub must be in 1 .. N");
                for (int a = 0; a < d->n_sub; ++a) {
                    if (d->subspace[a] < 0 || d->subspace[a] >= d->N) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: subspace index outside 0 .. N-1");
                    for (int b = 0; b < a; ++b)
                        if (d->subspace[b] == d->subspace[a]) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: subspace levels must be distinct");
                }
            }
        } else {
            if (d->subspace || d->fid_form != QC_FID_FORM_ABS)
                return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: subspace and fid_form apply to QC_FID_UNITARY only");
            if (nc != 1) return qc_sweep_fail(nullptr, QC_ERR_INVALID, d->fid_kind == QC_FID_KET ? "qc_sweep: the ket fidelity needs state_cols = 1"
                                                                                             : "qc_sweep: the density-operator fidelity needs state_cols = 1");
            if (d->fid_kind == QC_FID_DENSITY && qc_isqrt_exact(d->N) < 0)
                return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: the density-operator fidelity needs N = levels^2");
        }
    }
    if (2 * (int64_t)d->N > 64) return qc_sweep_fail(nullptr, QC_ERR_UNSUPPORTED, "qc_sweep: 2N = " + std::to_string(2 * (int64_t)d->N) + " exceeds the supported 2N <= 64");
    if (2 * (int64_t)d->N * nc > 4096) return qc_sweep_fail(nullptr, QC_ERR_UNSUPPORTED, "qc_sweep: states of more than 4096 entries (2N x state_cols) are not supported");
    if (d->m > 64) return qc_sweep_fail(nullptr, QC_ERR_UNSUPPORTED, "qc_sweep: more than 64 drives are not supported");
    // bits 1 (QC_SWEEP_WIDE_PARAMS), 3 (QC_SWEEP_WIDE_STORED), 4 (QC_SWEEP_WIDE_TANGENT), 6 (QC_SWEEP_WIDE_NOISE) and 8
    // (QC_SWEEP_WIDE_HESSIAN) only together with bit 0; bits 2, 5 and 7 are not assigned: 0, 1, 3, 9, 11, 17, 19, 25, 27, each of the
    // eight odd values | 64, and each of those sixteen odd values | 256; bit 10 (QC_SWEEP_WIDE_64) likewise only together with bit 0:
    // each of those thirty-two odd values | 1024; bit 9 is not assigned
    // bit 11 (QC_SWEEP_WIDE_64_GRAD) only together with bits 0 and 10: each of those thirty-two values | 1024 | 2048
    // bit 13 (QC_SWEEP_WIDE_64_PARAMS) only together with bits 0, 10 and 11: each of those | 8192; bit 12 is not assigned
    // bit 14 (QC_SWEEP_WIDE_64_TANGENT) only together with bits 0 and 10 (not 11 or 13: nothing is reversed): each valid value that has both | 16384
    // bit 16 (QC_SWEEP_WIDE_64_NOISE) only together with bits 0 and 10 (none of 11, 13, 14 needed): each valid value that has both | 65536; bit 15 is not assigned
    // bit 18 (QC_SWEEP_WIDE_64_STORED) only together with bits 0, 10 and 11, as bit 13: each valid value that has all three | 262144; bit 17 and everything from bit 19 up are not assigned
    if ((d->wide & ~(QC_SWEEP_WIDE | QC_SWEEP_WIDE_PARAMS | QC_SWEEP_WIDE_STORED | QC_SWEEP_WIDE_TANGENT | QC_SWEEP_WIDE_NOISE | QC_SWEEP_WIDE_HESSIAN | QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_PARAMS | QC_SWEEP_WIDE_64_TANGENT | QC_SWEEP_WIDE_64_NOISE | QC_SWEEP_WIDE_64_STORED)) != 0 ||
        (d->wide != 0 && !(d->wide & QC_SWEEP_WIDE)) || ((d->wide & QC_SWEEP_WIDE_64_GRAD) && !(d->wide & QC_SWEEP_WIDE_64)) ||
        ((d->wide & QC_SWEEP_WIDE_64_PARAMS) && !(d->wide & QC_SWEEP_WIDE_64_GRAD)) ||
        ((d->wide & QC_SWEEP_WIDE_64_STORED) && !(d->wide & QC_SWEEP_WIDE_64_GRAD)) ||
        ((d->wide & QC_SWEEP_WIDE_64_TANGENT) && !(d->wide & QC_SWEEP_WIDE_64)) ||
        ((d->wide & QC_SWEEP_WIDE_64_NOISE) && !(d->wide & QC_SWEEP_WIDE_64)))
        return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: wide must be 0 or QC_SWEEP_WIDE (1), alone or with QC_SWEEP_WIDE_PARAMS (2), QC_SWEEP_WIDE_STORED (8), QC_SWEEP_WIDE_TANGENT (16), QC_SWEEP_WIDE_NOISE (64) and / or QC_SWEEP_WIDE_HESSIAN (256): 0, 1, 3, 9, 11, 17, 19, 25 or 27, or one of those eight | 64, or one of the sixteen odd values | 256; or one of the thirty-two odd values | QC_SWEEP_WIDE_64 (1024); or one of those | QC_SWEEP_WIDE_64_GRAD (2048); or one of those | QC_SWEEP_WIDE_64_PARAMS (8192); or any of those that has QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_TANGENT (16384); or any of those that has QC_SWEEP_WIDE_64 | QC_SWEEP_WIDE_64_NOISE (65536); or any of those that has QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_STORED (262144)");
    if (d->reserved1[0] != 0 && d->reserved1[0] != QC_SWEEP_STORED_STATES)
        return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep: reserved1[0] must be 0 or QC_SWEEP_STORED_STATES (1)");
    return QC_OK;
}

qc_sweep_form qc_sweep_desc_form(const qc_sweep_desc* d) {
    if (2 * d->N > 32)      // only with both bits; below, the bit is not looked at
        return ((d->wide & QC_SWEEP_WIDE) && (d->wide & QC_SWEEP_WIDE_64) && 2 * d->N <= 64 && d->m <= kSMmax64) ? QC_SWEEP_FORM_64 : QC_SWEEP_FORM_PER_SAMPLE;
    if (d->m > kSMmax) return QC_SWEEP_FORM_PER_SAMPLE;
    if (2 * d->N <= 16) return QC_SWEEP_FORM_16;
    return ((d->wide & QC_SWEEP_WIDE) && 2 * d->N <= 32) ? QC_SWEEP_FORM_32 : QC_SWEEP_FORM_PER_SAMPLE;
}
bool qc_sweep_desc_is_mfma(const qc_sweep_desc* d) { return qc_sweep_desc_form(d) != QC_SWEEP_FORM_PER_SAMPLE; }

std::string qc_sweep_per_sample_why(const qc_sweep_desc* d) {
    const int n = 2 * d->N, top = (d->wide & QC_SWEEP_WIDE) ? 32 : 16;      // wide descriptors: "mfma32-sweep" up to 2N = 32
    if (n > 32 && (d->wide & QC_SWEEP_WIDE) && (d->wide & QC_SWEEP_WIDE_64))      // "mfma64-sweep" but for its drive limit
        return "the handle takes the rollout-per-sample form (" + std::to_string(d->m) + " drives > 16)";
    return n > top ? "the handle takes the rollout-per-sample form (2N = " + std::to_string(n) + " > " + std::to_string(top) + ")"
                   : "the handle takes the rollout-per-sample form (" + std::to_string(d->m) + " drives > 8)";
}

std::string qc_sweep_form64_why(const qc_sweep_desc* d) {
    return "the handle takes the mfma64-sweep form (2N = " + std::to_string(2 * d->N) + "), which serves the forward sweep only";
}

std::string qc_sweep_form64_unserved(const qc_sweep_desc* d, const char* what) {
    if (!(d->wide & QC_SWEEP_WIDE_64_GRAD)) return qc_sweep_form64_why(d);
    return "the handle takes the mfma64-sweep form (2N = " + std::to_string(2 * d->N) + "), which does not serve " + what;
}

int qc_sweep_check(qc_sweep* h, const char* who, const bool qc_sweep::*ok, const char* scope, const std::string qc_sweep::*why, const void* Z,
                   const void* init, const char* missing, int64_t S, const void* theta) {
    const std::string pre = std::string(who) + ": ";
    if (!h) return qc_sweep_fail(nullptr, QC_ERR_INVALID, pre + "NULL handle");
    if (ok && !(h->*ok)) return qc_sweep_fail(h, QC_ERR_UNSUPPORTED, scope + h->*why);
    if (!Z || !init) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "NULL input");
    if (missing) return qc_sweep_fail(h, QC_ERR_INVALID, pre + missing + " is NULL");
    if (S < 1 || S > (1ll << 24)) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "S must be in 1 .. 2^24");
    if (h->d.n_pert > 0 && !theta) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "theta is NULL but the handle has perturbations");
    return QC_OK;
}

int qc_sweep_launch_totals(qc_sweep* h, const double* dZ, int64_t S, const double* dtheta, const double* dscale, hipStream_t st, int64_t* chunk_out,
                           int64_t* n_chunks_out) {
    if (h->mfma64) return qc_sweep64_launch_totals(h, dZ, S, dtheta, dscale, st, chunk_out, n_chunks_out);
    if (h->mfma32) return qc_sweep32_launch_totals(h, dZ, S, dtheta, dscale, st, chunk_out, n_chunks_out);
    SweepParams P;
    if (int rc = qc_sweep_plan_totals(h, S, h->dTot, 256, &P, chunk_out, n_chunks_out)) return rc;
#define QC_SWEEP_LAUNCH(M_) \
    hipLaunchKernelGGL(qc_sweep_mfma16_kernel<M_>, dim3(qc_sweep_grid(P, kWaves)), dim3(64 * kWaves), 0, st, P, dZ, dtheta, dscale, h->dTot.p)
    QC_SWEEP_FOR_M(P.m, QC_SWEEP_LAUNCH);
#undef QC_SWEEP_LAUNCH
    return QC_OK;
}

extern "C" const char* qc_sweep_last_error(const qc_sweep* h) { return h ? h->err.c_str() : g_swerr.c_str(); }

extern "C" int64_t qc_sizeof_sweep_desc(void) { return (int64_t)sizeof(qc_sweep_desc); }

extern "C" int qc_sweep_desc_validate(const qc_sweep_desc* d) { return qc_sweep_validate_desc(d); }

extern "C" int qc_sweep_desc_launch(const qc_sweep_desc* d, int64_t S, int32_t* mfma, int64_t* chunk, int64_t* n_chunks) {
    int rc = qc_sweep_validate_desc(d);
    if (rc) return rc;
    if (S < 1) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep_desc_launch: S must be >= 1");
    const qc_sweep_form form = qc_sweep_desc_form(d);
    const bool mf = form != QC_SWEEP_FORM_PER_SAMPLE;
    int64_t ch = d->T - 1, nch = 0;      // per-sample form: the rollout kernels' own scan, no totals
    if (mf) qc_sweep_chunks(form, S, d->T, &ch, &nch);
    if (mfma) *mfma = mf ? 1 : 0;
    if (chunk) *chunk = ch;
    if (n_chunks) *n_chunks = nch;
    return QC_OK;
}

extern "C" const char* qc_sweep_kernel_name(const qc_sweep* h) {
    if (!h) return "none";
    return h->mfma64 ? "mfma64-sweep" : h->mfma32 ? "mfma32-sweep" : h->mfma ? "mfma16-sweep" : "rollout-per-sample";
}

extern "C" void qc_sweep_destroy(qc_sweep* h) {
    if (!h) return;
    h->release_device();
    delete h;
}

extern "C" int qc_sweep_create(const qc_sweep_desc* d, qc_sweep** out) {
    if (!out) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep_create: out is NULL");
    *out = nullptr;
    int rc = qc_sweep_validate_desc(d);
    if (rc) return rc;
    if ((rc = qc_side_check_device(d->device, "qc_sweep_create", &g_swerr))) return rc;
    qc_side_new<qc_sweep> h(new qc_sweep());
    h->d = *d;
    h->device = d->device;
    h->mfma = qc_sweep_desc_is_mfma(d);
    h->mfma32 = qc_sweep_desc_form(d) == QC_SWEEP_FORM_32;
    h->mfma64 = qc_sweep_desc_form(d) == QC_SWEEP_FORM_64;
    h->wide64_grad = h->mfma64 && (d->wide & QC_SWEEP_WIDE_64_GRAD);
    h->wide64_par = h->wide64_grad && (d->wide & QC_SWEEP_WIDE_64_PARAMS);
    h->wide64_stored = h->wide64_grad && (d->wide & QC_SWEEP_WIDE_64_STORED);
    h->wide64_tangent = h->mfma64 && (d->wide & QC_SWEEP_WIDE_64_TANGENT);
    h->wide64_noise = h->mfma64 && (d->wide & QC_SWEEP_WIDE_64_NOISE);
    h->wide_par = h->mfma32 && (d->wide & QC_SWEEP_WIDE_PARAMS);
    h->wide_stored = h->mfma32 && (d->wide & QC_SWEEP_WIDE_STORED);
    h->wide_tangent = h->mfma32 && (d->wide & QC_SWEEP_WIDE_TANGENT);
    h->wide_noise = h->mfma32 && (d->wide & QC_SWEEP_WIDE_NOISE);
    h->wide_hessian = h->mfma32 && (d->wide & QC_SWEEP_WIDE_HESSIAN);
    h->grad_ok = qc_sweep_grad_scope(d, &h->grad_why);      // from the caller's matrices, which the handle does not keep
    h->vjp_ok = qc_sweep_vjp_scope(d, &h->vjp_why);
    h->jvp_ok = qc_sweep_jvp_scope(d, &h->jvp_why);
    h->hvp_ok = qc_sweep_hvp_scope(d, &h->hvp_why);
    h->noise_ok = qc_sweep_noise_scope(d, &h->noise_why);
    {      // the noise gradient keeps the closed walk and its scope, whatever reserved1[0] says
        std::string closed_why;
        const bool closed_ok = qc_sweep_closed_grad_scope(d, &closed_why);
        h->noise_grad_ok = h->noise_ok && closed_ok;
        h->noise_grad_why = h->noise_ok ? closed_why : h->noise_why;
    }
    h->stored = d->reserved1[0] == QC_SWEEP_STORED_STATES;
    const int N = d->N, n = 2 * N, n2 = n * n, m = d->m, p = d->n_pert;
    h->n = n;
    h->nc = d->state_cols == 0 ? N : d->state_cols;
    h->ns = n * h->nc;
    h->Zlen = d->T * (int64_t)d->zdim + d->global_dim;
    // generators: drift, drives, perturbations
    const int nm = 1 + m + p;
    std::vector<double> G((size_t)nm * n2);
    memcpy(G.data(), d->G_drift, (size_t)n2 * 8);
    if (m) memcpy(G.data() + n2, d->G_drives, (size_t)m * n2 * 8);
    if (p) memcpy(G.data() + (size_t)(1 + m) * n2, d->G_pert, (size_t)p * n2 * 8);
    std::vector<double> img;
    if (h->mfma64) {
        img.resize((size_t)nm * 4096);
        for (int mat = 0; mat < nm; ++mat) qc_sweep64_image(G.data() + (size_t)mat * n2, n, img.data() + (size_t)mat * 4096);
    } else if (h->mfma32) {
        img.resize((size_t)nm * 1024);
        for (int mat = 0; mat < nm; ++mat) qc_sweep32_image(G.data() + (size_t)mat * n2, n, img.data() + (size_t)mat * 1024);
    } else if (h->mfma) {   // A layout: lane (g, i) reg kk holds G[i][4 kk + g], zero outside n x n
        img.assign((size_t)nm * 256, 0.0);
        for (int mat = 0; mat < nm; ++mat)
            for (int kk = 0; kk < 4; ++kk)
                for (int lane = 0; lane < 64; ++lane) {
                    const int g = lane >> 4, i = lane & 15, col = 4 * kk + g;
                    if (i < n && col < n) img[(size_t)mat * 256 + kk * 64 + lane] = G[(size_t)mat * n2 + (size_t)col * n + i];
                }
    }
    std::vector<double> gr, gi;      // the fidelity's constant vectors
    if (d->fid_kind != QC_SWEEP_FID_NONE) {
        gr.resize(h->ns);
        gi.resize(h->ns);
        h->fid_n = qc_fidelity_goal(d->fid_kind, N, d->goal_iso, d->subspace, d->n_sub, gr.data(), gi.data());
    }
    h->d.G_drift = h->d.G_drives = h->d.G_pert = h->d.goal_iso = nullptr;
    h->d.subspace = nullptr;
    qc_device_guard guard(d->device);
    QC_SIDE_HIP(nullptr, g_swerr, guard.err);
    if (h->mfma) {
        QC_SIDE_HIP(nullptr, g_swerr, h->alloc(&h->dImg, img.size(), img.data()));
    } else {
        const size_t T = (size_t)d->T;
        QcParams P{};
        P.n = n; P.nc = h->nc;
        size_t nE, nQ, nS;
        int ch, nch;
        qc_rollout_scratch(P, (long long)T, &nE, &nQ, &nS, &ch, &nch);
        QC_SIDE_HIP(nullptr, g_swerr, h->alloc(&h->dG, G.size(), G.data()));
        QC_SIDE_HIP(nullptr, g_swerr, h->alloc(&h->dGs, (size_t)(1 + m) * n2));
        QC_SIDE_HIP(nullptr, g_swerr, h->alloc(&h->dRE, nE));
        QC_SIDE_HIP(nullptr, g_swerr, h->alloc(&h->dRQ, nQ));
        QC_SIDE_HIP(nullptr, g_swerr, h->alloc(&h->dRS, nS));
        QC_SIDE_HIP(nullptr, g_swerr, h->alloc(&h->dRout, (size_t)h->ns * T));
    }
    if (!gr.empty()) {
        QC_SIDE_HIP(nullptr, g_swerr, h->alloc(&h->dgr, gr.size(), gr.data()));
        QC_SIDE_HIP(nullptr, g_swerr, h->alloc(&h->dgi, gi.size(), gi.data()));
    }
    QC_SIDE_HIP(nullptr, g_swerr, h->grow(h->sZ, (size_t)h->Zlen));
    QC_SIDE_HIP(nullptr, g_swerr, h->grow(h->sInit, (size_t)h->ns));
    QC_SIDE_HIP(nullptr, g_swerr, h->open_stream());
    *out = h.release();
    return QC_OK;
}

// the argument checks of both entry points, in the order of the header
static int eval_check(qc_sweep* h, const char* who, const double* Z, const double* init, int64_t S, const double* theta, const double* finals,
                      const double* fids) {
    int rc = qc_sweep_check(h, who, nullptr, nullptr, nullptr, Z, init, nullptr, S, theta);
    if (rc) return rc;
    const std::string pre = std::string(who) + ": ";
    if (!finals && !fids) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "finals and fids are both NULL");
    if (fids && h->d.fid_kind == QC_SWEEP_FID_NONE) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "fidelities requested from a handle created without one");
    return QC_OK;
}

// the second launch: qc_sweep_finish_kernel, one workgroup per sample
static int finish_launch(qc_sweep* h, const FinParams& F, int64_t S, const double* src, double* dfinals, double* dfids, hipStream_t st) {
    const size_t lds = ((size_t)2 * h->ns + (size_t)F.ld * F.ld) * 8;
    if (lds > 64 * 1024)
        QC_SIDE_HIP(h, g_swerr, hipFuncSetAttribute(reinterpret_cast<const void*>(&qc_sweep_finish_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(qc_sweep_finish_kernel, dim3((unsigned)S), dim3(kFinT), lds, st, F, (const double*)h->dTot.p, src, (const double*)h->dgr,
                       (const double*)h->dgi, dfinals, dfids);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qc_sweep_fail(h, QC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return QC_OK;
}

// MFMA forms: the same launch on the chunk totals in h->dTot, for the noise sweep of qc_sweep_noise.hip
int qc_sweep_launch_finish(qc_sweep* h, int64_t S, int64_t n_chunks, const double* dinit, double* dfinals, double* dfids, hipStream_t st) {
    FinParams F;
    F.n = h->n; F.ns = h->ns;
    F.fid_kind = h->d.fid_kind; F.fid_form = h->d.fid_form; F.fid_n = h->fid_n;
    F.ld = h->mfma64 ? 64 : h->mfma32 ? 32 : 16; F.n_chunks = (int)n_chunks; F.src_stride = 0;
    return finish_launch(h, F, S, dinit, dfinals, dfids, st);
}

static int qc_sweep_eval_launch(qc_sweep* h, const char* who, const double* dZ, const double* dinit, int64_t S, const double* dtheta,
                                const double* dscale, double* dfinals, double* dfids, void* stream) {
    int rc = eval_check(h, who, dZ, dinit, S, dtheta, dfinals, dfids);
    if (rc) return rc;
    qc_device_guard guard(h->device);
    QC_SIDE_HIP(h, g_swerr, guard.err);
    hipStream_t st = (hipStream_t)stream;
    const int n = h->n, m = h->d.m, p = h->d.n_pert;
    FinParams F;
    F.n = n; F.ns = h->ns;
    F.fid_kind = h->d.fid_kind; F.fid_form = h->d.fid_form; F.fid_n = h->fid_n;
    const double* src;
    if (h->mfma) {
        int64_t chunk, n_chunks;
        rc = qc_sweep_launch_totals(h, dZ, S, dtheta, dscale, st, &chunk, &n_chunks);
        if (rc) return rc;
        F.ld = h->mfma64 ? 64 : h->mfma32 ? 32 : 16; F.n_chunks = (int)n_chunks; F.src_stride = 0;
        src = dinit;
    } else {
        QC_SIDE_HIP(h, g_swerr, h->grow(h->dFin, (size_t)S * h->ns));
        QcParams P{};
        P.N = h->d.N; P.n = n; P.nc = h->nc; P.s = h->ns; P.m = m; P.zdim = h->d.zdim; P.off_a = h->d.off_a; P.off_dt = h->d.off_dt;
        P.dt_fixed = h->d.dt_fixed; P.G = h->dGs;
        const int n2 = n * n, gen_grid = ((1 + m) * n2 + 255) / 256;
        const size_t last = (size_t)(h->d.T - 1) * h->ns;
        for (int64_t s = 0; s < S; ++s) {
            hipLaunchKernelGGL(qc_sweep_gen_kernel, dim3(gen_grid), dim3(256), 0, st, n2, m, p, (const double*)h->dG, p ? dtheta + s * p : nullptr,
                               (dscale && m) ? dscale + s * m : nullptr, h->dGs);
            QC_SIDE_HIP(h, g_swerr, qc_launch_rollout(P, h->d.T, dZ, dinit, h->dRout, h->dRE, h->dRQ, h->dRS, st));
            QC_SIDE_HIP(h, g_swerr, hipMemcpyAsync(h->dFin.p + (size_t)s * h->ns, h->dRout + last, (size_t)h->ns * 8, hipMemcpyDeviceToDevice, st));
        }
        F.ld = n; F.n_chunks = 0; F.src_stride = h->ns;
        src = h->dFin.p;
    }
    return finish_launch(h, F, S, src, dfinals, dfids, st);
}

extern "C" int qc_sweep_eval_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                                 double* dfinals, double* dfids, void* stream) {
    return qc_sweep_eval_launch(h, "qc_sweep_eval_dev", dZ, dinit, S, dtheta, dscale, dfinals, dfids, stream);
}

extern "C" int qc_sweep_eval(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale, double* finals,
                             double* fids) {
    const char* who = "qc_sweep_eval";
    int rc = eval_check(h, who, Z, init, S, theta, finals, fids);
    if (rc) return rc;
    const size_t nS = (size_t)S, m = (size_t)h->d.m, p = (size_t)h->d.n_pert, ns = (size_t)h->ns;
    qc_stage stage(h, &g_swerr);
    const double* dZ = stage.in(h->sZ, Z, (size_t)h->Zlen);
    const double* dinit = stage.in(h->sInit, init, ns);
    const double* dtheta = stage.in(h->sTheta, theta, nS * p);
    const double* dscale = stage.in(h->sScale, scale, nS * m);
    double* dfinals = stage.out(h->sFinals, finals, nS * ns);
    double* dfids = stage.out(h->sFids, fids, nS);
    if ((rc = stage.status())) return rc;
    if ((rc = qc_sweep_eval_launch(h, who, dZ, dinit, S, dtheta, dscale, dfinals, dfids, h->stream))) return rc;
    return stage.finish();
}
