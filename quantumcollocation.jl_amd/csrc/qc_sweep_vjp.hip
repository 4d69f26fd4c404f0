// Sweep pullbacks: the adjoint of the map (Z, init, theta, c) -> x_final[s] of the rollout sweep, for cotangents the CALLER chooses.
// With phi_s = <C_s, x_final[s]> and lambda_{T-1} = C_s in place of the fidelity's dphi/dx, every formula of qc_sweep_grad.hip (read
// its header first) holds unchanged:
//     dphi_s/da_{t,k} = c_k h <L(hG^T; lambda_{t+1} x_t^T), G_k>,   dphi_s/dh_t = <lambda_{t+1}, G x_{t+1}>,   lambda_t = E_t^T lambda_{t+1},
// and, the final state being linear in the initial one, dphi_s/dinit = lambda_0.  The backward walks (qc_sweep_grad_kernel<M, PAR>,
// qc_sweep32_grad_kernel<PAR>) read lambda from a buffer and do not know where it came from: they are launched as they are, through
// qc_sweep16_launch_walk / qc_sweep32_launch_walk.  What is new here is the seed and the plain sum.
//
// Launches of one call:
//   1. the forward chunk totals (qc_sweep_launch_totals: the kernel and the chunk rule of qc_sweep_eval);
//   2. qc_sweep_cot_seed_kernel ("mfma16-sweep": totals 16 x 16, ld = 16) or qc_sweep32_cot_seed_kernel ("mfma32-sweep": 32 x 32,
//      ld = 32), one workgroup per sample.  Up: the loops of qc_sweep_finish_kernel (x at every chunk end into dXs; the last x into
//      `finals` when asked for: the bits of qc_sweep_eval).  Down: lambda at the last chunk end = C_s as read, no arithmetic; then
//      lambda <- Q_c^T lambda for c = n_chunks-1 .. 1, stored at every chunk end into dLs.  With `grad_init` one more step than the
//      fidelity seeds take: lambda_0 = Q_0^T lambda_{end of chunk 0}.  (n_chunks = 1: that step is the only transposed product.)
//   3. the walk, when a derivative over the intervals or the parameters is asked for: flavour <M, false> without grad_theta /
//      grad_scale, <M, true> and qc_sweep_par_reduce_kernel with either (as qc_sweep_grad_launch chooses); the wide walk likewise
//      (qc_sweep32_grad_kernel<false> / <true>), its parameter flavour only on handles made with QC_SWEEP_WIDE_PARAMS.  "mfma64-sweep"
//      handles made with QC_SWEEP_WIDE_64_GRAD: qc_sweep64_cot_seed_kernel (ld = 64) and qc_sweep64_grad_kernel<false>; parameter cotangents
//      (its flavour <true>, then qc_sweep_par_reduce_kernel) only on handles that also set QC_SWEEP_WIDE_64_PARAMS.
//      With m = 0 and a fixed timestep there is nothing per interval: only <1, true> runs, and only for grad_theta.
//   4. qc_sweep_vjp_reduce_kernel: grad = sum_s dphi_s/dZ, the PLAIN sum in ascending s (qc_sweep_grad_reduce_kernel reads a missing
//      weight vector as 1/S each); +0.0 at every entry that is not a control or timestep of knots 0 .. T-2.
// No atomics, sums in a fixed order: repeated calls return the same bits, and no output's bits depend on which others were asked for.
//
// Scope: the gradient's without its two fidelity conditions (qc_sweep_vjp_scope below is qc_sweep_reverse_scope: the closed scope, or with
// reserved1[0] = QC_SWEEP_STORED_STATES the stored-state walk's, and then launch 3 is qc_sweep_open_launch_walk of qc_sweep_open_grad.hip or,
// on an "mfma32-sweep" handle made with QC_SWEEP_WIDE_STORED, qc_sweep32_open_launch_walk of qc_sweep32_open_grad.hip; on an "mfma64-sweep"
// handle made with QC_SWEEP_WIDE_64_GRAD | QC_SWEEP_WIDE_64_STORED, qc_sweep64_open_launch_walk of qc_sweep64_open_grad.hip).
#include <math.h>

#include <string>

#include "qc_sweep_internal.h"
#include "qc_sweep_seed.h"

namespace {

constexpr int kCotT = qc_sweep_seed::kSeedT;      // threads of the seed workgroup
constexpr int kSumT = 256;

struct CotParams {
    int n, ns, n_chunks;
};

struct SumParams {
    int zdim, off_a, off_dt, m, nd;
    long long T, Zlen, S;
};

// The body of both seed kernels, on the chains of qc_sweep_seed.h; LD is the leading dimension of the totals.
template <int LD>
__device__ __forceinline__ void cot_seed(const CotParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                         const double* __restrict__ cot, double* __restrict__ xs, double* __restrict__ ls,
                                         double* __restrict__ finals, double* __restrict__ ginit, double* sm) {
    const int tid = threadIdx.x, ns = F.ns;
    const long long s = blockIdx.x;
    qc_sweep_seed::Lds L(sm, ns);
    const double* __restrict__ Qs = tot + s * F.n_chunks * (long long)(LD * LD);
    double* __restrict__ lo = ls + s * F.n_chunks * (long long)ns;
    qc_sweep_seed::chain_up<LD>(L, F.n, ns, F.n_chunks, Qs, src, xs + s * F.n_chunks * (long long)ns);
    if (finals)
        for (int idx = tid; idx < ns; idx += kCotT) finals[s * ns + idx] = L.cur[idx];
    // lambda at the final knot: the caller's cotangent
    for (int idx = tid; idx < ns; idx += kCotT) {
        const double v = cot[s * ns + idx];
        L.cur[idx] = v;
        lo[(long long)(F.n_chunks - 1) * ns + idx] = v;
    }
    qc_sweep_seed::chain_down<LD>(L, F.n, ns, F.n_chunks, Qs, lo, ginit ? ginit + s * ns : nullptr);
}

__global__ __launch_bounds__(kCotT) void qc_sweep_cot_seed_kernel(const CotParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                                                  const double* __restrict__ cot, double* __restrict__ xs, double* __restrict__ ls,
                                                                  double* __restrict__ finals, double* __restrict__ ginit) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    cot_seed<16>(F, tot, src, cot, xs, ls, finals, ginit, sm);
}

__global__ __launch_bounds__(kCotT) void qc_sweep32_cot_seed_kernel(const CotParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                                                    const double* __restrict__ cot, double* __restrict__ xs, double* __restrict__ ls,
                                                                    double* __restrict__ finals, double* __restrict__ ginit) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    cot_seed<32>(F, tot, src, cot, xs, ls, finals, ginit, sm);
}

__global__ __launch_bounds__(kCotT) void qc_sweep64_cot_seed_kernel(const CotParams F, const double* __restrict__ tot, const double* __restrict__ src,
                                                                    const double* __restrict__ cot, double* __restrict__ xs, double* __restrict__ ls,
                                                                    double* __restrict__ finals, double* __restrict__ ginit) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    cot_seed<64>(F, tot, src, cot, xs, ls, finals, ginit, sm);
}

// grad[i] = sum_s dphi_s/dZ_i, the plain sum in ascending s, for the controls and timesteps of knots 0 .. T-2; +0.0 everywhere else
__global__ __launch_bounds__(kSumT) void qc_sweep_vjp_reduce_kernel(const SumParams R, const double* __restrict__ gs, double* __restrict__ grad) {
    const long long i = (long long)blockIdx.x * kSumT + threadIdx.x;
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
        for (long long s = 0; s < R.S; ++s) acc += p[s * stride];
    }
    grad[i] = acc;
}

const char* const kNoWidePar = "qc_sweep pullback: parameter cotangents are not served in the mfma32-sweep form";

// the argument checks both entry points share, in the order of the header's table
int vjp_check(qc_sweep* h, const char* who, const void* Z, const void* init, int64_t S, const void* theta, const void* cot, bool any_out,
              bool g_theta, bool g_scale) {
    int rc = qc_sweep_check(h, who, &qc_sweep::vjp_ok, "qc_sweep pullback: ", &qc_sweep::vjp_why, Z, init, cot ? nullptr : "cot", S, theta);
    if (rc) return rc;
    const std::string pre = std::string(who) + ": ";
    if (!any_out) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "every output is NULL");
    if (g_theta && h->d.n_pert == 0) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "grad_theta is given but the handle has no perturbations (n_pert = 0)");
    if (g_scale && h->d.m == 0) return qc_sweep_fail(h, QC_ERR_INVALID, pre + "grad_scale is given but the handle has no drives (m = 0)");
    if ((g_theta || g_scale) && h->mfma32 && !h->wide_par) return qc_sweep_fail(h, QC_ERR_UNSUPPORTED, kNoWidePar);
    if ((g_theta || g_scale) && h->wide64_grad && !h->wide64_par)
        return qc_sweep_fail(h, QC_ERR_UNSUPPORTED, "qc_sweep pullback: parameter cotangents are not served in the mfma64-sweep form (2N = " + std::to_string(h->n) + ")");
    return QC_OK;
}

}  // namespace

bool qc_sweep_vjp_scope(const qc_sweep_desc* d, std::string* why) { return qc_sweep_reverse_scope(d, why); }

extern "C" int qc_sweep_desc_vjp_supported(const qc_sweep_desc* d, int32_t* supported) {
    int rc = qc_sweep_validate_desc(d);
    if (rc) return rc;
    if (!supported) return qc_sweep_fail(nullptr, QC_ERR_INVALID, "qc_sweep_desc_vjp_supported: supported is NULL");
    std::string why;
    const bool ok = qc_sweep_vjp_scope(d, &why);
    *supported = ok ? 1 : 0;
    if (!ok) (void)qc_sweep_fail(nullptr, QC_ERR_UNSUPPORTED, "qc_sweep pullback: " + why);
    return QC_OK;
}

// grad = the plain sum over the samples of the per-interval buffer gs (S x (T-1) x nd), for the pullback below and the Hessian product
// of qc_sweep_hvp.hip
void qc_sweep_launch_plain_sum(qc_sweep* h, int64_t S, const double* gs, double* dgrad, hipStream_t st) {
    SumParams R;
    R.zdim = h->d.zdim; R.off_a = h->d.off_a; R.off_dt = h->d.off_dt; R.m = h->d.m; R.nd = h->d.m + (h->d.off_dt >= 0 ? 1 : 0);
    R.T = h->d.T; R.Zlen = h->Zlen; R.S = S;
    hipLaunchKernelGGL(qc_sweep_vjp_reduce_kernel, dim3((unsigned)((h->Zlen + kSumT - 1) / kSumT)), dim3(kSumT), 0, st, R, gs, dgrad);
}

static int qc_sweep_vjp_launch(qc_sweep* h, const char* who, const double* dZ, const double* dinit, int64_t S, const double* dtheta,
                               const double* dscale, const double* dcot, double* dfinals, double* dgrad, double* dgrad_samples, double* dgrad_init,
                               double* dgrad_theta, double* dgrad_scale, void* stream) {
    const bool any_out = dfinals || dgrad || dgrad_samples || dgrad_init || dgrad_theta || dgrad_scale;
    int rc = vjp_check(h, who, dZ, dinit, S, dtheta, dcot, any_out, dgrad_theta != nullptr, dgrad_scale != nullptr);
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
    const bool want_par = dgrad_theta || dgrad_scale;
    const bool want_grad = (dgrad || dgrad_samples) && nd > 0;
    double* gsamp = dgrad_samples;
    if (want_grad && !gsamp) {
        QC_SIDE_HIP(h, slot, h->grow(h->dGsamp, (size_t)S * n_int * nd));
        gsamp = h->dGsamp.p;
    }
    if (want_par) QC_SIDE_HIP(h, slot, h->grow(h->dPart, (size_t)S * n_chunks * (p + m)));
    if (h->stored && (want_grad || want_par)) QC_SIDE_HIP(h, slot, h->grow(h->dXall, (size_t)S * (size_t)n_int * h->ns));
    CotParams F;
    F.n = h->n; F.ns = h->ns; F.n_chunks = (int)n_chunks;
    // at most 16 state columns: 16 KiB; "mfma64-sweep": at most 32, 64 KiB, hence the opt-in
    const size_t lds = qc_sweep_seed::lds_bytes(h->ns, h->mfma64 ? 64 : h->mfma32 ? 32 : 16);
    const auto seed = h->mfma64 ? qc_sweep64_cot_seed_kernel : h->mfma32 ? qc_sweep32_cot_seed_kernel : qc_sweep_cot_seed_kernel;
    if (h->mfma64)
        QC_SIDE_HIP(h, slot, hipFuncSetAttribute(reinterpret_cast<const void*>(&qc_sweep64_cot_seed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(seed, dim3((unsigned)S), dim3(kCotT), lds, st, F, (const double*)h->dTot.p, dinit, dcot, h->dXs.p, h->dLs.p, dfinals,
                       dgrad_init);
    if (h->mfma64 && h->stored && h->wide64_stored) {      // the 4 x 4-tile stored-state walk of qc_sweep64_open_grad.hip behind the same seed
        if ((want_grad || want_par) &&      // want_par: only on handles with QC_SWEEP_WIDE_64_PARAMS (vjp_check refuses the others)
            (rc = qc_sweep64_open_launch_walk(h, dZ, dinit, S, dtheta, dscale, chunk, n_chunks, want_grad ? gsamp : nullptr, want_par, h->dPart.p, st)))
            return rc;
        if (want_par) qc_sweep_launch_par_reduce(h, S, n_chunks, dgrad_theta, dgrad_scale, st);
    } else if (h->mfma64 && h->wide64_grad) {      // the 4 x 4-tile walk of qc_sweep64_grad.hip behind the seed at ld = 64
        if ((want_grad || want_par) &&      // want_par: only on handles with QC_SWEEP_WIDE_64_PARAMS (vjp_check refuses the others)
            (rc = qc_sweep64_launch_walk(h, dZ, S, dtheta, dscale, chunk, n_chunks, want_grad ? gsamp : nullptr, want_par, h->dPart.p, st)))
            return rc;
        if (want_par) qc_sweep_launch_par_reduce(h, S, n_chunks, dgrad_theta, dgrad_scale, st);
    } else if (h->stored) {      // reserved1[0] = QC_SWEEP_STORED_STATES: the walk of qc_sweep_open_grad.hip behind the same seed
        if (want_grad || want_par)      // (an "mfma32-sweep" handle is in scope only with QC_SWEEP_WIDE_STORED: qc_sweep32_open_grad.hip)
            (h->mfma32 ? qc_sweep32_open_launch_walk : qc_sweep_open_launch_walk)(h, dZ, dinit, S, dtheta, dscale, chunk, n_chunks,
                                                                                 want_grad ? gsamp : nullptr, want_par, dgrad_theta, dgrad_scale, st);
    } else if (h->mfma32) {
        if (want_grad || want_par)
            qc_sweep32_launch_walk(h, dZ, S, dtheta, dscale, chunk, n_chunks, want_grad ? gsamp : nullptr, want_par, dgrad_theta, dgrad_scale, st);
    } else if (want_grad || want_par)
        qc_sweep16_launch_walk(h, dZ, S, dtheta, dscale, chunk, n_chunks, want_grad ? gsamp : nullptr, want_par, dgrad_theta, dgrad_scale, st);
    if (dgrad) qc_sweep_launch_plain_sum(h, S, gsamp, dgrad, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qc_sweep_fail(h, QC_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return QC_OK;
}

extern "C" int qc_sweep_vjp_dev(qc_sweep* h, const double* dZ, const double* dinit, int64_t S, const double* dtheta, const double* dscale,
                                const double* dcot, double* dfinals, double* dgrad, double* dgrad_samples, double* dgrad_init,
                                double* dgrad_theta, double* dgrad_scale, void* stream) {
    return qc_sweep_vjp_launch(h, "qc_sweep_vjp_dev", dZ, dinit, S, dtheta, dscale, dcot, dfinals, dgrad, dgrad_samples, dgrad_init, dgrad_theta,
                               dgrad_scale, stream);
}

// The host-buffer entry point: stage, launch on the handle's stream, copy back, synchronise.
extern "C" int qc_sweep_vjp(qc_sweep* h, const double* Z, const double* init, int64_t S, const double* theta, const double* scale,
                            const double* cot, double* finals, double* grad, double* grad_samples, double* grad_init, double* grad_theta,
                            double* grad_scale) {
    const char* who = "qc_sweep_vjp";
    const bool any_out = finals || grad || grad_samples || grad_init || grad_theta || grad_scale;
    int rc = vjp_check(h, who, Z, init, S, theta, cot, any_out, grad_theta != nullptr, grad_scale != nullptr);
    if (rc) return rc;
    const size_t nS = (size_t)S, m = (size_t)h->d.m, p = (size_t)h->d.n_pert, n_fin = nS * (size_t)h->ns, Zlen = (size_t)h->Zlen;
    const size_t n_samp = nS * (size_t)(h->d.T - 1) * (m + (h->d.off_dt >= 0 ? 1 : 0));
    qc_stage stage(h, qc_sweep_err_slot());
    const double* dZ = stage.in(h->sZ, Z, Zlen);
    const double* dinit = stage.in(h->sInit, init, (size_t)h->ns);
    const double* dtheta = stage.in(h->sTheta, theta, nS * p);
    const double* dscale = stage.in(h->sScale, scale, nS * m);
    const double* dcot = stage.in(h->sCot, cot, n_fin);
    double* dfinals = stage.out(h->sFinals, finals, n_fin);
    double* dgrad = stage.out(h->sGrad, grad, Zlen);
    double* dsamp = stage.out(h->sGradS, grad_samples, n_samp);
    double* dginit = stage.out(h->sGinit, grad_init, n_fin);
    double* dgth = stage.out(h->sGth, grad_theta, nS * p);
    double* dgsc = stage.out(h->sGsc, grad_scale, nS * m);
    if ((rc = stage.status())) return rc;
    if ((rc = qc_sweep_vjp_launch(h, who, dZ, dinit, S, dtheta, dscale, dcot, dfinals, dgrad, dsamp, dginit, dgth, dgsc, h->stream))) return rc;
    return stage.finish();
}
