// The two chains of the seed kernels (qc_sweep_seed_kernel / qc_sweep32_seed_kernel of qc_sweep_grad.hip, qc_sweep_cot_seed_kernel /
// qc_sweep32_cot_seed_kernel of qc_sweep_vjp.hip): one workgroup of kSeedT threads per sample, LD the leading dimension of the chunk
// totals (16: "mfma16-sweep", 32: "mfma32-sweep").  The loops are those of qc_sweep_finish_kernel (qc_sweep.hip), thread for thread and
// fma for fma, so the states carry the bits of qc_sweep_eval.  Device code only.
#pragma once

namespace qc_sweep_seed {

constexpr int kSeedT = 256;       // the thread count of qc_sweep_finish_kernel (same sums, same bits)

// dynamic LDS of a seed workgroup: cur, nxt (ns doubles each) and one total (LD x LD)
constexpr size_t lds_bytes(int ns, int ld) { return ((size_t)2 * ns + (size_t)ld * ld) * 8; }

struct Lds {
    double *cur, *nxt, *Q;
    __device__ Lds(double* sm, int ns) : cur(sm), nxt(sm + ns), Q(sm + 2 * ns) {}
    __device__ void swap() { double* tmp = cur; cur = nxt; nxt = tmp; }
};

// Up: x = Q_c ... Q_0 src in ascending order, x stored at every chunk end into xo[c]; leaves the final state in L.cur, visible to the
// whole workgroup.  Qs: the sample's n_chunks totals.
template <int LD>
__device__ __forceinline__ void chain_up(Lds& L, int n, int ns, int n_chunks, const double* __restrict__ Qs, const double* __restrict__ src,
                                         double* __restrict__ xo) {
    constexpr int ld = LD, l2 = LD * LD;
    const int tid = threadIdx.x;
    for (int idx = tid; idx < ns; idx += kSeedT) L.cur[idx] = src[idx];
    for (int c = 0; c < n_chunks; ++c) {
        __syncthreads();
        for (int idx = tid; idx < l2; idx += kSeedT) L.Q[idx] = Qs[(long long)c * l2 + idx];
        __syncthreads();
        for (int idx = tid; idx < ns; idx += kSeedT) {
            const int r = idx % n, col = idx / n;
            double acc = 0.0;
            for (int q = 0; q < n; ++q) acc = fma(L.Q[r + ld * q], L.cur[q + n * col], acc);
            L.nxt[idx] = acc;
            xo[(long long)c * ns + idx] = acc;
        }
        L.swap();
    }
    __syncthreads();
}

// Down: from lambda at the last chunk end (in L.cur, every thread's own entries, already stored at lo[n_chunks - 1]),
// lambda <- Q_c^T lambda for c = n_chunks-1 .. 1, stored at every chunk end into lo[c - 1].  With `ginit` (the sample's, or NULL) one
// more step: lambda_0 = Q_0^T lambda_{end of chunk 0}.
template <int LD>
__device__ __forceinline__ void chain_down(Lds& L, int n, int ns, int n_chunks, const double* __restrict__ Qs, double* __restrict__ lo,
                                           double* __restrict__ ginit) {
    constexpr int ld = LD, l2 = LD * LD;
    const int tid = threadIdx.x;
    for (int c = n_chunks - 1; c >= (ginit ? 0 : 1); --c) {
        __syncthreads();
        for (int idx = tid; idx < l2; idx += kSeedT) L.Q[idx] = Qs[(long long)c * l2 + idx];
        __syncthreads();
        for (int idx = tid; idx < ns; idx += kSeedT) {
            const int r = idx % n, col = idx / n;
            double acc = 0.0;
            for (int q = 0; q < n; ++q) acc = fma(L.Q[q + ld * r], L.cur[q + n * col], acc);
            L.nxt[idx] = acc;
            if (c > 0) lo[(long long)(c - 1) * ns + idx] = acc;
            else ginit[idx] = acc;
        }
        L.swap();
    }
}

}  // namespace qc_sweep_seed
