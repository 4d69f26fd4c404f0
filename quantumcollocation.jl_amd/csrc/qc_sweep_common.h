// Device code that every sweep kernel shares, whatever its tile form ("mfma16-sweep": qc_sweep16_common.h, "mfma32-sweep":
// qc_sweep32_common.h): the series' degree and threshold, the 1 / k! table, the DPP move, the fixed-order wave sum and the scalar tail of
// the squaring rule, and the work item of the (sample, chunk) kernels (wave_item, chunk_range).  The closed walks reverse the forward step,
// and the stored states match the stored-state walks, only if every kernel of the family chooses the same number of squarings from the same
// norm: the rule is here once.
#pragma once
#include <math.h>

#include "qc_mfma_common.h"

namespace qc_sweep_common {

using namespace qc_mfma;

constexpr int kDeg = 8;             // as qc_mfma_exp.hip: ||Y||_1 <= 1/8, degree 8, truncation (1/8)^9 / 9! = 4e-14
constexpr double kTh = 0.125;
constexpr int kWaves = 4;           // (sample, chunk) items per workgroup: one wave each, the waves never synchronise

// 1 / k!, k = 0 .. 8, correctly rounded constants (a __constant__ table is private to the translation unit that includes this)
static __constant__ const double kInvFact[kDeg + 1] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0};

template <int CTRL>
__device__ __forceinline__ double dpp(double x) {
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// v summed over each row of 16 lanes, by DPP rotations: every lane of a row holds the row's sum
__device__ __forceinline__ double row_sum(double v) {
    v += dpp<0x128>(v);
    v += dpp<0x124>(v);
    v += dpp<0x122>(v);
    v += dpp<0x121>(v);
    return v;
}

// the sum over the 64 lanes in a fixed order, wave-uniform: row sums, then (row 0 + row 1) + (row 2 + row 3)
__device__ __forceinline__ double wave_sum(double v) {
    v = row_sum(v);
    return (bcast_lane(v, 0) + bcast_lane(v, 16)) + (bcast_lane(v, 32) + bcast_lane(v, 48));
}

// The scalar tail of the squaring rule.  Each form sums the columns of |h G| its own way (row_sum over the lanes' shares: rows of 16
// lanes share a column), keeps the largest sum in `best` and records in `bad` a sum that is not finite; from there the smallest sq with
// best / 2^sq <= 1/8, at most 60, 0 when the norm is not finite; wave-uniform.
__device__ __forceinline__ int squarings_of_norm(double best, bool bad) {
    int sq = 0;
    if (!bad && best > kTh) {
        int e;
        (void)frexp(best / kTh, &e);
        sq = e;
        if (ldexp(kTh, e - 1) >= best) sq = e - 1;
        sq = sq < 0 ? 0 : (sq > 60 ? 60 : sq);
    }
    return __builtin_amdgcn_readfirstlane(sq);
}

// The work item of every kernel that runs one wavefront per (sample, chunk of consecutive intervals): wave wq of a workgroup of `waves`
// takes item blockIdx.x * waves + wq = s * n_chunks + c and walks the intervals t0 .. t1-1 of sample s.  Two steps, by value: a wave whose
// item is not below P.items returns between them, so the launch parameters of the second are still read behind that branch.  The wave's
// LDS slice, scr_all + wq * (doubles a wave), is formed in the kernel: handed through a function the array loses its address space too late.
struct WaveItem { int lane, wq; long long item; };
struct ChunkRange { long long s; int c, t0, t1; };

__device__ __forceinline__ WaveItem wave_item(int waves) {
    WaveItem w;
    w.lane = threadIdx.x & 63;
    w.wq = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    w.item = (long long)blockIdx.x * waves + w.wq;
    return w;
}

__device__ __forceinline__ ChunkRange chunk_range(long long item, int n_chunks, int chunk, int n_int) {
    ChunkRange r;
    r.s = item / n_chunks;
    r.c = (int)(item - r.s * n_chunks);
    r.t0 = r.c * chunk;
    r.t1 = min(n_int, r.t0 + chunk);
    return r;
}

}  // namespace qc_sweep_common
