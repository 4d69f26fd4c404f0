// Base of the side handles (qc_fidelity, qc_terms, qc_robust, qc_sweep: the objects beside the dynamics handle).  It owns what they
// all have -- device, stream, last error, and every device allocation -- so a family's file holds its descriptor checks, its kernels
// and its launches only.  Not part of the ABI: the handle structs are opaque there.
#pragma once

#include <memory>

#include "qc_internal.h"

struct qc_side {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::vector<void*> owned;      // every live device allocation of the handle: alloc / grow are the only way to get one

    // `count` elements of T on the device (the caller has selected it), filled from `src` when given.
    template <class T>
    hipError_t alloc(T** p, size_t count, const T* src = nullptr) {
        hipError_t e = hipMalloc((void**)p, count * sizeof(T));
        if (e != hipSuccess) { *p = nullptr; return e; }
        if (*p) owned.push_back(*p);
        return src ? hipMemcpy(*p, src, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
    }
    // Scratch that follows the largest request so far: freed, then allocated afresh (the contents are never carried over).
    template <class T>
    hipError_t grow(T** p, size_t* cap, size_t need) {
        if (need <= *cap) return hipSuccess;
        if (*p) {
            for (void*& q : owned) if (q == *p) { q = owned.back(); owned.pop_back(); break; }
            hipError_t e = hipFree(*p);
            *p = nullptr;
            *cap = 0;
            if (e != hipSuccess) return e;
        }
        hipError_t e = alloc(p, need);
        if (e == hipSuccess) *cap = need;
        return e;
    }
    hipError_t open_stream() { return hipStreamCreateWithFlags(&stream, hipStreamNonBlocking); }
    // Waits for the stream, destroys it and frees every allocation; the caller's current device is left as it was.
    void release_device() {
        qc_device_guard guard(device);
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); stream = nullptr; }
        for (void* p : owned) (void)hipFree(p);
        owned.clear();
    }
};

// What qc_*_create holds its handle in until it hands it out: any early return releases the device state and deletes the handle.
struct qc_side_drop {
    template <class H>
    void operator()(H* h) const { h->release_device(); delete h; }
};
template <class H>
using qc_side_new = std::unique_ptr<H, qc_side_drop>;

// Records `msg` in the handle (when there is one) and in the family's thread-local slot (what qc_X_last_error(NULL) returns).
inline int qc_side_fail(qc_side* h, std::string* slot, int code, const std::string& msg) {
    if (h) h->err = msg;
    *slot = msg;
    return code;
}

// `h`: a qc_side* (null inside create: the handle does not exist for the caller yet); `slot`: the family's thread_local string.
#define QC_SIDE_HIP(h, slot, call)                                                                                        \
    do {                                                                                                                  \
        hipError_t e_ = (call);                                                                                           \
        if (e_ != hipSuccess) return qc_side_fail(h, &(slot), QC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline int qc_side_check_device(int device, const char* who, std::string* slot) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return qc_side_fail(nullptr, slot, QC_ERR_NO_DEVICE, std::string(who) + ": no HIP device visible");
    if (device < 0 || device >= ndev) return qc_side_fail(nullptr, slot, QC_ERR_NO_DEVICE, std::string(who) + ": device ordinal out of range");
    return QC_OK;
}

inline int qc_isqrt_exact(int v) {      // the root of a perfect square, else -1
    int r = 0;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r * r == v ? r : -1;
}

// The constant vectors of a fidelity: the complex overlap of the state x (iso-vec) with the goal is t = g_r.x + i g_i.x.
//   QC_FID_UNITARY  x = iso-vec of U (2N^2), goal_iso likewise: t = tr(G_sub' U_sub) over `subspace` (n_sub levels; NULL: all N)
//   QC_FID_KET      x = [Re psi; Im psi] (2N), goal_iso likewise: t = <g|psi>
//   QC_FID_DENSITY  x = [vec(Re rho); vec(Im rho)] (2N, N = levels^2), goal_iso = the goal KET [Re; Im] (2 levels): t = g' rho g
//                   over the Hermitian part of rho (g_i = 0)
// Fills g_r, g_i (2N^2 resp. 2N entries) and returns the normaliser n of F (n_sub, or 1 for ket and density).  Host arithmetic only;
// defined in qc_fidelity.hip.  The arguments are the caller's to check, and the callers differ: qc_fidelity accepts a subspace
// that names a level twice (the level then counts in n as often as it is named), qc_robust and qc_sweep refuse one.
int qc_fidelity_goal(int kind, int N, const double* goal_iso, const int32_t* subspace, int n_sub, double* g_r, double* g_i);
