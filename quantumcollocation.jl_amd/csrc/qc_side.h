// Base of the side handles (qc_fidelity, qc_terms, qc_robust, qc_sweep: the objects beside the dynamics handle).  It owns what they
// all have -- device, stream, last error, and every device allocation -- so a family's file holds its descriptor checks, its kernels
// and its launches only; qc_stage below is the host-buffer side of an entry point (copies in, copies out, one synchronise).  Not part of
// the ABI: the handle structs are opaque there.
#pragma once

#include <memory>

#include "qc_internal.h"

// Scratch of doubles that follows the largest request so far (qc_side::grow): the device pointer and its capacity in elements.
struct qc_buf {
    double* p = nullptr;
    size_t cap = 0;
};

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
    hipError_t grow(qc_buf& b, size_t need) {
        if (need <= b.cap) return hipSuccess;
        if (b.p) {
            for (void*& q : owned) if (q == b.p) { q = owned.back(); owned.pop_back(); break; }
            hipError_t e = hipFree(b.p);
            b = qc_buf();
            if (e != hipSuccess) return e;
        }
        hipError_t e = alloc(&b.p, need);
        if (e == hipSuccess) b.cap = need;
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

// The host-buffer side of one call, built on the stack at the top of a host entry point (after its argument checks): it selects the
// handle's device, stages every argument in a buffer of the handle on h->stream, and finish() queues the copies back and synchronises once.
// The FIRST HIP error is kept and every later step is skipped, so a nullptr from in / out means "not asked for" and nothing else; the
// caller tests status() once before it launches and returns finish().  Nothing here allocates host memory.
struct qc_stage {
    static constexpr int kMaxOut = 8;
    qc_side* h;
    std::string* slot;              // the family's thread_local string
    qc_device_guard guard;
    hipError_t err;
    const char* what = "select the device";
    struct { double* host; const double* dev; size_t count; } back[kMaxOut];
    int n_back = 0;

    qc_stage(qc_side* h_, std::string* slot_) : h(h_), slot(slot_), guard(h_->device), err(guard.err) {}
    // `count` doubles of host memory, copied into `b`: the device pointer, or nullptr when there is nothing to copy
    double* in(qc_buf& b, const double* host, size_t count) {
        if (!host || !count || !room(b, count)) return nullptr;
        note(hipMemcpyAsync(b.p, host, count * 8, hipMemcpyHostToDevice, h->stream), "copy to the device");
        return b.p;
    }
    // `count` doubles of `b` that finish() copies to `host`: the device pointer, or nullptr when the output is not asked for
    double* out(qc_buf& b, double* host, size_t count) {
        if (!host || !count || !room(b, count)) return nullptr;
        if (n_back == kMaxOut) { note(hipErrorInvalidValue, "more outputs than qc_stage holds"); return nullptr; }
        back[n_back++] = {host, b.p, count};
        return b.p;
    }
    int status() { return err == hipSuccess ? QC_OK : qc_side_fail(h, slot, QC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(err)); }
    int finish() {
        for (int i = 0; i < n_back && err == hipSuccess; ++i)
            note(hipMemcpyAsync(back[i].host, back[i].dev, back[i].count * 8, hipMemcpyDeviceToHost, h->stream), "copy to the host");
        if (err == hipSuccess) note(hipStreamSynchronize(h->stream), "hipStreamSynchronize");
        return status();
    }

private:
    void note(hipError_t e, const char* w) { if (err == hipSuccess && e != hipSuccess) { err = e; what = w; } }
    bool room(qc_buf& b, size_t count) {
        if (err == hipSuccess) note(h->grow(b, count), "staging buffer");
        return err == hipSuccess;
    }
};

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
