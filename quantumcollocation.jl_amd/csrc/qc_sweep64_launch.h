// The launch of every kernel of the "mfma64-sweep" form (host side; included by the qc_sweep64*.hip files only): one workgroup of
// qc_sweep64::kThreads per item, `lds` bytes of dynamic LDS, `P` (SweepParams) as the kernel's first argument.  The LDS opt-in is made
// per launch: the attribute belongs to the (function, device) pair and the call is a host-side table update.  A launch that fails (the
// opt-in refused) is reported by hipGetLastError.  A macro, not a function: QC_SIDE_HIP returns from the launch function and puts the
// call as written, the kernel's name included, into the error text.
#pragma once

#include "qc_side.h"
#include "qc_sweep64_common.h"
#include "qc_sweep_internal.h"

#define QC_SWEEP64_LAUNCH(h, kernel, lds, P, st, ...)                                                                                   \
    do {                                                                                                                                  \
        QC_SIDE_HIP(h, *qc_sweep_err_slot(),                                                                                              \
                    hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   \
        hipLaunchKernelGGL(kernel, dim3((unsigned)(P).items), dim3(qc_sweep64::kThreads), lds, st, P, __VA_ARGS__);                      \
        QC_SIDE_HIP(h, *qc_sweep_err_slot(), hipGetLastError());                                                                          \
    } while (0)
