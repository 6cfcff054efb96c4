/* qzstd_hip_internal.h — what the three HIP sources of the device layer share (not installed).  Everything here has hidden visibility:
 * the library's surface is the headers under include/ alone. */
#ifndef QZSTD_HIP_INTERNAL_H
#define QZSTD_HIP_INTERNAL_H

#include <hip/hip_runtime.h>

#pragma GCC visibility push(hidden)

/* the text qzstd_hip_last_error() returns: one thread-local buffer for the whole library (qzstd_runtime.hip); both return -1 */
int fail(const char *what, hipError_t e);
int fail_msg(const char *what);

#define QZ_CHECK(call, what)                       \
    do {                                           \
        hipError_t e_ = (call);                    \
        if (e_ != hipSuccess) return fail(what, e_); \
    } while (0)

/* the physical HIP device behind a device index of the C ABI, -1 when out of range; enumerates the devices on first use (qzstd_runtime.hip) */
int phys(int device);
extern int g_devReplicas; /* QZSTD_HIP_REPLICATE_DEVICES (test only): logical devices per physical one */

#define QZ_SET_DEVICE(device)                                            \
    do {                                                                 \
        const int pd_ = phys(device);                                    \
        if (pd_ < 0) return fail_msg("device index out of range");       \
        QZ_CHECK(hipSetDevice(pd_), "hipSetDevice");                     \
    } while (0)

/* qzstd_kernels.hip: the enumeration runs it once for every device (see there) */
int probe_lds_order(int device, int physDev);

/* qzstd_kernels.hip.  Around a free: hipFree / hipHostFree wait for every stream, which a resident kernel never lets finish */
struct SvcFreeze { SvcFreeze(); ~SvcFreeze(); };

#pragma GCC visibility pop

#endif
