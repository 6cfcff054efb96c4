/*
 * qzstd_runtime.hip — the device layer's runtime shim, the part of include/qzstd_hip.h and include/qzstd_hip_device.h that is a thin C ABI
 * over the HIP runtime: device enumeration and the logical-to-physical map, device / pinned / NUMA-placed memory, streams, copies, the
 * memset, events, the pointer query, the staging-copy kernel, and the library's error text.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <sched.h>
#include <time.h>
#include <sys/syscall.h>
#include <unistd.h>

#include "qzstd_hip.h"
#include "qzstd_hip_device.h"
#include "qzstd_hip_internal.h"

namespace {
thread_local char g_err[256] = "";
}

int fail(const char *what, hipError_t e)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -1;
}
int fail_msg(const char *what)
{
    snprintf(g_err, sizeof(g_err), "%s", what);
    return -1;
}

/* The library carries one code object (gfx950).  Only devices that can run it are counted, and the `device` argument
 * of every entry point indexes that filtered list (reference: instance discovery keeps only usable DC instances,
 * /root/reference/src/qatseqprod.c:529-600). */
static std::once_flag g_devOnce;
static int g_devCount = -1;
static int g_devMap[64];
int g_devReplicas = 1;

static void probe_devices()
{
    int n = 0;
    /* The runtime folds its streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and launches of different streams that share a queue run
     * one after the other.  Announcements no longer depend on it (they go out as a few large launches on the announcement batcher's own
     * streams, host/qatseqprod.c); the per-block paths' slot streams still do.  The variable is read when the runtime starts, so it only takes
     * effect when this is the process's first HIP call; a value the environment already carries is left alone.  QZSTD_HIP_HW_QUEUES=0 leaves
     * the runtime's default. */
    {
        const char *q = getenv("QZSTD_HIP_HW_QUEUES");
        const int want = q && *q ? atoi(q) : 16;
        if (want > 0 && want <= 64) {
            char buf[16];
            snprintf(buf, sizeof(buf), "%d", want);
            (void)setenv("GPU_MAX_HW_QUEUES", buf, 0);
        }
    }
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { fail("hipGetDeviceCount", e); (void)hipGetLastError(); g_devCount = -1; return; }
    g_devCount = 0;
    for (int d = 0; d < n && g_devCount < 64; d++) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) continue; /* no code object for it */
        g_devMap[g_devCount++] = d;
    }
    if (g_devCount == 0) fail_msg("no gfx950 device among the visible HIP devices");
    /* TEST ONLY — QZSTD_HIP_REPLICATE_DEVICES=k lists every physical device k times: the library then sees k x n LOGICAL devices, each with
     * its own streams, batches, pinned buffers and resident service, and the host's split of an announcement into per-GPU ranges, its state
     * placement and QZSTD_deviceStats run over several devices on a box that has one GPU (round-5 verdict: the N > 1 path had only ever run
     * against tests/mock/mock_hip.c).  Replicas share the physical GPU's CUs and LDS: no speed to be had, and resident services of two replicas
     * compete for the same CUs (the tests give each service half the CUs: QZSTD_HIP_SERVICE_WORKERS). */
    {
        const char *r = getenv("QZSTD_HIP_REPLICATE_DEVICES");
        const int k = r && *r ? atoi(r) : 1;
        const int n0 = g_devCount;
        for (int c = 1; c < k && c < 64; c++)
            for (int d = 0; d < n0 && g_devCount < 64; d++) g_devMap[g_devCount++] = g_devMap[d];
        if (n0 > 0 && g_devCount > n0) g_devReplicas = g_devCount / n0;
    }
    for (int d = 0; d < g_devCount; d++) (void)probe_lds_order(d, g_devMap[d]); /* now: nothing is resident yet (see probe_lds_order) */
}

int phys(int device)
{
    std::call_once(g_devOnce, probe_devices);
    return device >= 0 && device < g_devCount ? g_devMap[device] : -1;
}

extern "C" {

const char *qzstd_hip_last_error(void) { return g_err; }

int qzstd_hip_device_count(void)
{
    std::call_once(g_devOnce, probe_devices);
    return g_devCount;
}

int qzstd_hip_device_name(int device, char *buf, size_t bufLen)
{
    hipDeviceProp_t prop;
    if (phys(device) < 0) return fail_msg("device index out of range");
    QZ_CHECK(hipGetDeviceProperties(&prop, phys(device)), "hipGetDeviceProperties");
    if (buf && bufLen) snprintf(buf, bufLen, "%s (%s, %d CUs, %zu KiB LDS/WG)", prop.name, prop.gcnArchName,
                                prop.multiProcessorCount, prop.sharedMemPerBlock >> 10);
    return 0;
}

void *qzstd_hip_malloc(int device, size_t bytes)
{
    void *p = nullptr;
    if (phys(device) < 0 || hipSetDevice(phys(device)) != hipSuccess) return nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) { fail("hipMalloc", e); return nullptr; }
    return p;
}

void qzstd_hip_free(int device, void *dptr)
{
    if (!dptr) return;
    SvcFreeze frozen; /* hipFree waits for every stream of the device: the resident service has to leave first */
    if (phys(device) >= 0 && hipSetDevice(phys(device)) == hipSuccess) (void)hipFree(dptr);
}

void *qzstd_hip_host_alloc(size_t bytes)
{
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocPortable | hipHostMallocMapped);
    if (e != hipSuccess) { fail("hipHostMalloc", e); return nullptr; }
    return p;
}

void *qzstd_hip_host_device_ptr(void *hptr)
{
    void *d = nullptr;
    if (!hptr) return nullptr;
    hipError_t e = hipHostGetDevicePointer(&d, hptr, 0);
    if (e != hipSuccess) { fail("hipHostGetDevicePointer", e); return nullptr; }
    return d;
}

void *qzstd_hip_host_alloc_coherent(size_t bytes)
{
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) { fail("hipHostMalloc(coherent)", e); return nullptr; }
    return p;
}

/* The GPU's host NUMA node: the runtime's attribute first, the PCI function's sysfs entry second */
int qzstd_hip_device_numa_node(int device)
{
    const int pd = phys(device);
    if (pd < 0) return -1;
    int node = -1;
    if (hipDeviceGetAttribute(&node, hipDeviceAttributeHostNumaId, pd) == hipSuccess && node >= 0) return node;
    (void)hipGetLastError();
    char bus[32] = "", path[96];
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), pd) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char *c = bus; *c; c++) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a'); /* sysfs spells the address in lower case */
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

/* Pinned host memory on a NUMA node: hipHostMallocNumaUser makes the runtime allocate under the CALLING THREAD's memory policy, so
 * the policy is set to "prefer `node`" around the call (raw system calls: no libnuma in the image) and put back afterwards.  A
 * process that may not set a policy (seccomp, containers without CAP_SYS_NICE for other nodes) gets the memory anyway, unplaced. */
void *qzstd_hip_host_alloc_on_node(size_t bytes, int node, int coherent)
{
    const unsigned flags = hipHostMallocPortable | hipHostMallocMapped | (coherent ? hipHostMallocCoherent : 0u);
    void *p = nullptr;
    if (node >= 0 && node < 1024) {
        unsigned long want[16] = { 0 }, old[16] = { 0 };
        int oldMode = 0;
        want[node / (8 * sizeof(unsigned long))] = 1ul << (node % (8 * sizeof(unsigned long)));
        const bool got = syscall(SYS_get_mempolicy, &oldMode, old, (unsigned long)(8 * sizeof(old)), nullptr, 0ul) == 0;
        if (got && syscall(SYS_set_mempolicy, 1 /* MPOL_PREFERRED */, want, (unsigned long)(8 * sizeof(want))) == 0) {
            const hipError_t e = hipHostMalloc(&p, bytes, flags | hipHostMallocNumaUser);
            (void)syscall(SYS_set_mempolicy, oldMode, oldMode == 0 /* MPOL_DEFAULT takes no mask */ ? nullptr : old,
                          oldMode == 0 ? 0ul : (unsigned long)(8 * sizeof(old)));
            if (e == hipSuccess) return p;
            (void)hipGetLastError();
            p = nullptr;
        }
    }
    const hipError_t e = hipHostMalloc(&p, bytes, flags);
    if (e != hipSuccess) { fail(coherent ? "hipHostMalloc(coherent)" : "hipHostMalloc", e); return nullptr; }
    return p;
}

int qzstd_hip_host_node_of(const void *hptr)
{
    int node = -1;
    if (!hptr) return -1;
    if (syscall(SYS_get_mempolicy, &node, nullptr, 0ul, hptr, 3ul /* MPOL_F_NODE | MPOL_F_ADDR */) != 0) return -1;
    return node;
}

void qzstd_hip_host_free(void *hptr)
{
    if (!hptr) return;
    SvcFreeze frozen; /* hipHostFree waits for the device's streams too */
    (void)hipHostFree(hptr);
}

void *qzstd_hip_stream_create(int device)
{
    hipStream_t s = nullptr;
    if (phys(device) < 0 || hipSetDevice(phys(device)) != hipSuccess) return nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) { fail("hipStreamCreate", e); return nullptr; }
    return (void *)s;
}

void qzstd_hip_stream_destroy(int device, void *stream)
{
    if (stream && phys(device) >= 0 && hipSetDevice(phys(device)) == hipSuccess) (void)hipStreamDestroy((hipStream_t)stream);
}

int qzstd_hip_stream_sync(int device, void *stream)
{
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
    return 0;
}

int qzstd_hip_stream_query(int device, void *stream)
{
    QZ_SET_DEVICE(device);
    hipError_t e = hipStreamQuery((hipStream_t)stream);
    if (e == hipSuccess) return 0;
    if (e == hipErrorNotReady) return 1;
    return fail("hipStreamQuery", e);
}

int qzstd_hip_stream_wait(int device, void *stream, unsigned timeoutMs)
{
    QZ_SET_DEVICE(device);
    /* poll instead of hipStreamSynchronize: a wedged kernel must not take the calling thread with it.  Busy polls for
     * the first QZSTD_HIP_SPIN_US microseconds (default 50), then naps between polls so
     * that a waiting caller does not burn a core other callers could entropy-code on (QZSTD_HIP_NAP_US, default 20) */
    static const long long spinUs = [] { const char *v = getenv("QZSTD_HIP_SPIN_US"); return v ? atoll(v) : 50ll; }();
    static const long napNs = [] { const char *v = getenv("QZSTD_HIP_NAP_US"); return (v ? atol(v) : 20l) * 1000l; }();
    struct timespec t0, t;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (;;) {
        const hipError_t e = hipStreamQuery((hipStream_t)stream);
        if (e == hipSuccess) return 0;
        if (e != hipErrorNotReady) return fail("hipStreamQuery", e);
        clock_gettime(CLOCK_MONOTONIC, &t);
        const long long us = (long long)(t.tv_sec - t0.tv_sec) * 1000000ll + (t.tv_nsec - t0.tv_nsec) / 1000;
        if (us >= (long long)timeoutMs * 1000ll) {
            snprintf(g_err, sizeof(g_err), "stream still busy after %u ms", timeoutMs);
            return 1;
        }
        if (us < spinUs) continue;
        if (napNs <= 0) sched_yield();
        else { const struct timespec nap = { 0, us < 20000 ? napNs : 200000l }; nanosleep(&nap, nullptr); }
    }
}

int qzstd_hip_memcpy_h2d(int device, void *stream, void *dst, const void *src, size_t bytes)
{
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream), "hipMemcpyAsync H2D");
    return 0;
}

/* pinned host memory -> device memory by a KERNEL on the stream: 16 bytes per lane and step, every wave streaming its own 16 KiB stripes.
 * For the staging copies of announcements (host/qatseqprod.c, qzLaunchPart): hipMemcpyAsync holds the calling thread for 0.8-1.1 ms per 4 MiB
 * when 16 threads announce (the runtime's copy path and its locks); a launch costs 10-30 us, and the copy then runs at the bus's rate in front
 * of the match-finder on the same stream.  src_dev = the DEVICE address of the pinned buffer (qzstd_hip_host_device_ptr); bytes a multiple
 * of 16, both addresses 16-byte aligned. */
}
namespace {
__global__ __launch_bounds__(256) void qzstd_copy_in_kernel(uint4 *__restrict__ dst, const uint4 *__restrict__ src, uint32_t n16)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n16; i += gridDim.x * 256u) dst[i] = src[i];
}
}
extern "C" {
int qzstd_hip_copy_in(int device, void *stream, void *dst, const void *src_dev, size_t bytes)
{
    if (bytes == 0) return 0;
    if (!dst || !src_dev || (bytes & 15u) || ((uintptr_t)dst & 15u) || ((uintptr_t)src_dev & 15u) || bytes > ((size_t)1 << 34))
        return fail_msg("qzstd_hip_copy_in: null, unaligned or oversized");
    QZ_SET_DEVICE(device);
    const uint32_t n16 = (uint32_t)(bytes >> 4);
    uint32_t groups = (n16 + 1023u) / 1024u; /* four steps per lane */
    if (groups > 1024u) groups = 1024u;
    hipLaunchKernelGGL(qzstd_copy_in_kernel, dim3(groups), dim3(256), 0, (hipStream_t)stream, static_cast<uint4 *>(dst), static_cast<const uint4 *>(src_dev), n16);
    QZ_CHECK(hipGetLastError(), "launch qzstd_copy_in_kernel");
    return 0;
}

int qzstd_hip_memcpy_d2h(int device, void *stream, void *dst, const void *src, size_t bytes)
{
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream), "hipMemcpyAsync D2H");
    return 0;
}

int qzstd_hip_memset(int device, void *stream, void *dst, int value, size_t bytes)
{
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream), "hipMemsetAsync");
    return 0;
}

int qzstd_hip_memcpy2d_d2h(int device, void *stream, void *dst, size_t dpitch, const void *src, size_t spitch,
                           size_t width, size_t height)
{
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost, (hipStream_t)stream),
             "hipMemcpy2DAsync D2H");
    return 0;
}

int qzstd_hip_pointer_device(const void *p)
{
    if (!p) return -1;
    const int n = qzstd_hip_device_count();
    if (n <= 0) return -1;
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return -1; } /* memory the runtime does not know: host */
    if (a.type != hipMemoryTypeDevice || a.isManaged) return -1;
    for (int d = 0; d < n; d++)
        if (g_devMap[d] == a.device) return d;
    return -1;
}

int qzstd_hip_pointer_extent(const void *p, const void **lo, size_t *size)
{
    if (lo) *lo = nullptr;
    if (size) *size = 0;
    const int d = qzstd_hip_pointer_device(p);
    if (d < 0 || !lo || !size) return d;
    hipDeviceptr_t b = nullptr;
    size_t n = 0;
    if (hipMemGetAddressRange(&b, &n, (hipDeviceptr_t)const_cast<void *>(p)) != hipSuccess) { (void)hipGetLastError(); return d; }
    const char *first = static_cast<const char *>((const void *)b), *at = static_cast<const char *>(p);
    if (b && at >= first && (size_t)(at - first) < n) { *lo = (const void *)b; *size = n; }
    return d;
}

void *qzstd_hip_event_create(int device)
{
    hipEvent_t e = nullptr;
    if (phys(device) < 0 || hipSetDevice(phys(device)) != hipSuccess) return nullptr;
    const hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (r != hipSuccess) { fail("hipEventCreate", r); return nullptr; }
    return (void *)e;
}

void qzstd_hip_event_destroy(int device, void *event)
{
    if (event && phys(device) >= 0 && hipSetDevice(phys(device)) == hipSuccess) (void)hipEventDestroy((hipEvent_t)event);
}

int qzstd_hip_event_record(int device, void *event, void *stream)
{
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipEventRecord((hipEvent_t)event, (hipStream_t)stream), "hipEventRecord");
    return 0;
}

int qzstd_hip_stream_wait_event(int device, void *stream, void *event)
{
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0), "hipStreamWaitEvent");
    return 0;
}

int qzstd_hip_memcpy2d_d2d(int device, void *stream, void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height)
{
    QZ_SET_DEVICE(device);
    QZ_CHECK(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToDevice, (hipStream_t)stream), "hipMemcpy2DAsync D2D");
    return 0;
}

} /* extern "C" */
