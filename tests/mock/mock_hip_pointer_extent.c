/*
 * mock_hip_pointer_extent.c — TEST INFRASTRUCTURE ONLY.  qzstd_hip_pointer_extent (include/qzstd_hip_device.h) for the CPU stand-in of
 * tests/mock/mock_hip_device.c: the allocations are what the test registers with qzstd_mock_extent_range() — beside the ranges it registers
 * there, which answer qzstd_hip_pointer_device — and the look-ups are counted.  A source of its own: a mock built without it is a device layer
 * that tells no extents, and the front-end looks every range up at its first and its last byte.
 */
#include "qzstd_hip_device.h"

#define MOCK_EXTENTS 16
static struct { const unsigned char *p; size_t n; } gExtents[MOCK_EXTENTS];
static int gExtentLookups;

/* test hooks */
void qzstd_mock_extent_range(int slot, const void *p, size_t n)
{
    if (slot < 0 || slot >= MOCK_EXTENTS) return;
    gExtents[slot].p = (const unsigned char *)p;
    gExtents[slot].n = n;
}
int qzstd_mock_extent_lookups(void) { return gExtentLookups; }

int qzstd_hip_pointer_extent(const void *p, const void **lo, size_t *size)
{
    const int d = qzstd_hip_pointer_device(p);
    int k;
    __sync_fetch_and_add(&gExtentLookups, 1);
    if (lo) *lo = 0;
    if (size) *size = 0;
    if (d < 0 || !lo || !size) return d;
    for (k = 0; k < MOCK_EXTENTS; k++)
        if (gExtents[k].p && (const unsigned char *)p >= gExtents[k].p && (const unsigned char *)p < gExtents[k].p + gExtents[k].n) {
            *lo = gExtents[k].p;
            *size = gExtents[k].n;
            break;
        }
    return d;
}
