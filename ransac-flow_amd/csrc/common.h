// Shared helpers for the librfx HIP translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/rfx_api.h"

#define RFX_LAUNCH_CHECK()                         \
    do {                                           \
        hipError_t e__ = hipGetLastError();        \
        if (e__ != hipSuccess) return (int)e__;    \
    } while (0)

static inline hipStream_t rfx_stream(void* s) { return (hipStream_t)s; }

static inline int rfx_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// XCD-aware bijective remap of a launch's nwg workgroups.  The hardware deals workgroup b to XCD b % 8 (observed), so consecutive
// workgroups sit on eight different L2s.  Here each XCD walks one contiguous chunk of the tile space instead (the first nwg % 8
// XCDs get one tile more): with the channel tile running fastest in the id that comes back, the workgroups that share one input
// pixel tile / patch run on one L2.  A persistent kernel whose grid is a multiple of 8 may call it per tile: v % 8 stays its XCD.
static __device__ __forceinline__ int xcd_remap(unsigned bx, int nwg) {
    const int v = (int)bx, q = nwg / 8, r = nwg % 8, xcd = v % 8, j = v / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}
