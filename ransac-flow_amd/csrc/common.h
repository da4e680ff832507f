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

// workspace sub-arrays start on 256-byte boundaries
static inline size_t rfx_al256(size_t x) { return (x + 255) & ~(size_t)255; }

// Ordered compaction for ONE 1024-thread workgroup (16 wavefronts): item s + threadIdx.x of trip s / 1024 gets the number of kept items
// before it, so the kept items land in item order.  rfx_ordered_compact_begin() owns the LDS (16 per-wavefront tallies, the running
// total).  place() holds three barriers: EVERY thread of the workgroup calls it the same number of times (keep = false past the end of
// the list), and what a thread writes with the returned position is not ordered against the other threads without a further barrier.
struct RfxOrderedCompact {
    int* wsum;   // [16], then the running total
    __device__ __forceinline__ int place(bool keep) {
        const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int c = wsum[w]; if (w < wave) woff += c; tot += c; }
        const int b = wsum[16];
        __syncthreads();
        if (t == 0) wsum[16] = b + tot;
        __syncthreads();
        return b + woff + before;
    }
    // kept items of all trips so far (any thread, after a place())
    __device__ __forceinline__ int total() const { return wsum[16]; }
};

static __device__ __forceinline__ RfxOrderedCompact rfx_ordered_compact_begin() {
    __shared__ int lds[17];
    if (threadIdx.x == 0) lds[16] = 0;
    __syncthreads();
    return RfxOrderedCompact{lds};
}

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
