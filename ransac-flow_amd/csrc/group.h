// group.h -- grouped launches: ONE launch for the same layer of several independent problems of different sizes.
//
// A single 480x640 pair runs the ResNet-50 trunk on 8 images of 8 different sizes (7 pyramid levels + the target,
// quick_start/coarseAlignFeatMatch.py:92-125).  Layer by layer that is 8 launches of 2-150 workgroups each on 256 CUs: the
// pass is bound by one workgroup lifetime per layer AND level.  Between rfx_group_begin() and rfx_group_end() the
// convolution entry points, the two stems and the fine-stage kernels (warp.hip, pool.hip, corr.hip) do not launch; they record (kernel instance, argument block, grid), and rfx_group_end() issues,
// per kernel instance, ONE launch whose blockIdx.y selects the problem (argument block p[blockIdx.y], workgroups past that
// problem's own grid exit at once).  The device code of a problem is the single-launch kernel's body, unchanged: results are
// bit-identical by construction.  Everything recorded in one group must be mutually independent.
#pragma once
#include "common.h"

constexpr int RFX_MAX_GROUP = 8;

template <class A> struct RfxGroupArgs {
    A p[RFX_MAX_GROUP];
    unsigned gx[RFX_MAX_GROUP];   // workgroups of problem i (its own gridDim.x)
};

// launcher of one grouped kernel instance: `blob` = n argument blocks of `arg_size` bytes, gx = their grids
typedef int (*rfx_group_launch_fn)(const void* blob, const unsigned* gx, int n, hipStream_t st);

bool rfx_group_recording();
int rfx_group_record(rfx_group_launch_fn fn, const void* args, size_t arg_size, unsigned grid_x);

// Generic launcher body for a grouped kernel K(RfxGroupArgs<A>) with BLOCK threads.
template <class A, class K>
static int rfx_group_launch_impl(K kernel, int block, const void* blob, const unsigned* gx, int n, hipStream_t st) {
    static_assert(sizeof(RfxGroupArgs<A>) <= 2048, "grouped argument block: keep it well under the 4 KB kernarg limit");
    RfxGroupArgs<A> g;
    unsigned gmax = 0;
    const A* src = static_cast<const A*>(blob);
    for (int i = 0; i < RFX_MAX_GROUP; ++i) {
        g.p[i] = src[i < n ? i : 0];
        g.gx[i] = i < n ? gx[i] : 0u;
        if (g.gx[i] > gmax) gmax = g.gx[i];
    }
    hipLaunchKernelGGL(kernel, dim3(gmax, (unsigned)n), dim3(block), 0, st, g);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// A kernel family = its argument block A, its body -- a __device__ function of (arguments, the problem's own block index bx, the
// problem's own grid gx; a body without a grid-stride loop leaves gx unnamed) -- its block size and, only where the family has one,
// the second __launch_bounds__ argument.  RfxFamily makes the grouped kernel, the launcher rfx_group_record() stores and the
// "record if a group is recording" step from them; the single-launch kernel takes its launch bound from it:
//     using WarpGrid = RfxFamily<WarpGridArgs, warp_grid_body, 256>;
//     __global__ __launch_bounds__(WarpGrid::BLOCK) void warp_grid_kernel(WarpGridArgs a) { ...body(a, blockIdx.x, gridDim.x); }
//     ... return WarpGrid::launch(warp_grid_kernel, a, grid, stream);
template <class A> using RfxBody = void (*)(const A&, unsigned, unsigned);

// The grouped kernel of family F (an RfxFamily: a class type, so that the kernel's name demangles everywhere and shows the body
// with its template arguments): blockIdx.y = problem, the body on that problem's argument block and its own grid.  The body is called
// straight from the kernel, as the hand-written grouped kernels called it, not through one more inlined function: that keeps every
// instance's machine code what it was (profiles/group_launch_codegen.tsv).
template <class F>
__global__ __launch_bounds__(F::BLOCK) void rfx_group_kernel(RfxGroupArgs<typename F::Args> g) {
    const unsigned y = blockIdx.y;
    if (blockIdx.x >= g.gx[y]) return;
    F::body(g.p[y], blockIdx.x, g.gx[y]);
}
// __launch_bounds__(B) and __launch_bounds__(B, n) are different attributes for every n, so a family without a second argument must
// not get one from a default: the families that have one take this kernel
template <class F>
__global__ __launch_bounds__(F::BLOCK, F::min_waves()) void rfx_group_kernel_w(RfxGroupArgs<typename F::Args> g) {
    const unsigned y = blockIdx.y;
    if (blockIdx.x >= g.gx[y]) return;
    F::body(g.p[y], blockIdx.x, g.gx[y]);
}

template <class A, RfxBody<A> Body, int BLOCK_, int... MIN_WAVES_>
struct RfxFamily {
    static_assert(sizeof...(MIN_WAVES_) <= 1, "at most one second __launch_bounds__ argument");
    using Args = A;
    static constexpr RfxBody<A> body = Body;
    static constexpr int BLOCK = BLOCK_;
    // the second __launch_bounds__ argument; a compile error in a family declared without one
    static constexpr int min_waves() {
        static_assert(sizeof...(MIN_WAVES_) == 1, "this family has no second __launch_bounds__ argument");
        return (0 + ... + MIN_WAVES_);
    }

    // the launcher rfx_group_record() stores (and keys the bucket by)
    static int group_launch(const void* blob, const unsigned* gx, int n, hipStream_t st) {
        if constexpr (sizeof...(MIN_WAVES_) == 0)
            return rfx_group_launch_impl<A>(rfx_group_kernel<RfxFamily>, BLOCK, blob, gx, n, st);
        else
            return rfx_group_launch_impl<A>(rfx_group_kernel_w<RfxFamily>, BLOCK, blob, gx, n, st);
    }
    // the record half alone, for a family with a single-launch statement of its own (corr.hip)
    static int record(const A& a, unsigned gx) { return rfx_group_record(&group_launch, &a, sizeof(A), gx); }
    // record where a group is recording, else launch `single`, the family's single-launch kernel, on gx workgroups
    template <class K> static int launch(K single, const A& a, unsigned gx, hipStream_t st) {
        if (rfx_group_recording()) return record(a, gx);
        hipLaunchKernelGGL(single, dim3(gx), dim3(BLOCK), 0, st, a);
        RFX_LAUNCH_CHECK();
        return RFX_OK;
    }
};
