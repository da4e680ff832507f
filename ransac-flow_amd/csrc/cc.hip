// cc.hip -- the small-component filter of the KITTI scripts on the device: zero every 8-connected component of
// (match > match_th) whose area is at most max_area pixels (evaluation/evalKITTI/evaluation.py:85-100 online,
// evaluation/evalKITTI/getResults.py:66-84 offline; both call skimage.measure.label on the host and loop over the
// component ids).  The result does not depend on how components are numbered, so any exact labelling reproduces the
// reference bit for bit: here a lock-free union-find over the pixel grid.
//   1. background pixels get parent -1; foreground pixels are linked along their row (no atomics, see cc_init_kernel);
//   2. unions with the row above, only the non-redundant ones: roots are linked larger -> smaller index with atomicCAS,
//      finds use path halving (see cc_union_kernel);
//   3. label[p] = find(p);  4. area[label] += 1;  5. out = (foreground && area[label] <= max_area && area[label] < H*W) ? 0 : in.
// Steps are separate launches (the grid-wide ordering between them is the stream's).  One int32 triple per pixel of
// workspace.  The area threshold arrives as an integer (the host turns the reference's float64 test
// "area / size <= cc_th" into the largest pixel count that passes it), so no floating point enters the decision.
// The four kernel bodies are the cc_*_body.inc files: the dense kernels run them on an (N,H,W) batch, the ragged kernels (below) on
// each map of a packed buffer of maps of different sizes.
#include "common.h"

namespace {

// parent[] is read and written by every CU while the forest is being built: device-scope atomic loads / stores keep the
// accesses out of the (non-coherent) per-CU L1, so a find never spins on a stale line.
__device__ __forceinline__ int cc_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int cc_find(int* parent, int i) {
    while (true) {
        const int p = cc_ld(parent + i);
        if (p == i) return i;
        const int gp = cc_ld(parent + p);
        if (gp != p) cc_st(parent + i, gp);   // path halving; a late write only keeps a longer (still valid) chain
        i = p;
    }
}

__device__ __forceinline__ void cc_unite(int* parent, int a, int b) {
    while (true) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }          // link the larger root under the smaller
        if (atomicCAS(&parent[a], a, b) == a) return;           // a was still a root: linked; otherwise retry
    }
}

// 1. A wavefront takes 64 consecutive pixels.  Every foreground pixel is linked -- without atomics, nobody else writes
// parent[] yet -- to the first pixel of its horizontal run inside this 64-pixel segment; a run that continues from the
// previous segment hangs its first pixel here on the pixel to its left.  The row direction of the labelling is thereby
// done before the union phase starts: a solid region costs no union at all (see the rules below), and a find walks at most
// one link per 64 pixels of a run.
__global__ __launch_bounds__(256) void cc_init_kernel(const float* __restrict__ in, int* __restrict__ parent, int* __restrict__ area,
                                                     long long total, int W, float th) {
#include "cc_init_body.inc"
}

// 2. Unions across rows, only where they can join something new.  With the row links in place, for a foreground pixel p
// (W, NW, N, NE, E = its neighbours):
//   N  is redundant when W and NW are foreground (p - W - NW - N is already a path);
//   NW is redundant when W or N is foreground (W's own N neighbour is NW; N and NW are row neighbours);
//   NE is redundant when N is foreground (row neighbours) or E is foreground (E's N neighbour is NE).
// An interior pixel of a solid region issues nothing; the atomics that remain are the ones at region boundaries.
__global__ __launch_bounds__(256) void cc_union_kernel(int* __restrict__ parent, long long total, int H, int W) {
#include "cc_union_body.inc"
}

// 3./4. label = root; area[root] += 1.  The pixels of one wavefront mostly share their root (a matched region is one large
// component), and a per-pixel atomicAdd would queue every pixel of that component on ONE address: the lanes that hold the
// same root are counted with a ballot and their leader adds the count -- one atomic per (wavefront, root).
__global__ __launch_bounds__(256) void cc_label_kernel(int* __restrict__ parent, int* __restrict__ label, int* __restrict__ area,
                                                      long long total) {
#include "cc_label_body.inc"
}

__global__ __launch_bounds__(256) void cc_apply_kernel(const float* __restrict__ in, const int* __restrict__ label,
                                                      const int* __restrict__ area, float* __restrict__ out, long long total,
                                                      int max_area, int HW) {
#include "cc_apply_body.inc"
}

// ---- ragged form: the maps of one launch chain differ in size -------------------------------------------------------------------
// Map k of the round is h_k x w_k floats at element offset off[k] of ONE packed buffer (the layout rfx_multih_accept_ragged_f32
// consumes); row k of the device table dims (n,3) int32 = h_k, w_k, max_area_k.  blockIdx.y = the map; the workgroups of a column of
// the grid stride over that map's own pixels.  Every kernel moves its pointers to the map's origin and runs the dense kernel's body
// text on the map as an image batch of one: indices, parents and labels are LOCAL to the map, so a wavefront's 64-pixel segment is
// cut relative to the map's origin (off[k] need not be a multiple of 64), rows and columns come from the map's own width, and no
// link or union can leave the map.  A table row that does not fit the buffer is skipped (nothing is read or written for it).
struct CcMap { long long org, total; int H, W, max_area; bool ok; };
__device__ __forceinline__ CcMap cc_map(const long long* __restrict__ off, const int32_t* __restrict__ dims, long long total_px) {
    const int k = blockIdx.y;
    CcMap m;
    m.org = off[k]; m.H = dims[3 * k]; m.W = dims[3 * k + 1]; m.max_area = dims[3 * k + 2];
    m.total = (long long)m.H * m.W;
    m.ok = m.H > 0 && m.W > 0 && m.max_area >= 0 && m.org >= 0 && m.org + m.total <= total_px;
    return m;
}

__global__ __launch_bounds__(256) void cc_init_ragged_kernel(const float* __restrict__ in, int* __restrict__ parent, int* __restrict__ area,
                                                            const long long* __restrict__ off, const int32_t* __restrict__ dims,
                                                            long long total_px, float th) {
    const CcMap m = cc_map(off, dims, total_px);
    if (!m.ok) return;
    in += m.org; parent += m.org; area += m.org;
    const long long total = m.total;
    const int W = m.W;
#include "cc_init_body.inc"
}

__global__ __launch_bounds__(256) void cc_union_ragged_kernel(int* __restrict__ parent, const long long* __restrict__ off,
                                                             const int32_t* __restrict__ dims, long long total_px) {
    const CcMap m = cc_map(off, dims, total_px);
    if (!m.ok) return;
    parent += m.org;
    const long long total = m.total;
    const int H = m.H, W = m.W;
#include "cc_union_body.inc"
}

__global__ __launch_bounds__(256) void cc_label_ragged_kernel(int* __restrict__ parent, int* __restrict__ label, int* __restrict__ area,
                                                             const long long* __restrict__ off, const int32_t* __restrict__ dims,
                                                             long long total_px) {
    const CcMap m = cc_map(off, dims, total_px);
    if (!m.ok) return;
    parent += m.org; label += m.org; area += m.org;
    const long long total = m.total;
#include "cc_label_body.inc"
}

__global__ __launch_bounds__(256) void cc_apply_ragged_kernel(const float* __restrict__ in, const int* __restrict__ label,
                                                             const int* __restrict__ area, float* __restrict__ out,
                                                             const long long* __restrict__ off, const int32_t* __restrict__ dims,
                                                             long long total_px) {
    const CcMap m = cc_map(off, dims, total_px);
    if (!m.ok) return;
    in += m.org; label += m.org; area += m.org; out += m.org;
    const long long total = m.total;
    const int max_area = m.max_area, HW = (int)m.total;         // "the whole image" is the map's own h * w
#include "cc_apply_body.inc"
}

}  // namespace

extern "C" size_t rfx_remove_small_cc_ws_bytes(int N, int H, int W) { return (size_t)3 * sizeof(int) * (size_t)N * H * W; }

extern "C" int rfx_remove_small_cc_f32(const float* in, float* out, int N, int H, int W, float match_th, int max_area, void* ws,
                                       void* stream) {
    if (!in || !out || !ws || N <= 0 || H <= 0 || W <= 0 || max_area < 0) return RFX_E_ARG;
    const long long total = (long long)N * H * W;
    if (total > 0x7fffffffLL) return RFX_E_LIMIT;
    int* parent = static_cast<int*>(ws);
    int* label = parent + total;
    int* area = label + total;
    hipStream_t st = rfx_stream(stream);
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    hipLaunchKernelGGL(cc_init_kernel, dim3(grid), dim3(256), 0, st, in, parent, area, total, W, match_th);
    hipLaunchKernelGGL(cc_union_kernel, dim3(grid), dim3(256), 0, st, parent, total, H, W);
    hipLaunchKernelGGL(cc_label_kernel, dim3(grid), dim3(256), 0, st, parent, label, area, total);
    hipLaunchKernelGGL(cc_apply_kernel, dim3(grid), dim3(256), 0, st, in, label, area, out, total, max_area, H * W);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" size_t rfx_remove_small_cc_ragged_ws_bytes(long long total_px) {
    return total_px > 0 ? (size_t)3 * sizeof(int) * (size_t)total_px : 0;
}

extern "C" int rfx_remove_small_cc_ragged_f32(const float* in, float* out, const long long* match_off, const int32_t* dims,
                                              int n_active, long long total_px, long long max_hw, float match_th, void* ws,
                                              void* stream) {
    if (!in || !out || !match_off || !dims || !ws || n_active <= 0 || total_px <= 0 || max_hw <= 0 || max_hw > total_px)
        return RFX_E_ARG;
    if (total_px > 0x7fffffffLL || n_active > 65535) return RFX_E_LIMIT;
    int* parent = static_cast<int*>(ws);
    int* label = parent + total_px;
    int* area = label + total_px;
    hipStream_t st = rfx_stream(stream);
    // the grid's x extent follows the LARGEST map: a smaller map's surplus workgroups find no pixel and leave
    const dim3 grid((unsigned)((max_hw + 255) / 256 < 16384 ? (max_hw + 255) / 256 : 16384), (unsigned)n_active);
    hipLaunchKernelGGL(cc_init_ragged_kernel, grid, dim3(256), 0, st, in, parent, area, match_off, dims, total_px, match_th);
    hipLaunchKernelGGL(cc_union_ragged_kernel, grid, dim3(256), 0, st, parent, match_off, dims, total_px);
    hipLaunchKernelGGL(cc_label_ragged_kernel, grid, dim3(256), 0, st, parent, label, area, match_off, dims, total_px);
    hipLaunchKernelGGL(cc_apply_ragged_kernel, grid, dim3(256), 0, st, in, label, area, out, match_off, dims, total_px);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}
