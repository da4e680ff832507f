// points_ragged.hip -- rfx_flow_points_ragged_f32: the pixel correspondences of all explained pixels (evaluation/evalYFCC/
// getResults.py:53-71, matches_from_flow) of B maps of DIFFERENT sizes in one chain -- the packed buffers rfx_assemble_records_f32
// fills for a ragged batch, every map with its own quarter turn k and its own source size (wA, hA).  The design is points.hip's
// carried over (its rule, its three launches, its tiling: points_tile.h); what differs is where a tile's map comes from:
//   a map of H * W pixels has ceil(H * W / POINTS_TILE) tiles, so the tiles per map differ and a workgroup finds the map of its tile
//   by a binary search over the table's first-tile column -- uniform per workgroup -- and takes the map's offset, shape, turn and
//   sizes from that row;
//   1. count:   counts[tile] = kept pixels of the tile (ballots, a tally per wavefront, four tallies added by thread 0);
//   2. scan:    ONE 1024-thread workgroup turns the tile counts into their exclusive prefix, in place, then writes
//               offsets[b] = the prefix at map b's first tile, offsets[B] = the total;
//   3. scatter: the tiling of 1. again; recomputed ballots rank every kept pixel inside its tile, row = tile prefix + rank.
// No atomics, no workgroup waits on another; both tiled grids are capped and stride.  A table row that does not describe a map
// inside the buffers (ragged_tile) has no kept pixel.  Built with -ffp-contract=off, like points.hip.
#include "common.h"
#include "points_tile.h"

namespace {

constexpr int RT_COLS = 8;       // table row: pixel offset | H | W | k | wA | hA | index of the map's first tile | 0

struct RaggedTile {
    long long off;               // the map's first pixel in the packed buffers
    long long p0;                // the tile's first pixel inside the map
    int HW, W, k, wB, hB;
    float sx, sy;                // (float)(wA - 1), (float)(hA - 1)
    bool ok;
};

// The map of ``tile`` and the tile's place in it: the last row whose first tile is <= tile.  Not ok -- nothing is read, nothing is
// kept -- unless the row describes a map inside the buffers: 0 <= off, 1 <= H, W, off + H * W <= total_px, k in 0..3, 1 <= wA, hA
// < 2^31 and the tile starts inside the map.
__device__ __forceinline__ RaggedTile ragged_tile(const long long* __restrict__ table, int B, long long tile, long long total_px) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(long long)mid * RT_COLS + 6] <= tile) lo = mid; else hi = mid - 1;
    }
    const long long* r = table + (long long)lo * RT_COLS;
    const long long off = r[0], H = r[1], W = r[2], k = r[3], wA = r[4], hA = r[5], first = r[6];
    RaggedTile m;
    m.ok = off >= 0 && H >= 1 && W >= 1 && H <= total_px && W <= total_px && H * W <= total_px - off && k >= 0 && k <= 3 && wA >= 1 &&
           hA >= 1 && wA <= 0x7fffffffLL && hA <= 0x7fffffffLL && first >= 0 && first <= tile &&
           (tile - first) * POINTS_TILE < H * W;
    m.off = off;
    m.p0 = m.ok ? (tile - first) * POINTS_TILE : 0;              // with HW = 0: no pixel of the tile is inside
    m.HW = m.ok ? (int)(H * W) : 0;
    m.W = m.ok ? (int)W : 1;
    m.k = (int)k;
    m.wB = (int)((k & 1) ? H : W);
    m.hB = (int)((k & 1) ? W : H);
    m.sx = (float)(wA - 1);
    m.sy = (float)(hA - 1);
    return m;
}

// pixel p of the tile's map is kept: inside the map, keep non-zero, and bg (if any) non-zero
__device__ __forceinline__ bool ragged_kept(const unsigned char* __restrict__ keep, const unsigned char* __restrict__ bg,
                                            const RaggedTile& m, long long p) {
    if (p >= m.HW) return false;
    const long long i = m.off + p;
    return keep[i] != 0 && (!bg || bg[i] != 0);
}

// 1. counts[tile] = kept pixels of the tile
__global__ __launch_bounds__(POINTS_BLOCK) void points_ragged_count_kernel(const unsigned char* __restrict__ keep,
                                                                           const unsigned char* __restrict__ bg,
                                                                           const long long* __restrict__ table, int B, long long tiles,
                                                                           long long total_px, int* __restrict__ counts) {
    __shared__ int wsum[POINTS_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const RaggedTile m = ragged_tile(table, B, tile, total_px);
        int c = 0;
#pragma unroll
        for (int s = 0; s < POINTS_PASSES; ++s) c += __popcll(__ballot(ragged_kept(keep, bg, m, m.p0 + s * POINTS_BLOCK + t)));
        if (lane == 0) wsum[wave] = c;
        __syncthreads();
        if (t == 0) {
            int tot = 0;
#pragma unroll
            for (int w = 0; w < POINTS_WAVES; ++w) tot += wsum[w];
            counts[tile] = tot;
        }
        __syncthreads();                                           // the next tile rewrites wsum
    }
}

// 2. counts -> exclusive prefix, in place (points_scan_kernel's trips: the running total lives in a register, int32 holds a sum of
// at most total_px <= 2^31 - 1), then offsets (B+1): map b's rows start at the prefix of its first tile.  The barrier between the
// two orders the prefix stores of this one workgroup before its reads.
__global__ __launch_bounds__(POINTS_SCAN_BLOCK) void points_ragged_scan_kernel(int* __restrict__ counts, long long* __restrict__ offsets,
                                                                               const long long* __restrict__ table, int B,
                                                                               long long tiles) {
    __shared__ int wsum[POINTS_SCAN_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int base = 0;
    for (long long s = 0; s < tiles; s += POINTS_SCAN_BLOCK) {
        const long long i = s + t;
        const int c = i < tiles ? counts[i] : 0;
        int inc = c;                                               // inclusive prefix inside the wavefront
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(inc, d);
            if (lane >= d) inc += v;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < POINTS_SCAN_BLOCK / 64; ++w) { const int x = wsum[w]; if (w < wave) woff += x; tot += x; }
        __syncthreads();                                           // the next trip rewrites wsum
        if (i < tiles) counts[i] = base + woff + inc - c;
        base += tot;
    }
    __syncthreads();
    for (int b = t; b < B; b += POINTS_SCAN_BLOCK) {
        const long long first = table[(long long)b * RT_COLS + 6];
        offsets[b] = first < 0 ? 0 : first < tiles ? counts[first] : base;         // (a first tile outside the grid: a skipped row)
    }
    if (t == 0) offsets[B] = base;
}

// 3. prefix[tile] = rows before the tile; wsum double-buffered over the passes as in points_scatter_kernel.
__global__ __launch_bounds__(POINTS_BLOCK) void points_ragged_scatter_kernel(const float2* __restrict__ flow,
                                                                             const unsigned char* __restrict__ keep,
                                                                             const unsigned char* __restrict__ bg,
                                                                             const long long* __restrict__ table, int B, long long tiles,
                                                                             long long total_px, const int* __restrict__ prefix,
                                                                             float2* __restrict__ pts1, i64x2* __restrict__ pts2) {
    __shared__ int wsum[2][POINTS_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const RaggedTile m = ragged_tile(table, B, tile, total_px);
        int base = prefix[tile];
#pragma unroll
        for (int s = 0; s < POINTS_PASSES; ++s) {
            const long long p = m.p0 + s * POINTS_BLOCK + t;
            const bool kept = ragged_kept(keep, bg, m, p);
            const unsigned long long bal = __ballot(kept);
            if (lane == 0) wsum[s & 1][wave] = __popcll(bal);
            __syncthreads();
            int woff = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < POINTS_WAVES; ++w) { const int x = wsum[s & 1][w]; if (w < wave) woff += x; tot += x; }
            const long long row = (long long)base + woff + __popcll(bal & ((1ull << lane) - 1ull));
            if (kept && (unsigned long long)row < (unsigned long long)total_px) {   // inside the buffers whatever prefix[] holds
                const int i = (int)p / m.W, j = (int)p - i * m.W;  // p < H * W <= 2^31 - 1
                const float2 f = flow[m.off + p];
                float2 a;
                a.x = f.x + 1.0f; a.x = a.x * m.sx; a.x = a.x / 2.0f;
                a.y = f.y + 1.0f; a.y = a.y * m.sy; a.y = a.y / 2.0f;
                i64x2 b;                                           // np.rot90(gridB, k)[i, j]
                if (m.k == 0) { b.x = j; b.y = i; }
                else if (m.k == 1) { b.x = m.wB - 1 - i; b.y = j; }
                else if (m.k == 2) { b.x = m.wB - 1 - j; b.y = m.hB - 1 - i; }
                else { b.x = i; b.y = m.hB - 1 - j; }
                pts1[row] = a;
                pts2[row] = b;
            }
            base += tot;
        }
    }
}

}  // namespace

extern "C" size_t rfx_flow_points_ragged_ws_bytes(long long total_tiles) {
    return total_tiles > 0 ? sizeof(int) * (size_t)total_tiles : 0;
}

extern "C" int rfx_flow_points_ragged_f32(const float* flow, const unsigned char* keep, const unsigned char* bg, const long long* table,
                                          int B, long long total_px, long long total_tiles, float* pts1, long long* pts2,
                                          long long* offsets, void* ws, void* stream) {
    if (!flow || !keep || !table || !pts1 || !pts2 || !offsets || !ws || B <= 0 || total_px <= 0 || total_tiles <= 0 ||
        total_tiles > total_px)
        return RFX_E_ARG;
    if (!points_aligned(flow, 8) || !points_aligned(table, 8) || !points_aligned(pts1, 8) || !points_aligned(pts2, 16) ||
        !points_aligned(offsets, 8) || !points_aligned(ws, 4))
        return RFX_E_ARG;
    if (total_px > 0x7fffffffLL || B > 65535) return RFX_E_LIMIT;
    hipStream_t st = rfx_stream(stream);
    int* counts = static_cast<int*>(ws);
    const int grid = (int)(total_tiles < POINTS_GRID_CAP ? total_tiles : POINTS_GRID_CAP);
    hipLaunchKernelGGL(points_ragged_count_kernel, dim3(grid), dim3(POINTS_BLOCK), 0, st, keep, bg, table, B, total_tiles, total_px,
                       counts);
    hipLaunchKernelGGL(points_ragged_scan_kernel, dim3(1), dim3(POINTS_SCAN_BLOCK), 0, st, counts, offsets, table, B, total_tiles);
    hipLaunchKernelGGL(points_ragged_scatter_kernel, dim3(grid), dim3(POINTS_BLOCK), 0, st, reinterpret_cast<const float2*>(flow), keep,
                       bg, table, B, total_tiles, total_px, counts, reinterpret_cast<float2*>(pts1), reinterpret_cast<i64x2*>(pts2));
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}
