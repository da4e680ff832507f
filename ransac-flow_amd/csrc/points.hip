// points.hip -- what the YFCC and Corr results scripts read off an assembled flow, on the device.
// (a) rfx_flow_points_f32: the pixel correspondences of all explained pixels (evaluation/evalYFCC/getResults.py:53-71,
//     matches_from_flow: gridB = np.rot90(meshgrid, k); pts2 = gridB[mask]; pts1 = (flow[mask] + 1) * (size - 1) / 2), a stream
//     compaction over N full-resolution maps in numpy's boolean-indexing order: map after map, row-major inside a map.
//     Three launches, ordered by the stream; no workgroup waits on another, no atomic decides a position:
//       1. count:   a workgroup takes a tile of POINTS_TILE consecutive pixels of ONE map (tiles never straddle two maps) and writes
//                   the number of kept pixels in it -- ballots, a tally per wavefront, four tallies added by thread 0;
//       2. scan:    ONE 1024-thread workgroup turns the tile counts into their exclusive prefix, in place, 1024 tiles per trip, and
//                   writes offsets[n] = the prefix at map n's first tile, offsets[N] = the total;
//       3. scatter: the tiling of 1. again; a workgroup recomputes its ballots, ranks every kept pixel inside the tile (kept pixels of
//                   earlier passes + of earlier wavefronts of this pass + of lower lanes) and writes row (tile prefix + rank).
//     Flow is read only where kept; a pts1 row is one 8-byte store, a pts2 row one 16-byte store.
// (b) rfx_sample_points_f32: the keypoint transfer of evaluation/evalCorr/getResults.py:15-31 (alignmentError), one thread per point.
// Built with -ffp-contract=off: every float32 step below is rounded on its own, in the order written.
#include "common.h"
#include "points_tile.h"

namespace {

struct PointsTiling {
    long long tiles;     // N * per_map
    int per_map;         // ceil(H * W / POINTS_TILE)
    int HW;
    long long rows;      // N * H * W: the rows pts1 / pts2 have room for
};

// pixel p of map n is kept: inside the map, keep non-zero, and bg (if any) non-zero
__device__ __forceinline__ bool points_kept(const unsigned char* __restrict__ keep, const unsigned char* __restrict__ bg,
                                            long long n, long long p, int HW) {
    if (p >= HW) return false;
    const long long i = n * HW + p;
    return keep[i] != 0 && (!bg || bg[i] != 0);
}

// 1. counts[tile] = kept pixels of the tile.  Pass s of a tile looks at pixels tile * POINTS_TILE + s * 256 + threadIdx.x.
__global__ __launch_bounds__(POINTS_BLOCK) void points_count_kernel(const unsigned char* __restrict__ keep,
                                                                    const unsigned char* __restrict__ bg, int* __restrict__ counts,
                                                                    PointsTiling tl) {
    __shared__ int wsum[POINTS_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (long long tile = blockIdx.x; tile < tl.tiles; tile += gridDim.x) {
        const long long n = tile / tl.per_map;
        const long long p0 = (tile - n * tl.per_map) * POINTS_TILE;
        int c = 0;
#pragma unroll
        for (int s = 0; s < POINTS_PASSES; ++s)
            c += __popcll(__ballot(points_kept(keep, bg, n, p0 + s * POINTS_BLOCK + t, tl.HW)));
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

// 2. counts -> exclusive prefix, in place; offsets (N+1).  Every thread of the one workgroup walks the same trips and adds up the same
// running total, so the total lives in a register.  The whole sum is at most N * H * W <= 2^31 - 1: int32 holds it.
__global__ __launch_bounds__(POINTS_SCAN_BLOCK) void points_scan_kernel(int* __restrict__ counts, long long* __restrict__ offsets,
                                                                        PointsTiling tl, int N) {
    __shared__ int wsum[POINTS_SCAN_BLOCK / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int base = 0;
    for (long long s = 0; s < tl.tiles; s += POINTS_SCAN_BLOCK) {
        const long long i = s + t;
        const int c = i < tl.tiles ? counts[i] : 0;
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
        if (i < tl.tiles) {
            const int before = base + woff + inc - c;
            counts[i] = before;
            if (i % tl.per_map == 0) offsets[i / tl.per_map] = before;
        }
        base += tot;
    }
    if (t == 0) offsets[N] = base;
}

// 3. prefix[tile] = rows before the tile.  wsum is double-buffered over the passes: one barrier per pass (a thread that writes the
// buffer of pass s + 2 has passed the barrier of pass s + 1, which every reader of pass s reached after its reads).
__global__ __launch_bounds__(POINTS_BLOCK) void points_scatter_kernel(const float2* __restrict__ flow,
                                                                      const unsigned char* __restrict__ keep,
                                                                      const unsigned char* __restrict__ bg,
                                                                      const int* __restrict__ prefix, float2* __restrict__ pts1,
                                                                      i64x2* __restrict__ pts2, PointsTiling tl, int W, int k,
                                                                      float sx, float sy, int wB, int hB) {
    __shared__ int wsum[2][POINTS_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (long long tile = blockIdx.x; tile < tl.tiles; tile += gridDim.x) {
        const long long n = tile / tl.per_map;
        const long long p0 = (tile - n * tl.per_map) * POINTS_TILE;
        int base = prefix[tile];
#pragma unroll
        for (int s = 0; s < POINTS_PASSES; ++s) {
            const long long p = p0 + s * POINTS_BLOCK + t;
            const bool kept = points_kept(keep, bg, n, p, tl.HW);
            const unsigned long long bal = __ballot(kept);
            if (lane == 0) wsum[s & 1][wave] = __popcll(bal);
            __syncthreads();
            int woff = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < POINTS_WAVES; ++w) { const int x = wsum[s & 1][w]; if (w < wave) woff += x; tot += x; }
            const long long row = (long long)base + woff + __popcll(bal & ((1ull << lane) - 1ull));
            if (kept && (unsigned long long)row < (unsigned long long)tl.rows) {   // inside the buffers whatever prefix[] holds
                const int i = (int)p / W, j = (int)p - i * W;       // p < H * W <= 2^31 - 1
                const float2 f = flow[n * tl.HW + p];
                float2 a;
                a.x = f.x + 1.0f; a.x = a.x * sx; a.x = a.x / 2.0f;
                a.y = f.y + 1.0f; a.y = a.y * sy; a.y = a.y / 2.0f;
                i64x2 b;                                           // np.rot90(gridB, k)[i, j]
                if (k == 0) { b.x = j; b.y = i; }
                else if (k == 1) { b.x = wB - 1 - i; b.y = j; }
                else if (k == 2) { b.x = wB - 1 - j; b.y = hB - 1 - i; }
                else { b.x = i; b.y = hB - 1 - j; }
                pts1[row] = a;
                pts2[row] = b;
            }
            base += tot;
        }
    }
}

// (b) One thread per keypoint.  A point outside the map (the Python wrapper refuses it on the host) reads nothing: 0, 0, not kept.
__global__ __launch_bounds__(POINTS_BLOCK) void sample_points_kernel(const float2* __restrict__ flow, const float* __restrict__ match,
                                                                     const int32_t* __restrict__ xb, const int32_t* __restrict__ yb,
                                                                     int K, int H, int W, float sx, float sy, float* __restrict__ xa,
                                                                     float* __restrict__ ya, unsigned char* __restrict__ keep) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= K) return;
    const int x = xb[q], y = yb[q];
    float ox = 0.0f, oy = 0.0f;
    unsigned char kp = 0;
    if (x >= 0 && x < W && y >= 0 && y < H) {
        const long long i = (long long)y * W + x;
        const float2 f = flow[i];
        ox = f.x + 1.0f; ox = ox * 0.5f; ox = ox * sx;
        oy = f.y + 1.0f; oy = oy * 0.5f; oy = oy * sy;
        kp = match[i] > 0.5f ? 1 : 0;
    }
    xa[q] = ox;
    ya[q] = oy;
    keep[q] = kp;
}

PointsTiling points_tiling(int N, int H, int W) {
    PointsTiling tl;
    tl.HW = H * W;
    tl.per_map = (tl.HW + POINTS_TILE - 1) / POINTS_TILE;
    tl.tiles = (long long)N * tl.per_map;
    tl.rows = (long long)N * tl.HW;
    return tl;
}

}  // namespace

extern "C" size_t rfx_flow_points_ws_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    const size_t per_map = ((size_t)H * W + POINTS_TILE - 1) / POINTS_TILE;
    return sizeof(int) * (size_t)N * per_map;
}

extern "C" int rfx_flow_points_f32(const float* flow, const unsigned char* keep, const unsigned char* bg, int N, int H, int W, int k,
                                   int wA, int hA, int wB, int hB, float* pts1, long long* pts2, long long* offsets, void* ws,
                                   void* stream) {
    if (!flow || !keep || !pts1 || !pts2 || !offsets || !ws || N <= 0 || H <= 0 || W <= 0 || k < 0 || k > 3 || wA < 1 || hA < 1)
        return RFX_E_ARG;
    if ((k & 1) ? (H != wB || W != hB) : (H != hB || W != wB)) return RFX_E_ARG;
    if (!points_aligned(flow, 8) || !points_aligned(pts1, 8) || !points_aligned(pts2, 16) || !points_aligned(offsets, 8) ||
        !points_aligned(ws, 4))
        return RFX_E_ARG;
    if ((long long)N * H * W > 0x7fffffffLL) return RFX_E_LIMIT;
    hipStream_t st = rfx_stream(stream);
    const PointsTiling tl = points_tiling(N, H, W);
    int* counts = static_cast<int*>(ws);
    const int grid = (int)(tl.tiles < POINTS_GRID_CAP ? tl.tiles : POINTS_GRID_CAP);
    hipLaunchKernelGGL(points_count_kernel, dim3(grid), dim3(POINTS_BLOCK), 0, st, keep, bg, counts, tl);
    hipLaunchKernelGGL(points_scan_kernel, dim3(1), dim3(POINTS_SCAN_BLOCK), 0, st, counts, offsets, tl, N);
    hipLaunchKernelGGL(points_scatter_kernel, dim3(grid), dim3(POINTS_BLOCK), 0, st, reinterpret_cast<const float2*>(flow), keep, bg,
                       counts, reinterpret_cast<float2*>(pts1), reinterpret_cast<i64x2*>(pts2), tl, W, k, (float)(wA - 1),
                       (float)(hA - 1), wB, hB);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_sample_points_f32(const float* flow, const float* match, const int32_t* xb, const int32_t* yb, int K, int H, int W,
                                     int wA, int hA, float* xa, float* ya, unsigned char* keep, void* stream) {
    if (!flow || !match || !xb || !yb || !xa || !ya || !keep || K <= 0 || H <= 0 || W <= 0 || wA < 1 || hA < 1) return RFX_E_ARG;
    if (!points_aligned(flow, 8)) return RFX_E_ARG;
    if ((long long)H * W > 0x7fffffffLL) return RFX_E_LIMIT;
    hipLaunchKernelGGL(sample_points_kernel, dim3((K + POINTS_BLOCK - 1) / POINTS_BLOCK), dim3(POINTS_BLOCK), 0, rfx_stream(stream),
                       reinterpret_cast<const float2*>(flow), match, xb, yb, K, H, W, (float)(wA - 1), (float)(hA - 1), xa, ya, keep);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}
