// keypoints.hip -- the sparse-correspondence results step (evaluation/evalCorr/getResults.py: getFlow :78-136, alignmentError :15-38,
// the threshold loop :279-285; train/validation.py uses the same alignmentError) of a whole batch of pairs of any sizes, from the
// drivers' device records, without the dense maps: the protocol reads flowGlobal / matchGlobal at the annotated target pixels only.
// (a) rfx_records_keypoints_f32: one thread per keypoint of the batch.  The thread finds its pair by a binary search over the keypoint
//     table's first-keypoint column (as points_ragged.hip finds the map of a tile), evaluates the assembled maps at its pixel from the
//     record alone (assemble_pixel.h: the body of assemble_records_kernel's pixel loop) and transfers the point as
//     sample_points_kernel does.  No atomics, no LDS.
// (b) rfx_pck_tally_f64: one workgroup per (matchability threshold, pair): the float64 distances of the kept keypoints and their
//     tally under the pixel grid.  Ballots and popcounts per wavefront, one LDS pass, thread 0 writes; no atomics; integer sums.
// Built with -ffp-contract=off, like points.hip: every float32 and float64 step below is rounded on its own, in the order written.
#include "common.h"
#include "assemble_pixel.h"
#include "points_tile.h"

// this unit's own rule from here on, whatever the header above set or the command line says: a fused step in the distance would
// change its last bit.  (HIP's __dmul_rn / __dadd_rn are plain products and sums compiled under the command line's rule; the
// distance below is written as plain float64 operators under THIS pragma, which holds under any.)
#pragma clang fp contract(off)

namespace {

constexpr int KP_COLS = 4;       // keypoint table row: first keypoint | number of keypoints | wA | hA
constexpr int PCK_MAX_T = 16;    // thresholds of the pixel grid
constexpr int PCK_BLOCK = 256;
constexpr int PCK_WAVES = PCK_BLOCK / 64;

// The pair of keypoint q: the last row whose first keypoint is <= q (rows without keypoints share their first with the next row, so
// the last of them is the one that holds q).
__device__ __forceinline__ int keypoint_pair(const long long* __restrict__ ktable, int B, long long q) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ktable[(long long)mid * KP_COLS] <= q) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct RecKeypointArgs {
    const float* rec; const long long* table; const uint8_t* bg; const long long* ktable; const int32_t* xb; const int32_t* yb;
    float* xa; float* ya; float* m; uint8_t* flag;
    long long rec_elems, total_px, K_total;
    int width, max_h, off_H, off_flow, multiH, cycle, B; float th;
};

__global__ __launch_bounds__(POINTS_BLOCK) void records_keypoints_kernel(RecKeypointArgs a) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.K_total) return;
    float ox = 0.0f, oy = 0.0f, mv = 0.0f;
    uint8_t fl = 0;
    const int b = keypoint_pair(a.ktable, a.B, q);
    const long long* __restrict__ r = a.ktable + (long long)b * KP_COLS;
    const long long first = r[0], count = r[1], wA = r[2], hA = r[3];
    // a row that does not hold q, or without a source size, gives 0, 0, 0, 0 -- like a keypoint outside its map
    if (first >= 0 && q - first < count && wA >= 1 && hA >= 1 && wA <= 0x7fffffffLL && hA <= 0x7fffffffLL) {
        const RecPair k = rec_pair(a.rec, a.rec_elems, a.table, b, a.width, a.max_h, a.off_H, a.off_flow, a.multiH, a.total_px);
        const int x = a.xb[q], y = a.yb[q];
        if (k.ok && x >= 0 && x < k.W && y >= 0 && y < k.H) {
            const PixelResult p = assemble_pixel(k, y, x, a.cycle, a.th);
            // sample_points_kernel: add 1, halve, times (size - 1), each step rounded
            ox = __fmul_rn(__fmul_rn(__fadd_rn(p.flow.x, 1.0f), 0.5f), (float)(wA - 1));
            oy = __fmul_rn(__fmul_rn(__fadd_rn(p.flow.y, 1.0f), 0.5f), (float)(hA - 1));
            mv = p.match;
            const bool bin = p.found && (!a.bg || a.bg[k.out_off + (long long)y * k.W + x] != 0);
            const bool inside = p.flow.x >= -1.0f && p.flow.x <= 1.0f && p.flow.y >= -1.0f && p.flow.y <= 1.0f;
            fl = (uint8_t)((bin ? 1 : 0) | (inside ? 2 : 0));
        }
    }
    a.xa[q] = ox;
    a.ya[q] = oy;
    a.m[q] = mv;
    a.flag[q] = fl;
}

struct PckArgs {
    const float* xa; const float* ya; const float* m; const uint8_t* flag; const int32_t* xs; const int32_t* ys;
    const long long* ktable; const float* match_th; const double* grid; const uint8_t* valid;
    long long* counts; long long* nb; double* dist;
    long long K_total;
    int B, M, T;
};

// blockIdx.x = threshold index, blockIdx.y = pair.  Every thread of the workgroup walks the same trips, so each ballot sees whole
// wavefronts; a wavefront's tallies live in its (uniform) registers until the one LDS pass.
__global__ __launch_bounds__(PCK_BLOCK) void pck_tally_kernel(PckArgs a) {
    __shared__ int wsum[PCK_WAVES][PCK_MAX_T + 1];
    const int ti = blockIdx.x, b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6, T = a.T;
    const long long* __restrict__ r = a.ktable + (long long)b * KP_COLS;
    long long first = r[0], count = r[1];
    if (first < 0 || count < 0 || count > a.K_total || first > a.K_total - count) count = 0;     // a row outside the buffers: no keypoint
    const float mth = a.match_th[ti];
    const bool skip = a.valid && a.valid[b] == 0;        // the script's ``continue`` branch: every keypoint counts, none is measured
    int c[PCK_MAX_T + 1];
#pragma unroll
    for (int j = 0; j <= PCK_MAX_T; ++j) c[j] = 0;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (long long s = 0; s < count; s += PCK_BLOCK) {
        const long long i = s + t;
        bool keep = false;
        double d = nan;
        if (i < count && !skip) {
            const long long q = first + i;
            keep = mth > 0.0f ? (a.m[q] >= mth && (a.flag[q] & 2) != 0) : true;
            if (keep) {
                const double dx = (double)a.xa[q] - (double)a.xs[q], dy = (double)a.ya[q] - (double)a.ys[q];
                const double sx = dx * dx, sy = dy * dy;               // each product rounded, then their sum, then the root
                d = __dsqrt_rn(sx + sy);
            }
        }
        if (a.dist && i < count) a.dist[(long long)ti * a.K_total + first + i] = d;
        c[PCK_MAX_T] += __popcll(__ballot(keep));
#pragma unroll
        for (int j = 0; j < PCK_MAX_T; ++j)
            if (j < T) c[j] += __popcll(__ballot(keep && d <= a.grid[j]));      // (a uniform, cached read)
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j <= PCK_MAX_T; ++j) wsum[wave][j] = c[j];
    }
    __syncthreads();
    if (t == 0) {
        long long* __restrict__ out = a.counts + ((long long)ti * a.B + b) * T;
        for (int j = 0; j < T; ++j) {
            long long tot = 0;
            for (int w = 0; w < PCK_WAVES; ++w) tot += wsum[w][j];
            out[j] = tot;
        }
        long long kept = 0;
        for (int w = 0; w < PCK_WAVES; ++w) kept += wsum[w][PCK_MAX_T];
        a.nb[(long long)ti * a.B + b] = skip ? count : kept;
    }
}

}  // namespace

extern "C" int rfx_records_keypoints_f32(const float* rec, long long rec_elems, int width, int max_h, int off_H, int off_flow,
                                         const long long* table, int B, long long total_px, float th, int multiH, int cycle,
                                         const uint8_t* bg, const long long* ktable, const int32_t* xb, const int32_t* yb,
                                         long long K_total, float* xa, float* ya, float* m, uint8_t* flag, void* stream) {
    if (!rec || !table || !ktable || !xb || !yb || !xa || !ya || !m || !flag || B <= 0 || width <= 0 || max_h <= 0 || off_H < 1 ||
        off_flow < (long long)off_H + 9LL * max_h || off_flow > width || rec_elems < (long long)B * width || total_px <= 0 || K_total <= 0 ||
        !points_aligned(table, 8) || !points_aligned(ktable, 8))
        return RFX_E_ARG;
    if (B > 65535 || total_px > 0x7fffffffLL || K_total > 0x7fffffffLL) return RFX_E_LIMIT;
    const RecKeypointArgs a = {rec, table, bg, ktable, xb, yb, xa, ya, m, flag, rec_elems, total_px, K_total,
                               width, max_h, off_H, off_flow, multiH ? 1 : 0, cycle ? 1 : 0, B, th};
    hipLaunchKernelGGL(records_keypoints_kernel, dim3((unsigned)((K_total + POINTS_BLOCK - 1) / POINTS_BLOCK)), dim3(POINTS_BLOCK), 0,
                       rfx_stream(stream), a);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

extern "C" int rfx_pck_tally_f64(const float* xa, const float* ya, const float* m, const uint8_t* flag, const int32_t* xs,
                                 const int32_t* ys, const long long* ktable, int B, long long K_total, const float* match_th, int M,
                                 const double* grid, int T, const uint8_t* valid, long long* counts, long long* nb, double* dist,
                                 void* stream) {
    if (!ktable || !match_th || !grid || !counts || !nb || B <= 0 || M <= 0 || T <= 0 || T > 16 || K_total < 0 ||
        (K_total > 0 && (!xa || !ya || !m || !flag || !xs || !ys)) || !points_aligned(ktable, 8) || !points_aligned(grid, 8) ||
        !points_aligned(counts, 8) || !points_aligned(nb, 8) || !points_aligned(dist, 8))
        return RFX_E_ARG;
    if (B > 65535 || K_total > 0x7fffffffLL) return RFX_E_LIMIT;
    const PckArgs a = {xa, ya, m, flag, xs, ys, ktable, match_th, grid, valid, counts, nb, K_total > 0 ? dist : nullptr, K_total, B, M, T};
    hipLaunchKernelGGL(pck_tally_kernel, dim3(M, B), dim3(PCK_BLOCK), 0, rfx_stream(stream), a);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}
