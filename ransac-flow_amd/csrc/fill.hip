// fill.hip -- the nearest-explained-pixel fill of the KITTI flow assembly (evaluation/evalKITTI/getResults.py:87-93,
// interpolate_flow_match: scipy.ndimage.distance_transform_edt(~binary, return_indices=True), then flow[idx]) on the device.
// Every pixel of an (N,H,W,C) map takes the value of its nearest explained pixel, index for index what scipy returns:
//   the explained pixel (r', c') that minimises (r' - r)^2 + (c' - x)^2 -- an exact integer --, among equals the smallest column c',
//   among those the smallest row r';  a map without any explained pixel: scipy's index is (-1, 0) everywhere, which numpy's
//   indexing reads as pixel (H-1, 0).
// Two launches, ordered by the stream:
//   1. column pass: near[n,r,c] = the row of the nearest explained pixel in column c (ties: the smaller row), -1 if the column has
//      none.  One thread per (n, c) -- consecutive threads take consecutive columns, so mask reads coalesce --, a downward sweep that
//      carries the last explained row at or above, then an upward sweep that compares it with the nearest one at or below.
//   2. row pass + gather: a workgroup takes a 256-pixel segment of one (n, r) row.  It stages the whole row's vertical squared
//      distances v[c] = (near[n,r,c] - r)^2 in LDS (FILL_NONE for a column without explained pixel); each thread searches outward
//      from its pixel x over the candidates x-k, then x+k, with distance k^2 + v, and copies the C values of the winner.
// Integer work and a gather of 32-bit words: nothing is rounded, NaN payloads and -0.0 pass through bit for bit.
#include "common.h"

namespace {

constexpr int FILL_BLOCK = 256;
constexpr int FILL_MAX_W = 8192;                 // the staged row: 8192 int32 = 32 KB of LDS
constexpr int FILL_MAX_C = 8;
constexpr int FILL_NONE = 1 << 30;               // v of a column without explained pixel
// (H-1)^2 + (W-1)^2, the largest distance between two pixels, stays below FILL_NONE, and FILL_NONE + (W-1)^2 below 2^31
constexpr int FILL_MAX_H = 31728;
static_assert((long long)(FILL_MAX_H - 1) * (FILL_MAX_H - 1) + (long long)(FILL_MAX_W - 1) * (FILL_MAX_W - 1) < FILL_NONE, "sentinel");
static_assert((long long)FILL_NONE + (long long)(FILL_MAX_W - 1) * (FILL_MAX_W - 1) <= 0x7fffffffLL, "int32 distance");
constexpr int FILL_ROWS = 8;                     // rows whose loads one step of a column sweep issues together

// 1. One thread per (n, c).  Down: near = the last explained row at or above r (-1: none).  Up: dn = the nearest explained row at
// or below r; it replaces near where there is none above or it is STRICTLY closer -- at equal distance the smaller row, the one
// above, stays.  Both sweeps walk FILL_ROWS rows per step: their loads do not depend on each other and are issued together.
__global__ __launch_bounds__(FILL_BLOCK) void fill_columns_kernel(const unsigned char* __restrict__ explained, int* __restrict__ near,
                                                                  long long cols, int H, int W) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < cols; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / W;
        const long long org = n * H * W + (i - n * W);           // pixel (n, 0, c)
        int up = -1;
        for (int r0 = 0; r0 < H; r0 += FILL_ROWS) {
            unsigned char e[FILL_ROWS];
#pragma unroll
            for (int j = 0; j < FILL_ROWS; ++j) e[j] = r0 + j < H ? explained[org + (long long)(r0 + j) * W] : 0;
#pragma unroll
            for (int j = 0; j < FILL_ROWS; ++j) {
                if (r0 + j >= H) break;
                if (e[j]) up = r0 + j;
                near[org + (long long)(r0 + j) * W] = up;
            }
        }
        int dn = -1;
        for (int r0 = H - 1; r0 >= 0; r0 -= FILL_ROWS) {
            int a[FILL_ROWS];
#pragma unroll
            for (int j = 0; j < FILL_ROWS; ++j) a[j] = r0 - j >= 0 ? near[org + (long long)(r0 - j) * W] : -1;
#pragma unroll
            for (int j = 0; j < FILL_ROWS; ++j) {
                const int r = r0 - j;
                if (r < 0) break;
                if (a[j] == r) dn = r;                           // an explained pixel is its own nearest row above
                if (dn >= 0 && (a[j] < 0 || dn - r < r - a[j])) near[org + (long long)r * W] = dn;
            }
        }
    }
}

// Candidate column c of a search step (skipped when outside the row), at horizontal squared distance kk.  takes_ties: the
// candidate also wins at an EQUAL distance.
__device__ __forceinline__ void fill_try(const int* v, int W, int c, int kk, bool takes_ties, int& best, int& bc) {
    if (c < 0 || c >= W) return;
    const int d = kk + v[c];
    if (d < best || (takes_ties && d == best)) { best = d; bc = c; }
}

// 2. An item = (row of the batch, 256-pixel segment of it); a workgroup strides the grid over the items.  The search of pixel x
// keeps (best, bc) = the smallest distance so far and its column.  Step k tries x-k FIRST: its column is smaller than every column
// tried before, so it also wins at an equal distance; x+k second: the largest column so far, it has to be strictly closer.  That
// is "smaller distance, or equal distance and smaller column" for this order of candidates.  The search goes on while k^2 <= best
// -- at k^2 == best the candidate x-k in the pixel's own row (v = 0) still ties with a smaller column -- and while a candidate is
// in range; k < W bounds it whatever the data.  A row of FILL_NONE only (a map without explained pixel) ends with best >=
// FILL_NONE: source pixel (H-1, 0), index (-1, 0).
__global__ __launch_bounds__(FILL_BLOCK) void fill_rows_kernel(const uint32_t* __restrict__ values, const int* __restrict__ near,
                                                               uint32_t* __restrict__ out, int32_t* __restrict__ index,
                                                               long long rows, int H, int W, int C) {
    __shared__ int v[FILL_MAX_W];
    const int segs = (W + FILL_BLOCK - 1) / FILL_BLOCK;
    const long long items = rows * segs;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long row = it / segs;                          // n * H + r
        const int seg = (int)(it - row * segs);
        const long long n = row / H;
        const int r = (int)(row - n * H);
        const int* near_row = near + row * W;
        for (int c = threadIdx.x; c < W; c += FILL_BLOCK) {
            const int a = near_row[c];
            v[c] = a < 0 ? FILL_NONE : (a - r) * (a - r);
        }
        __syncthreads();
        const int x = seg * FILL_BLOCK + threadIdx.x;
        if (x < W) {
            int best = v[x], bc = x;
            for (int k = 1; k < W; ++k) {
                const int kk = k * k;
                if (kk > best || (x - k < 0 && x + k >= W)) break;
                fill_try(v, W, x - k, kk, true, best, bc);
                fill_try(v, W, x + k, kk, false, best, bc);
            }
            const bool none = best >= FILL_NONE;
            const int sr = none ? H - 1 : near_row[bc];
            const int sc = none ? 0 : bc;
            const uint32_t* src = values + ((n * H + sr) * W + sc) * C;
            uint32_t* dst = out + (row * W + x) * C;
            for (int c = 0; c < C; ++c) dst[c] = src[c];
            if (index) {
                index[((n * 2 + 0) * H + r) * W + x] = none ? -1 : sr;
                index[((n * 2 + 1) * H + r) * W + x] = sc;
            }
        }
        __syncthreads();                                          // the next item restages v
    }
}

}  // namespace

extern "C" size_t rfx_nearest_fill_ws_bytes(int N, int H, int W) {
    return N > 0 && H > 0 && W > 0 ? sizeof(int) * (size_t)N * H * W : 0;
}

extern "C" int rfx_nearest_fill_f32(const float* values, const unsigned char* explained, float* out, int32_t* index, int N, int H,
                                    int W, int C, void* ws, void* stream) {
    if (!values || !explained || !out || !ws || N <= 0 || H <= 0 || W <= 0 || C <= 0 || out == values) return RFX_E_ARG;
    if (W > FILL_MAX_W || H > FILL_MAX_H || C > FILL_MAX_C) return RFX_E_LIMIT;
    hipStream_t st = rfx_stream(stream);
    int* near = static_cast<int*>(ws);
    const long long cols = (long long)N * W, rows = (long long)N * H;
    const long long items = rows * ((W + FILL_BLOCK - 1) / FILL_BLOCK);
    const int gc = (int)((cols + FILL_BLOCK - 1) / FILL_BLOCK < 8192 ? (cols + FILL_BLOCK - 1) / FILL_BLOCK : 8192);
    const int gr = (int)(items < 8192 ? items : 8192);
    hipLaunchKernelGGL(fill_columns_kernel, dim3(gc), dim3(FILL_BLOCK), 0, st, explained, near, cols, H, W);
    hipLaunchKernelGGL(fill_rows_kernel, dim3(gr), dim3(FILL_BLOCK), 0, st, reinterpret_cast<const uint32_t*>(values), near,
                       reinterpret_cast<uint32_t*>(out), index, rows, H, W, C);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}
