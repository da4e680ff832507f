// epe.hip -- the end-point error the HPatches and KITTI results scripts take of an assembled flow, on the device.
// (a) rfx_epe_homography_f32: evaluation/evalHpatch/getResults.py:83-144 (getGT), :147-156 (epe) and the statements :221-250 between
//     them.  The ground-truth map of one 3x3 homography is formed per pixel and never stored:
//       1. (X, Y) = (j, i) as float64; (xw, yw, zw) = Hinv (X, Y, 1) in float64, each row as (h0 * X + h1 * Y) + h2: two rounded
//          products, added left to right, then the third entry (the product with 1 is exact) -- no fused step;
//       2. xw, yw, zw rounded to float32;
//       3. gx = ((2 * xw) / (zw + 1e-8f)) / (float)(S_w - 1) - 1, every step float32; gy with yw and S_h - 1;
//       4. inside iff -1 <= gx <= 1 and -1 <= gy <= 1 (a NaN is outside);
//       5. both maps to pixels: t = v + 1; t = t * (float)(S - 1); t = t / 2 (S_w for x, S_h for y);
//       6. err = sqrtf(fmaf(dy, dy, dx * dx)): torch.norm(p=2, dim=1) of a two-element row on the CPU.
// (b) rfx_epe_flow_f32: evaluation/evalKITTI/getResults.py:221-228.  up = ((fx - lin(j, W)) * (float)(W - 1)) / 2 in float32 steps
//     (lin = torch.linspace(-1, 1, W), linspace.h), vp with H; dx = (double)up - (double)u, dy likewise;
//     err = sqrt(dx * dx + dy * dy) in float64; counted iff valid != 0.
// Both reduce the same way, in two launches ordered by the stream; no floating-point atomic, no workgroup waits on another:
//   1. tiles:  a workgroup takes a tile of EPE_TILE consecutive pixels of ONE map (tiles never straddle two maps).  A thread adds its
//              EPE_PASSES pixels in pass order (float64; a pixel that is not counted adds +0.0, which changes nothing), a wavefront
//              adds its 64 lanes by the fixed tree of __shfl_down 32, 16, ... 1, thread 0 adds the four wavefronts in order and writes
//              the tile's sum and count to the workspace;
//   2. finish: ONE wavefront per map adds the map's tile sums in index order, 64 at a time (a coalesced read into LDS, then lane 0
//              one by one).
// The order of every addition depends on the pixel's place in its map alone: a map's sum has the same bits run after run, alone or
// at any position of a batch.
// Built with -ffp-contract=off (only the fmaf written here fuses) and -fhip-fp32-correctly-rounded-divide-sqrt (the float32
// divisions and root round like ATen's on the CPU).
#include "common.h"
#include "linspace.h"
#include <math.h>

namespace {

constexpr int EPE_BLOCK = 256;                   // 4 wavefronts
constexpr int EPE_PASSES = 4;
constexpr int EPE_TILE = EPE_BLOCK * EPE_PASSES;
constexpr int EPE_WAVES = EPE_BLOCK / 64;
constexpr int EPE_GRID_CAP = 8192;               // workgroups stride over the tiles (finish: the maps) beyond it

struct EpeTiling {
    long long tiles;     // N * per_map
    int per_map;         // ceil(H * W / EPE_TILE)
    int HW;
};

// Per-pixel rules: pixel(n, p, e) -> counted?, e = the error as float64 (exact for the float32 rule); stores err[n, p] if asked to.
struct HomographyRule {
    const float2* __restrict__ flow;
    const double* __restrict__ Hinv;
    float* __restrict__ err;
    int W, HW;
    float sx, sy;        // (float)(S_w - 1), (float)(S_h - 1)

    __device__ __forceinline__ bool pixel(long long n, int p, double& e) const {
        const double* __restrict__ h = Hinv + n * 9;
        const int i = p / W, j = p - i * W;
        const double X = (double)j, Y = (double)i;
        const float xw = (float)((h[0] * X + h[1] * Y) + h[2]);
        const float yw = (float)((h[3] * X + h[4] * Y) + h[5]);
        const float zw = (float)((h[6] * X + h[7] * Y) + h[8]);
        const float z = zw + 1e-8f;
        float gx = 2.0f * xw; gx = gx / z; gx = gx / sx; gx = gx - 1.0f;
        float gy = 2.0f * yw; gy = gy / z; gy = gy / sy; gy = gy - 1.0f;
        const bool inside = gx >= -1.0f && gx <= 1.0f && gy >= -1.0f && gy <= 1.0f;
        float r = __builtin_nanf("");
        if (inside) {
            const float2 f = flow[n * HW + p];
            float tx = gx + 1.0f; tx = tx * sx; tx = tx / 2.0f;
            float ty = gy + 1.0f; ty = ty * sy; ty = ty / 2.0f;
            float ex = f.x + 1.0f; ex = ex * sx; ex = ex / 2.0f;
            float ey = f.y + 1.0f; ey = ey * sy; ey = ey / 2.0f;
            const float dx = tx - ex, dy = ty - ey;
            r = sqrtf(fmaf(dy, dy, dx * dx));
        }
        if (err) err[n * HW + p] = r;
        e = (double)r;
        return inside;
    }
};

struct FlowRule {
    const float2* __restrict__ flow;
    const float* __restrict__ u;
    const float* __restrict__ v;
    const unsigned char* __restrict__ valid;
    double* __restrict__ err;
    int H, W, HW;
    float sx, sy;        // (float)(W - 1), (float)(H - 1)

    __device__ __forceinline__ bool pixel(long long n, int p, double& e) const {
        const long long q = n * HW + p;
        const bool counted = valid[q] != 0;
        double r = __builtin_nan("");
        if (counted) {
            const int i = p / W, j = p - i * W;
            const float2 f = flow[q];
            float up = f.x - rfx_lin(j, W); up = up * sx; up = up / 2.0f;
            float vp = f.y - rfx_lin(i, H); vp = vp * sy; vp = vp / 2.0f;
            const double dx = (double)up - (double)u[q], dy = (double)vp - (double)v[q];
            r = sqrt(dx * dx + dy * dy);
        }
        if (err) err[q] = r;
        e = r;
        return counted;
    }
};

// 1. psum[tile], pcount[tile].  Pass s of a tile looks at pixels tile * EPE_TILE + s * 256 + threadIdx.x of its map.
template <class Rule>
__global__ __launch_bounds__(EPE_BLOCK) void epe_tiles_kernel(Rule rule, double* __restrict__ psum, int* __restrict__ pcount,
                                                              EpeTiling tl) {
    __shared__ double wsum[EPE_WAVES];
    __shared__ int wcnt[EPE_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (long long tile = blockIdx.x; tile < tl.tiles; tile += gridDim.x) {
        const long long n = tile / tl.per_map;
        const long long p0 = (tile - n * tl.per_map) * EPE_TILE;
        double acc = 0.0;
        int c = 0;
#pragma unroll
        for (int s = 0; s < EPE_PASSES; ++s) {
            const long long p = p0 + s * EPE_BLOCK + t;
            double e = 0.0;
            const bool counted = p < tl.HW && rule.pixel(n, (int)p, e);    // p < H * W <= 2^31 - 1
            acc += counted ? e : 0.0;
            c += __popcll(__ballot(counted));
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d);      // lane 0 ends with the whole fixed tree
        if (lane == 0) { wsum[wave] = acc; wcnt[wave] = c; }
        __syncthreads();
        if (t == 0) {
            double tot = wsum[0];
            int cnt = wcnt[0];
#pragma unroll
            for (int w = 1; w < EPE_WAVES; ++w) { tot += wsum[w]; cnt += wcnt[w]; }
            psum[tile] = tot;
            pcount[tile] = cnt;
        }
        __syncthreads();                                           // the next tile rewrites wsum / wcnt
    }
}

// 2. sum[n] = psum[n * per_map + 0] + ... in index order; count[n] likewise (<= H * W: int32 holds it).  One wavefront per map: lane l
// of trip k stages partial k + l in LDS (0 past the map's last tile: adding +0.0 is exact), then lane 0 adds the 64 values in order.
__global__ __launch_bounds__(64) void epe_finish_kernel(const double* __restrict__ psum, const int* __restrict__ pcount,
                                                        double* __restrict__ sum, int* __restrict__ count, int N, int per_map) {
    __shared__ double vs[64];
    __shared__ int cs[64];
    const int lane = threadIdx.x;
    for (long long n = blockIdx.x; n < N; n += gridDim.x) {
        const double* __restrict__ ps = psum + n * per_map;
        const int* __restrict__ pc = pcount + n * per_map;
        double s = 0.0;
        int c = 0;
        for (int k = 0; k < per_map; k += 64) {
            const bool in = k + lane < per_map;
            vs[lane] = in ? ps[k + lane] : 0.0;
            cs[lane] = in ? pc[k + lane] : 0;
            __syncthreads();
            if (lane == 0) {
#pragma unroll 16
                for (int l = 0; l < 64; ++l) { s += vs[l]; c += cs[l]; }
            }
            __syncthreads();                                       // the next trip rewrites vs / cs
        }
        if (lane == 0) { sum[n] = s; count[n] = c; }
    }
}

EpeTiling epe_tiling(int N, int H, int W) {
    EpeTiling tl;
    tl.HW = H * W;
    tl.per_map = (int)(((long long)tl.HW + EPE_TILE - 1) / EPE_TILE);   // H * W may be within a tile of 2^31
    tl.tiles = (long long)N * tl.per_map;
    return tl;
}

bool epe_aligned(const void* p, size_t a) { return ((size_t)p & (a - 1)) == 0; }

template <class Rule>
int epe_launch(const Rule& rule, int N, const EpeTiling& tl, double* sum, int32_t* count, void* ws, hipStream_t st) {
    double* psum = static_cast<double*>(ws);
    int* pcount = reinterpret_cast<int*>(psum + tl.tiles);
    const int grid = (int)(tl.tiles < EPE_GRID_CAP ? tl.tiles : EPE_GRID_CAP);
    hipLaunchKernelGGL(epe_tiles_kernel<Rule>, dim3(grid), dim3(EPE_BLOCK), 0, st, rule, psum, pcount, tl);
    hipLaunchKernelGGL(epe_finish_kernel, dim3(N < EPE_GRID_CAP ? N : EPE_GRID_CAP), dim3(64), 0, st, psum, pcount, sum, count, N,
                       tl.per_map);
    RFX_LAUNCH_CHECK();
    return RFX_OK;
}

}  // namespace

extern "C" size_t rfx_epe_ws_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    const size_t per_map = ((size_t)H * W + EPE_TILE - 1) / EPE_TILE;
    return (sizeof(double) + sizeof(int)) * (size_t)N * per_map;
}

extern "C" int rfx_epe_homography_f32(const float* flow, const double* Hinv, int N, int Sh, int Sw, double* sum, int32_t* count,
                                      float* err, void* ws, void* stream) {
    if (!flow || !Hinv || !sum || !count || !ws || N <= 0 || Sh < 2 || Sw < 2) return RFX_E_ARG;
    if (!epe_aligned(flow, 8) || !epe_aligned(Hinv, 8) || !epe_aligned(sum, 8) || !epe_aligned(ws, 8) || !epe_aligned(count, 4) ||
        !epe_aligned(err, 4))
        return RFX_E_ARG;
    if ((long long)N * Sh * Sw > 0x7fffffffLL) return RFX_E_LIMIT;
    const EpeTiling tl = epe_tiling(N, Sh, Sw);
    const HomographyRule rule = {reinterpret_cast<const float2*>(flow), Hinv, err, Sw, tl.HW, (float)(Sw - 1), (float)(Sh - 1)};
    return epe_launch(rule, N, tl, sum, count, ws, rfx_stream(stream));
}

extern "C" int rfx_epe_flow_f32(const float* flow, const float* u, const float* v, const unsigned char* valid, int N, int H, int W,
                                double* sum, int32_t* count, double* err, void* ws, void* stream) {
    if (!flow || !u || !v || !valid || !sum || !count || !ws || N <= 0 || H <= 0 || W <= 0) return RFX_E_ARG;
    if (!epe_aligned(flow, 8) || !epe_aligned(u, 4) || !epe_aligned(v, 4) || !epe_aligned(sum, 8) || !epe_aligned(ws, 8) ||
        !epe_aligned(count, 4) || !epe_aligned(err, 8))
        return RFX_E_ARG;
    if ((long long)N * H * W > 0x7fffffffLL) return RFX_E_LIMIT;
    const EpeTiling tl = epe_tiling(N, H, W);
    const FlowRule rule = {reinterpret_cast<const float2*>(flow), u, v, valid, err, H, W, tl.HW, (float)(W - 1), (float)(H - 1)};
    return epe_launch(rule, N, tl, sum, count, ws, rfx_stream(stream));
}
