// assemble_pixel.h -- one pixel of the offline flow assembly (evaluation/evalHpatch/getResults.py:16-63, evalCorr/getResults.py:78-136,
// evalYFCC/getResults.py:150-190) from a driver's result record alone: the device helpers assemble_records_kernel (warp.hip) walks a
// record with, shared with the kernels that read the assembled maps at a few pixels only (keypoints.hip).
// The helpers' expressions are written as the chain's kernels in warp.hip are compiled, with that unit's contraction rule: the pragma
// below keeps it for every unit that includes this header, whatever -ffp-contract the unit is built with (the float steps of
// assemble_pixel itself are spelled out -- __fmul_rn / __fadd_rn / fmaf -- and depend on neither).
#pragma once
#include "common.h"
#include "linspace.h"
#include <math.h>

#pragma clang fp contract(fast)      // a unit built with another rule states its own again after the include (keypoints.hip)

namespace {

__device__ __forceinline__ float unnormalize(float g, int size, int align) {
    return align ? (g + 1.0f) * 0.5f * (float)(size - 1) : ((g + 1.0f) * (float)size - 1.0f) * 0.5f;
}

struct Corners {
    int x0, y0;
    float nw, ne, sw, se;
    bool m_nw, m_ne, m_sw, m_se;
};

// ATen grid_sampler_2d (bilinear, zeros): weights from the fractional parts, out-of-image corners contribute 0.
__device__ __forceinline__ Corners corners(float gx, float gy, int Hi, int Wi, int align) {
    Corners c;
    const float ix = unnormalize(gx, Wi, align), iy = unnormalize(gy, Hi, align);
    const float xw = floorf(ix), yn = floorf(iy);
    const float w = ix - xw, e = 1.0f - w, n = iy - yn, s = 1.0f - n;
    c.nw = s * e; c.ne = s * w; c.sw = n * e; c.se = n * w;
    // NaN / +-inf / huge coordinates: the comparisons below are all false -> the pixel is 0, as in ATen's CUDA grid_sampler (its
    // within-bounds masks); ATen's CPU kernel returns NaN for NaN / +-inf coordinates and is not followed.  The (int) conversion
    // further down is applied only to a floor that passed a range test (tests/test_gpu_pointwise_exact.py pins all of this).
    const bool xin0 = xw >= 0.0f && xw <= (float)(Wi - 1), xin1 = xw + 1.0f >= 0.0f && xw + 1.0f <= (float)(Wi - 1);
    const bool yin0 = yn >= 0.0f && yn <= (float)(Hi - 1), yin1 = yn + 1.0f >= 0.0f && yn + 1.0f <= (float)(Hi - 1);
    c.m_nw = xin0 && yin0; c.m_ne = xin1 && yin0; c.m_sw = xin0 && yin1; c.m_se = xin1 && yin1;
    c.x0 = (xin0 || xin1) ? (int)xw : 0;
    c.y0 = (yin0 || yin1) ? (int)yn : 0;
    return c;
}

// kornia's warp_grid at integer pixel (x, y) of an h x w grid: M (px, py, 1) divided by its third component
__device__ __forceinline__ float2 warp_point(const float* __restrict__ M, int x, int y, int h, int w) {
    const float px = rfx_lin(x, w), py = rfx_lin(y, h);
    // (x', y', z') = M (px, py, 1): k-ordered fma chain like a K=3 sgemm
    const float xs = fmaf(1.0f, M[2], fmaf(py, M[1], __fmul_rn(px, M[0])));
    const float ys = fmaf(1.0f, M[5], fmaf(py, M[4], __fmul_rn(px, M[3])));
    const float zs = fmaf(1.0f, M[8], fmaf(py, M[7], __fmul_rn(px, M[6])));
    float2 o;
    o.x = xs / zs;
    o.y = ys / zs;
    return o;
}

__device__ __forceinline__ float src_index(float scale, int dst) {  // align_corners=False
    const float s = scale * ((float)dst + 0.5f) - 0.5f;
    return s < 0.f ? 0.f : s;
}

// the taps of resize_bilinear_body (align_corners = 0) at one output pixel: the upper left tap's offset inside a plane, the steps to
// the clamped right and lower neighbours and the two fractions
struct UpTap { int o00, dx, dy; float lx, ly; };

__device__ __forceinline__ UpTap up_tap(float sh, float sw, int y, int x, int hd, int wd) {
    UpTap t;
    const float fy = src_index(sh, y), fx = src_index(sw, x);
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 < hd - 1 ? y0 : hd - 1;          // (never taken by an index the rule above produces: keeps every read inside the plane)
    x0 = x0 < wd - 1 ? x0 : wd - 1;
    t.ly = fy - (float)y0;
    t.lx = fx - (float)x0;
    t.o00 = y0 * wd + x0;
    t.dx = x0 < wd - 1 ? 1 : 0;
    t.dy = y0 < hd - 1 ? wd : 0;
    return t;
}

// resize_bilinear_body's per-sample expression, operation for operation
__device__ __forceinline__ float up_resize(const float* __restrict__ plane, const UpTap& t) {
    const float* q = plane + t.o00;
    const float v00 = q[0], v01 = q[t.dx], v10 = q[t.dy], v11 = q[t.dy + t.dx];
    const float hy = 1.f - t.ly, hx = 1.f - t.lx;
    const float r0 = fmaf(v01, t.lx, __fmul_rn(v00, hx));
    const float r1 = fmaf(v11, t.lx, __fmul_rn(v10, hx));
    return fmaf(r1, t.ly, __fmul_rn(r0, hy));
}

// compose_flow_body's up-sampling of one residual-flow channel: hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11), contracted
// as compose_flow_kernel is (the second product of every sum fused)
__device__ __forceinline__ float up_flow(const float* __restrict__ plane, const UpTap& t) {
    const float* q = plane + t.o00;
    const float v00 = q[0], v01 = q[t.dx], v10 = q[t.dy], v11 = q[t.dy + t.dx];
    const float hy = 1.f - t.ly, hx = 1.f - t.lx;
    const float top = fmaf(t.lx, v01, __fmul_rn(hx, v00));
    const float bot = fmaf(t.lx, v11, __fmul_rn(hx, v10));
    return fmaf(hy, top, __fmul_rn(t.ly, bot));
}

// One pair of a batch of records: row b of the (B,8) table of rfx_assemble_records_f32, checked.
//     row offset in rec | h8 | w8 | off_match | H | W | offset of the pair's pixels in the packed maps | 0
// ok == false for a row that does not describe a record inside rec and a map inside [0, total_px): nothing of it is read or written.
struct RecPair {
    const float* Hm; const float* flowDown; const float* matchDown;
    long long out_off;
    int hd, wd, H, W, HW, last;              // last: the homographies the walk may visit (nbH, or min(nbH, 1) without multiH)
    float sh, sw;
    bool ok;
};

__device__ __forceinline__ RecPair rec_pair(const float* __restrict__ rec, long long rec_elems, const long long* __restrict__ table,
                                            int b, int width, int max_h, int off_H, int off_flow, int multiH, long long total_px) {
    const long long* __restrict__ T = table + (long long)b * 8;
    const long long row_off = T[0], h8l = T[1], w8l = T[2], off_match = T[3], Hl = T[4], Wl = T[5], out_off = T[6];
    RecPair k;
    k.ok = false;
    if (row_off < 0 || row_off + width > rec_elems || h8l <= 0 || w8l <= 0 || h8l > width || w8l > width || Hl <= 0 ||
        Wl <= 0 || Hl > 0x7fffffffLL || Wl > 0x7fffffffLL || Hl * Wl > 0x7fffffffLL)
        return k;
    const long long n8 = 2 * h8l * w8l * max_h, HWl = Hl * Wl;
    if (off_match < off_flow + n8 || off_match + n8 > width || out_off < 0 || out_off + HWl > total_px) return k;
    k.hd = (int)h8l; k.wd = (int)w8l; k.H = (int)Hl; k.W = (int)Wl; k.HW = (int)HWl;
    const float* __restrict__ row = rec + row_off;
    k.Hm = row + off_H; k.flowDown = row + off_flow; k.matchDown = row + off_match;
    k.out_off = out_off;
    const float nf = row[0];                                   // nbH, a small integer held as a float
    const int nb = nf >= 1.0f ? (nf < (float)max_h ? (int)nf : max_h) : 0;
    k.last = multiH ? nb : (nb < 1 ? nb : 1);
    k.sh = (float)k.hd / (float)k.H; k.sw = (float)k.wd / (float)k.W;
    k.ok = true;
    return k;
}

// flowGlobal, matchGlobal and the explained bit (before any background mask) of pixel (y, x) of pair k: the walk over homographies
// 0..last-1 in the merge's order, stopping at the owner -- per homography what rfx_warp_grid_f32 -> rfx_compose_flow_f32(clamp, inb
// [, flowUp]) -> rfx_resize_bilinear_f32 [-> rfx_grid_sample_f32] give at the pixel, then rfx_merge_multi_h_f32's owner rule and its
// final clamp.  The coarse grid of a homography is not stored: a tap of its bilinear sample is warp_grid_body's expression at the
// tap's integer pixel.  A pair without a homography (last == 0) gives 0, 0, false.
struct PixelResult { float2 flow; float match; bool found; };

__device__ __forceinline__ PixelResult assemble_pixel(const RecPair& k, const int y, const int x, const int cycle, const float th) {
    const int hd = k.hd, wd = k.wd, H = k.H, W = k.W, hw = hd * wd, last = k.last;
    const float sh = k.sh, sw = k.sw;
    const float* __restrict__ Hm = k.Hm;
    const float* __restrict__ flowDown = k.flowDown;
    const float* __restrict__ matchDown = k.matchDown;
    const UpTap t = up_tap(sh, sw, y, x, hd, wd);
    float2 fbest;
    fbest.x = 0.0f; fbest.y = 0.0f;
    float mbest = 0.0f;
    bool found = false;
    for (int i = 0; i < last; ++i) {
        // compose_flow (clamp = 1) on homography i's grid: the sampling point, flow_i, the in-bounds mask
        const float* f = flowDown + (size_t)i * 2 * hw;
        float gx = __fadd_rn(up_flow(f, t), rfx_lin(x, W)), gy = __fadd_rn(up_flow(f + hw, t), rfx_lin(y, H));
        gx = fminf(fmaxf(gx, -1.0f), 1.0f);
        gy = fminf(fmaxf(gy, -1.0f), 1.0f);
        const Corners c = corners(gx, gy, H, W, 0);
        const float* M = Hm + i * 9;
        float ox = 0.f, oy = 0.f;
        if (c.m_nw) { const float2 v = warp_point(M, c.x0, c.y0, H, W); ox = fmaf(v.x, c.nw, ox); oy = fmaf(v.y, c.nw, oy); }
        if (c.m_ne) { const float2 v = warp_point(M, c.x0 + 1, c.y0, H, W); ox = fmaf(v.x, c.ne, ox); oy = fmaf(v.y, c.ne, oy); }
        if (c.m_sw) { const float2 v = warp_point(M, c.x0, c.y0 + 1, H, W); ox = fmaf(v.x, c.sw, ox); oy = fmaf(v.y, c.sw, oy); }
        if (c.m_se) { const float2 v = warp_point(M, c.x0 + 1, c.y0 + 1, H, W); ox = fmaf(v.x, c.se, ox); oy = fmaf(v.y, c.se, oy); }
        const float inb = (ox >= -1.0f && ox <= 1.0f && oy >= -1.0f && oy <= 1.0f) ? 1.0f : 0.0f;
        // resize_bilinear of match12Down8 at the pixel; with the cycle check, grid_sample of the up-sampled match21 at (gx, gy):
        // the map has the grid's size, so the taps and weights are c's, each tap the resize expression at its integer pixel
        const float* m12 = matchDown + (size_t)i * 2 * hw;
        float v = up_resize(m12, t);
        if (cycle) {
            const float* s21 = m12 + hw;
            float cyc = 0.0f;
            if (c.m_nw) cyc = fmaf(up_resize(s21, up_tap(sh, sw, c.y0, c.x0, hd, wd)), c.nw, cyc);
            if (c.m_ne) cyc = fmaf(up_resize(s21, up_tap(sh, sw, c.y0, c.x0 + 1, hd, wd)), c.ne, cyc);
            if (c.m_sw) cyc = fmaf(up_resize(s21, up_tap(sh, sw, c.y0 + 1, c.x0, hd, wd)), c.sw, cyc);
            if (c.m_se) cyc = fmaf(up_resize(s21, up_tap(sh, sw, c.y0 + 1, c.x0 + 1, hd, wd)), c.se, cyc);
            v = __fmul_rn(v, cyc);
        }
        v = __fmul_rn(v, inb);                             // score_i = match12 (* cycle) * in-bounds, left to right
        // merge_multi_h_kernel's rule: 0 owns the pixel unless a later homography is the first to reach th
        if (i == 0) { mbest = v; fbest.x = ox; fbest.y = oy; }
        if (v >= th) {
            mbest = v; fbest.x = ox; fbest.y = oy;
            found = true;
            break;
        }
    }
    // torch.clamp: a NaN stays a NaN (merge_multi_h_kernel)
    PixelResult r;
    r.flow.x = fbest.x < -1.0f ? -1.0f : (fbest.x > 1.0f ? 1.0f : fbest.x);
    r.flow.y = fbest.y < -1.0f ? -1.0f : (fbest.y > 1.0f ? 1.0f : fbest.y);
    r.match = mbest;
    r.found = found;
    return r;
}

}  // namespace
